"""Launch lists: the C-ABI calls, stream hand-overs and bucket markers of a step, recorded once with their arguments already
marshalled and replayed afterwards (why: the comment at Engine.use_launch_lists).

Nothing here needs a GPU or torch: library entry points are callables that return a status, events and streams are whatever
offers record(stream) / wait_event(event).  Engine records through a Recorder (Engine._rec), keeps the finished lists in
_Buffers.launch_lists and replays them with replay(); how a launch is instrumented for a measurement (`around`) is the same
callable on the replayed and on the eager path (Engine._launch)."""
from typing import NamedTuple

LAUNCH, HAND_OVER, BUCKET_READY, EAGER = range(4)
_KIND, _FN, _ARGS = 0, 1, 2  # every op record starts with its kind; Launch and Eager go on with fn and args (replay's hot loop)


class HipLibraryError(RuntimeError):
    pass


def raise_status(name, rc, last_error):
    """the one place a non-zero status of library entry point `name` becomes an exception (last_error: callable -> text)"""
    raise HipLibraryError("{} failed with status {}: {}".format(name, rc, last_error()))


class Launch(NamedTuple):
    """one C-ABI call: the raw entry point, its marshalled arguments, its name, the logical kernel instance it is (tag, e.g.
    'fwd:big_conv_1') and the stream it was enqueued on"""
    kind: int
    fn: object
    args: tuple
    name: str
    tag: str
    stream: object


class HandOver(NamedTuple):
    """dst waits for everything enqueued on src so far"""
    kind: int
    event: object
    src: object
    dst: object


class BucketReady(NamedTuple):
    """every launch that writes gradient bucket `bucket` is enqueued: the replay's callback gets the index"""
    kind: int
    bucket: int


class Eager(NamedTuple):
    """a step of the sequence that has to be marshalled afresh every time (pointers / sizes that change per batch)"""
    kind: int
    fn: object
    args: tuple


class Recorder(list):
    """A launch list while it is recorded and afterwards: the ops in order; last_error is the library's error text."""

    def __init__(self, last_error):
        super().__init__()
        self.last_error = last_error

    def launch(self, fn, args, name, tag, stream):
        self.append(Launch(LAUNCH, fn, args, name, tag, stream))

    def hand_over(self, event, src, dst):
        self.append(HandOver(HAND_OVER, event, src, dst))

    def bucket_ready(self, b):
        self.append(BucketReady(BUCKET_READY, b))

    def eager(self, fn, args):
        self.append(Eager(EAGER, fn, args))


def entry_points(ops):
    """(entry-point name, tag) of every launch of a recorded list, in order"""
    return [(op.name, op.tag) for op in ops if op.kind == LAUNCH]


def replay(ops, callback=None, around=None):
    """Runs a recorded list.  around=None is the timed region: a tight loop, nothing per op but its own call.  Otherwise every
    launch goes through around(fn, args, tag, stream) -> status (timed / profiled below) -- the same loop over a copy of the
    list with its launches wrapped: the step still runs from its recorded lists.  Marshalled eagerly, the Python between the
    launches starves the GPU and the MFMA-bound kernels behind the gaps run at other clocks (round 5: their durations came out
    17 % above the kernel's own timestamps)."""
    if around is not None:
        plain, ops = ops, Recorder(ops.last_error)
        ops.extend(op._replace(fn=lambda *args, op=op: around(op.fn, args, op.tag, op.stream)) if op.kind == LAUNCH else op
                   for op in plain)
    # (by position: a named field costs 30 ns more per access, which showed in the host-bound configuration-5 step)
    kind_at, fn_at, args_at = _KIND, _FN, _ARGS
    for op in ops:
        kind = op[kind_at]
        if kind == LAUNCH:
            rc = op[fn_at](*op[args_at])
            if rc != 0:
                raise_status(op.name, rc, ops.last_error)
        elif kind == HAND_OVER:
            op.event.record(op.src)
            op.dst.wait_event(op.event)
        elif kind == BUCKET_READY:
            callback(op.bucket)
        else:
            op[fn_at](*op[args_at])


def timed(out, new_event):
    """around= of the per-launch timeline: events (new_event(): timestamps only, _hipevents.TimingEvent) on the launch's own
    stream around every C-ABI call -- bias passes run on the side stream; stream None = the current one -- and one
    (tag, start, stop) per launch appended to `out`"""
    def around(fn, args, tag, stream):
        start, stop = new_event(), new_event()
        start.record(stream)
        rc = fn(*args)
        stop.record(stream)
        out.append((tag, start, stop))
        return rc
    return around


def profiled(tags, out, new_event, attach):
    """around= of the profiled-kernel mode: events immediately around the MAIN kernel of the launches whose tag is in `tags`
    (attach(start, stop): sl_profile_next_kernel), none anywhere else -- the step runs as in the timed region and the duration
    is what rocprofv3 reports for that kernel"""
    def around(fn, args, tag, stream):
        if tag in tags:
            start, stop = new_event(), new_event()
            start.record()  # creates the HIP events; the library records them again around the kernel's dispatch
            stop.record()
            attach(start, stop)
            out.append((tag, start, stop))
        return fn(*args)
    return around
