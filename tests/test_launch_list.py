"""speechless_amd/launch_list.py with fakes (no GPU): what is recorded is what is replayed, in all three launch modes, and
_Buffers.grow drops the recorded lists exactly when it re-allocates."""
import pytest

from speechless_amd import launch_list as ll


class FakeStream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_event(self, event):
        self.log.append(("wait", self, event))


class FakeEvent:
    def __init__(self, log):
        self.log = log

    def record(self, stream=None):
        self.log.append(("record", self, stream))


class FakeEntryPoint:
    def __init__(self, name, log, status=0):
        self.name, self.log, self.status = name, log, status

    def __call__(self, *args):
        self.log.append(("call", self.name, args))
        return self.status


def recorded_step(log, status=0, failing=None):
    """A recorder holding: launch a (main), hand-over main -> side, launch b (side), bucket 3, an eager op, launch c (main).
    The eager op makes a launch of its own, which is NOT part of the list."""
    main, side = FakeStream("main", log), FakeStream("side", log)
    fns = {n: FakeEntryPoint("sl_" + n, log, status if n == failing else 0) for n in "abcx"}
    args = {n: (object(), 7, n) for n in "abcx"}
    rec = ll.Recorder(lambda: "the library's text")
    event = FakeEvent(log)

    def per_batch(which):
        fns["x"](*args["x"])  # (Engine._eager_op runs this with recording switched off)
        log.append(("eager", which))

    rec.launch(fns["a"], args["a"], "sl_a", "fwd:a", main)
    rec.hand_over(event, main, side)
    rec.launch(fns["b"], args["b"], "sl_b", "bgrad:b", side)
    rec.bucket_ready(3)
    rec.eager(per_batch, ("tail",))
    rec.launch(fns["c"], args["c"], "sl_c", "fwd:c", main)
    return rec, dict(main=main, side=side, event=event, args=args)


def test_replay_repeats_the_recorded_calls_with_the_same_objects_in_order():
    log, buckets = [], []
    rec, w = recorded_step(log)
    assert len(rec) == 6  # the launch made inside the eager op is not in the list
    assert ll.entry_points(rec) == [("sl_a", "fwd:a"), ("sl_b", "bgrad:b"), ("sl_c", "fwd:c")]
    ll.replay(rec, buckets.append)
    assert buckets == [3]
    assert [e[:2] for e in log] == [("call", "sl_a"), ("record", w["event"]), ("wait", w["side"]), ("call", "sl_b"),
                                    ("call", "sl_x"), ("eager", "tail"), ("call", "sl_c")]
    calls = {e[1]: e[2] for e in log if e[0] == "call"}
    for n in "abcx":
        assert len(calls["sl_" + n]) == 3 and all(x is y for x, y in zip(calls["sl_" + n], w["args"][n]))
    assert log[1][2] is w["main"] and log[2][2] is w["event"]  # recorded on src, waited for by dst
    log.clear()
    ll.replay(rec, buckets.append)  # ... and again: the eager op is called at every replay
    assert buckets == [3, 3] and ("eager", "tail") in log and len(log) == 7


def arounds(log, out):
    return {"plain": None,
            "timed": ll.timed(out, lambda: FakeEvent(log)),
            "profiled": ll.profiled({"fwd:c"}, out, lambda: FakeEvent(log), lambda start, stop: log.append(("attach", start, stop)))}


@pytest.mark.parametrize("mode", ["plain", "timed", "profiled"])
def test_a_failing_launch_raises_with_the_entry_point_name(mode):
    log = []
    rec, _ = recorded_step(log, status=5, failing="b")
    with pytest.raises(ll.HipLibraryError, match=r"sl_b failed with status 5: the library's text"):
        ll.replay(rec, lambda b: None, arounds(log, [])[mode])
    assert ("call", "sl_c") not in [e[:2] for e in log]  # nothing is launched behind the failure
    from speechless_amd import _lib
    assert _lib.HipLibraryError is ll.HipLibraryError


def test_timeline_mode_brackets_every_launch_on_its_recorded_stream():
    log, out, buckets = [], [], []
    rec, w = recorded_step(log)
    ll.replay(rec, buckets.append, arounds(log, out)["timed"])
    assert [tag for tag, _, _ in out] == ["fwd:a", "bgrad:b", "fwd:c"] and buckets == [3]
    for (tag, start, stop), stream in zip(out, (w["main"], w["side"], w["main"])):
        i, j = log.index(("record", start, stream)), log.index(("record", stop, stream))
        assert j == i + 2 and log[i + 1][0] == "call"  # start, the launch, stop -- on the launch's own stream
    assert sum(1 for e in log if e[0] == "record") == 2 * 3 + 1  # (+ the hand-over's event)
    assert ("eager", "tail") in log


def test_profiled_mode_instruments_exactly_the_tagged_launches():
    log, out, buckets = [], [], []
    rec, w = recorded_step(log)
    ll.replay(rec, buckets.append, arounds(log, out)["profiled"])
    assert [tag for tag, _, _ in out] == ["fwd:c"] and buckets == [3]
    (_, start, stop), = out
    kinds = [e[:2] if e[0] == "call" else e[0] for e in log]
    assert kinds == [("call", "sl_a"), "record", "wait", ("call", "sl_b"), ("call", "sl_x"), "eager",
                     "record", "record", "attach", ("call", "sl_c")]
    assert log[-2] == ("attach", start, stop) and log[-4] == ("record", start, None) and log[-3] == ("record", stop, None)


def test_the_same_instrumentation_serves_a_single_eager_launch():
    log, out = [], []
    fn = FakeEntryPoint("sl_a", log)
    assert ll.timed(out, lambda: FakeEvent(log))(fn, (1, 2), "fwd:a", None) == 0
    assert [e[0] for e in log] == ["record", "call", "record"] and out[0][0] == "fwd:a" and log[0][2] is None


def test_buffers_grow_drops_the_lists_exactly_when_it_allocates():
    from speechless_amd.buffers import _Buffers

    class StandIn:
        device = "cpu"
        grow, invalidate = _Buffers.grow, _Buffers.invalidate

    buf = StandIn()
    buf.launch_lists = {"k": [1]}
    assert buf.grow("ws", 100, 16) is True and buf.ws.numel() == 100 and buf.launch_lists == {}
    ws = buf.ws
    buf.launch_lists = {"k": [1]}
    assert buf.grow("ws", 100) is False and buf.grow("ws", 40) is False
    assert buf.ws is ws and buf.launch_lists == {"k": [1]}  # large enough: neither
    assert buf.grow("ws", 101) is True and buf.ws.numel() == 101 and buf.launch_lists == {}
    buf.small = None
    assert buf.grow("small", 0, 16) is True and buf.small.numel() == 16  # the floor
    # first_drops=False: a workspace that did not exist is in no list; one that did is
    buf.launch_lists = {"k": [1]}
    assert buf.grow("late", 8, 16, first_drops=False) is True and buf.launch_lists == {"k": [1]}
    assert buf.grow("late", 32, 16, first_drops=False) is True and buf.late.numel() == 32 and buf.launch_lists == {}
    buf.launch_lists, buf.multi_tables, buf.wgrad_multi_ws = {"k": [1]}, {"t": 1}, ws
    buf.invalidate()
    assert buf.launch_lists == {} and buf.multi_tables == {} and buf.wgrad_multi_ws is None
