"""The engine's launch sequence, argument for argument, on every path it has: dtype (bf16, f32, bf16x3, f16x3), activation,
dropout, frozen layers, bucket callbacks and the CU hint, split top, the unfused / ungrouped schedules, the raw-wave front layer.

tests/golden/engine_launches/ was captured with capture() (and stored with encode()) on the commit BEFORE the engine's launch sites
moved into shared helpers; a refactor of the engine's Python launches what that commit launched.  Stricter than
tests/golden/default_step_launches.json: a device address is recorded as the tensor of the engine that holds it plus the byte
offset, geometries and job tables are expanded field by field, and the recorded lists keep their hand-overs, bucket markers and
eager ops in sequence.

Shapes: the spectrogram stack of the existing golden (test_gpu_parity.make_case(b=4, t=200, seed=3)); raw wave:
test_gpu_round4._wave_case cut to 4007 samples (26 frames of wave_conv, 13 of striding_conv).  Two training steps each."""
import ctypes
import gzip
import json
from pathlib import Path

import numpy as np
import pytest

from test_gpu_parity import make_case
from test_gpu_round4 import _wave_case

pytestmark = pytest.mark.gpu

GOLDEN_DIR = Path(__file__).resolve().parent / "golden" / "engine_launches"
_CASES = {}


def _case(kind, activation):
    key = (kind, activation)
    if key not in _CASES:
        if kind == "wave":
            _CASES[key] = _wave_case(b=3, t_audio=4007, activation=activation)
        else:
            _CASES[key] = make_case(b=4, t=200, seed=3, sizes=dict(activation=activation))
    return _CASES[key]


def _configurations():
    """name -> (input kind, dtype, activation, dropout rate, Engine keywords, attributes set on the engine, how a step runs:
    'resident' = train_step_resident, 'bucket' = forward / loss / backward(on_bucket_ready = no-op) / adam_step)"""
    out = {}

    def add(name, kind, dtype, activation="relu", rate=None, kw=None, attrs=None, how="resident", comm_cus=0):
        out[name] = dict(kind=kind, dtype=dtype, activation=activation, rate=rate, kw=kw or {}, attrs=attrs or {}, how=how,
                         comm_cus=comm_cus)

    add("bf16_default", "spec", "bf16")
    add("bf16_dropout", "spec", "bf16", rate=0.25)
    add("bf16_elu_dropout", "spec", "bf16", "elu", 0.25)
    add("bf16_frozen2", "spec", "bf16", kw=dict(frozen_layer_count=2))
    add("bf16_bucket", "spec", "bf16", how="bucket")
    add("bf16_bucket_cus32", "spec", "bf16", how="bucket", comm_cus=32)
    add("bf16_split_top", "spec", "bf16", attrs=dict(split_top=True, split_min_tiles=0))
    add("bf16_no_chain", "spec", "bf16", attrs=dict(use_chain=False))
    add("bf16_no_group_wgrad", "spec", "bf16", attrs=dict(group_wgrad=False))
    add("f32_default", "spec", "f32")
    add("f32_dropout", "spec", "f32", rate=0.25)
    for dtype in ("bf16x3", "f16x3"):
        add(dtype + "_relu", "spec", dtype)
        add(dtype + "_relu_dropout", "spec", dtype, rate=0.25)
        add(dtype + "_elu_dropout", "spec", dtype, "elu", 0.25)
        add(dtype + "_unfused_epilogue", "spec", dtype, attrs=dict(x3_fused_epilogue=False))
        add(dtype + "_bucket", "spec", dtype, how="bucket")
    for dtype in ("bf16", "bf16x3", "f16x3"):
        for activation in ("relu", "elu"):
            for rate in (None, 0.25):
                add("wave_{}_{}{}".format(dtype, activation, "_dropout" if rate else ""), "wave", dtype, activation, rate)
    return out


CONFIGURATIONS = _configurations()


# ------------------------------------------------------------------------------------------ what an argument is recorded as
def _tensor_table(eng):
    """(first byte, one past the last byte, attribute path) of every device tensor reachable from vars(eng) and vars(eng.cur),
    through lists, tuples and dicts; and {stream handle: attribute path} of the engine's own streams"""
    import torch
    table, streams = [], {}

    def walk(value, path, depth):
        if isinstance(value, torch.Tensor):
            if value.is_cuda and value.numel():
                extent = sum((n - 1) * s for n, s in zip(value.shape, value.stride())) + 1
                table.append((value.data_ptr(), value.data_ptr() + extent * value.element_size(), path))
        elif isinstance(value, torch.cuda.Stream):
            streams[value.cuda_stream] = path
        elif depth < 4 and isinstance(value, (list, tuple)):
            for n, item in enumerate(value):
                walk(item, "{}[{}]".format(path, n), depth + 1)
        elif depth < 4 and isinstance(value, dict):
            for key, item in value.items():
                walk(item, "{}[{!r}]".format(path, key), depth + 1)

    for prefix, owner in (("", eng), ("cur.", eng.cur)):
        for name, value in vars(owner).items():
            if name != "launch_lists":
                walk(value, prefix + name, 0)
    return table, streams


class _Normalizer:
    def __init__(self, eng):
        self.table, self.streams = _tensor_table(eng)
        self.unresolved = 0

    def address(self, value):
        if value in self.streams:
            return "stream:" + self.streams[value]
        # the smallest tensor that contains the address; among equals (aliases) the first path in sorted order
        hits = sorted((hi - lo, path, value - lo) for lo, hi, path in self.table if lo <= value < hi)
        if not hits:
            self.unresolved += 1
            return "address"
        return "{}+{}".format(hits[0][1], hits[0][2])

    def __call__(self, arg):
        import torch
        if arg is None or isinstance(arg, (bool, str)):
            return arg
        if isinstance(arg, int):
            return self.address(arg) if abs(arg) >= 1 << 32 else arg
        if isinstance(arg, float):
            return repr(arg)
        if isinstance(arg, torch.cuda.Stream):
            return "stream:" + self.streams.get(arg.cuda_stream, str(arg.cuda_stream) if arg.cuda_stream == 0 else "other")
        if isinstance(arg, ctypes.c_void_p):
            return self(arg.value)
        if isinstance(arg, ctypes.Structure):
            return {name: self(getattr(arg, name)) for name, _ in arg._fields_}
        if isinstance(arg, ctypes.Array):
            return [self(item) for item in arg]
        if hasattr(arg, "_obj"):  # ctypes.byref(structure)
            return self(arg._obj)
        return type(arg).__name__


def _normalized_ops(ops, norm):
    from speechless_amd import launch_list
    out = []
    for op in ops:
        if op.kind == launch_list.LAUNCH:
            out.append(["launch", op.name, op.tag, [norm(a) for a in op.args], norm(op.stream)])
        elif op.kind == launch_list.HAND_OVER:
            out.append(["hand_over", "", "", [norm(op.src), norm(op.dst)]])
        elif op.kind == launch_list.BUCKET_READY:
            out.append(["bucket_ready", "", "", [op.bucket]])
        else:
            out.append(["eager", op.fn.__name__, "", [norm(a) for a in op.args]])
    return out


def capture(engine_module, name):
    """Two training steps of configuration `name` on engine_module.Engine -> {"steps": per step, every C-ABI call that went
    through Engine._launch (recorded or not) as [entry point, tag, arguments]; "lists": the launch lists the buffer set holds
    afterwards, every op as [kind, entry point / function, tag, payload]; "unresolved": the addresses no tensor of the engine
    contains}"""
    import torch
    cfg = CONFIGURATIONS[name]
    case = _case(cfg["kind"], cfg["activation"])
    eng = engine_module.Engine(case["specs"], case["k"], dtype=cfg["dtype"], **cfg["kw"])
    eng.set_weights(case["weights"])
    eng.dropout_rate = cfg["rate"]
    for attr, value in cfg["attrs"].items():
        assert hasattr(eng, attr), attr
        setattr(eng, attr, value)
    seen = []
    launch = eng._launch
    eng._launch = lambda tag, entry, *args: (seen.append((entry, tag, args)), launch(tag, entry, *args))
    out = {"steps": [], "lists": {}}
    unresolved = 0
    for _ in range(2):
        eng.load_input(case["x"])
        eng.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]))
        if cfg["how"] == "bucket":
            eng.set_comm_cus(cfg["comm_cus"])
            eng.forward(training=True)
            eng.loss(grad_scale=1.0 / eng.cur.batch)
            eng.backward(on_bucket_ready=lambda b: None)
            eng.adam_step()
        else:
            eng.train_step_resident()
        torch.cuda.synchronize()
        norm = _Normalizer(eng)  # (after the step: what it allocated on the way is in the table)
        out["steps"].append([[entry, tag, [norm(a) for a in args]] for entry, tag, args in seen])
        unresolved += norm.unresolved
        del seen[:]
    norm = _Normalizer(eng)
    for key, ops in eng.cur.launch_lists.items():
        assert key[0] not in out["lists"], key
        out["lists"][key[0]] = _normalized_ops(ops, norm)
    out["unresolved"] = unresolved + norm.unresolved
    del eng
    torch.cuda.empty_cache()
    return json.loads(json.dumps(out))


# ------------------------------------------------------------------------------------------ how the goldens are stored
# Most launches recur: in the second step, in the recorded lists, in other configurations.  tables.json.gz (gzip of JSON text,
# 0.2 MB unpacked) holds every distinct launch [entry point, tag, arguments] once, a geometry inside it as {"geom": index into
# the distinct sl_conv_geom value rows}; <configuration>.json holds what capture() returned with every launch replaced by its
# index (in a list: [index, stream]).
GEOM_FIELDS = ["batch", "t_out", "taps", "cin", "cout", "x_row0", "x_row_stride", "x_batch_stride", "y_row0", "y_row_stride",
               "y_batch_stride", "acc_scale"]


def _intern(table, value):
    if value not in table:
        table.append(value)
    return table.index(value)


def encode(results):
    """{configuration: capture()} -> {file name: text or bytes} of the golden folder; decode() returns the captures unchanged"""
    geoms, launches, files = [], [], {}

    def pack(x):
        if isinstance(x, dict):
            if list(x) == GEOM_FIELDS:
                return {"geom": _intern(geoms, [x[f] for f in GEOM_FIELDS])}
            return {k: pack(v) for k, v in x.items()}
        return [pack(v) for v in x] if isinstance(x, list) else x

    def text(value):
        return json.dumps(value, separators=(",", ":"))

    for name in sorted(results):
        res = results[name]
        steps = [[_intern(launches, pack(e)) for e in step] for step in res["steps"]]
        lists = {key: [[_intern(launches, pack(op[1:4])), op[4]] if op[0] == "launch" else op for op in ops]
                 for key, ops in sorted(res["lists"].items())}
        files[name + ".json"] = "{{\n \"unresolved\": {},\n \"steps\": {},\n \"lists\": {}\n}}\n".format(
            res["unresolved"], text(steps), text(lists))
    rows = lambda table: ",\n".join("  " + text(v) for v in table)  # noqa: E731  (one row per line: a new launch is a new line)
    tables = "{{\n \"geom_fields\": {},\n \"geoms\": [\n{}\n ],\n \"launches\": [\n{}\n ]\n}}\n".format(
        text(GEOM_FIELDS), rows(geoms), rows(launches))
    files["tables.json.gz"] = gzip.compress(tables.encode("ascii"), mtime=0)
    return files


def decode(tables, golden):
    def unpack(x):
        if isinstance(x, dict):
            if list(x) == ["geom"]:
                return dict(zip(tables["geom_fields"], tables["geoms"][x["geom"]]))
            return {k: unpack(v) for k, v in x.items()}
        return [unpack(v) for v in x] if isinstance(x, list) else x

    launch = lambda i: unpack(tables["launches"][i])  # noqa: E731
    return {"unresolved": golden["unresolved"], "steps": [[launch(i) for i in step] for step in golden["steps"]],
            "lists": {key: [["launch"] + launch(op[0]) + [op[1]] if isinstance(op[0], int) else op for op in ops]
                      for key, ops in golden["lists"].items()}}


def _golden(name):
    if "tables" not in _CASES:
        _CASES["tables"] = json.loads(gzip.decompress((GOLDEN_DIR / "tables.json.gz").read_bytes()))
    return decode(_CASES["tables"], json.loads((GOLDEN_DIR / (name + ".json")).read_text()))


@pytest.mark.parametrize("name", sorted(CONFIGURATIONS))
def test_engine_launches_what_the_commit_before_the_launch_helpers_launched(name):
    from speechless_amd import engine
    want = _golden(name)
    got = capture(engine, name)
    assert sorted(got["lists"]) == sorted(want["lists"]) and len(got["steps"]) == len(want["steps"]) == 2
    parts = [("step {}".format(n), g, w, 2) for n, (g, w) in enumerate(zip(got["steps"], want["steps"]))]
    parts += [("list " + key, got["lists"][key], want["lists"][key], 3) for key in sorted(want["lists"])]
    for what, g, w, head in parts:  # names and tags first: a failure names the first differing launch
        assert [e[:head] for e in g] == [e[:head] for e in w], (name, what)
    for what, g, w, _ in parts:
        for n, (eg, ew) in enumerate(zip(g, w)):
            assert eg == ew, (name, what, n)
    assert got["unresolved"] == want["unresolved"], name
    assert len(got["steps"][0]) > 20  # (something was captured at all)
