"""The host side of sl_ctc_loss_grad for labels of 512 .. 2047 letters (no GPU): exported symbols, the workspace size, the refusals
that come before any launch, the engine's label-width check, and the margin of the loss bound the GPU tests use."""
import types

import numpy as np
import pytest

from oracle import w2l_oracle as o

SL_ERR_INVALID_ARGUMENT, SL_ERR_UNSUPPORTED, SL_ERR_WORKSPACE_TOO_SMALL = -1, -2, -3


def lattice_sp(l_max):
    return (2 * l_max + 1 + 63) // 64 * 64


def test_symbols_and_signatures_are_unchanged():
    from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p
    from speechless_amd import _lib
    assert _lib.SIGNATURES["sl_ctc_workspace_bytes"] == (c_size_t, [c_int, c_int, c_int])
    assert _lib.SIGNATURES["sl_ctc_loss_grad"] == (c_int, [c_void_p] * 7 + [c_int] * 6 + [c_int64, c_int, c_float, c_float,
                                                                                       c_void_p, c_size_t, c_void_p])
    assert _lib.SIGNATURES["sl_ctc_select"] == (c_int, [c_int])
    assert not any("ctc_long" in name for name in _lib.SIGNATURES)  # the long path is behind the same entry point


def test_label_limits_are_stated_in_one_place():
    from speechless_amd import longform
    assert longform.CTC_LOSS_MAX_LABEL == 2047 < longform.ALIGN_MAX_LABEL


def test_workspace_size(hip_lib):
    size = hip_lib.raw("sl_ctc_workspace_bytes")
    lens = (1, 255, 256, 511, 512, 1023, 1024, 2047)
    for batch, frames in ((1, 100), (3, 777), (32, 1280)):
        sizes = [size(batch, frames, l) for l in lens]
        assert sizes == sorted(sizes) and sizes[0] > 0, sizes
    for l_max in lens:
        assert size(2, 100, l_max) <= size(3, 100, l_max) <= size(3, 101, l_max)
    for l_max in (512, 600, 1023, 1024, 2047):
        for batch, frames in ((1, 1), (2, 700), (8, 4000)):
            assert size(batch, frames, l_max) >= 2 * batch * frames * lattice_sp(l_max) * 8
    assert size(2, 100, 2048) == 0 and size(2, 100, 8191) == 0
    assert size(0, 100, 600) == 0 and size(2, 0, 600) == 0 and size(-1, 100, 600) == 0 and size(2, 100, -1) == 0
    # 64-bit arithmetic: 32 x 4000 frames of 4096 doubles, twice, is 8.4e9 bytes
    assert 2 * 32 * 4000 * 4096 * 8 <= size(32, 4000, 2047) < 2 * 32 * 4000 * 4096 * 8 + (1 << 24)


def test_refusals_come_before_any_launch(hip_lib):
    """valid HOST addresses: nothing may be launched on them"""
    call = hip_lib.raw("sl_ctc_loss_grad")
    buf = np.zeros((64,), dtype=np.float32).ctypes.data
    ptrs = (buf,) * 7

    def run(ptrs, l_max, ws=buf, ws_bytes=1 << 40, batch=1, t_out=10, k=29):
        return call(*ptrs, batch, t_out, k, l_max, 0, k, t_out * k, 0, 1e-8, 1.0, ws, ws_bytes, None)

    assert run(ptrs, 2048) == SL_ERR_UNSUPPORTED
    assert "l_max" in hip_lib.last_error() and "2047" in hip_lib.last_error() and "2048" in hip_lib.last_error()
    assert run(ptrs, 8191) == SL_ERR_UNSUPPORTED
    assert run(ptrs, 0) == SL_ERR_INVALID_ARGUMENT
    for l_max in (100, 600, 2047):
        for i in range(7):
            args = list(ptrs)
            args[i] = None
            assert run(args, l_max) == SL_ERR_INVALID_ARGUMENT and "null pointer" in hip_lib.last_error(), (l_max, i)
        assert run(ptrs, l_max, ws=None) == SL_ERR_INVALID_ARGUMENT
        need = hip_lib.raw("sl_ctc_workspace_bytes")(1, 10, l_max)
        assert run(ptrs, l_max, ws_bytes=need - 1) == SL_ERR_WORKSPACE_TOO_SMALL
        assert "workspace too small" in hip_lib.last_error()
    assert run(ptrs, 600, k=65) == SL_ERR_INVALID_ARGUMENT and run(ptrs, 600, batch=0) == SL_ERR_INVALID_ARGUMENT


def test_engine_refuses_a_label_batch_wider_than_the_loss_takes():
    """Engine.set_labels / set_labels_resident both go through _check_label_width (an Engine itself needs a device)"""
    from speechless_amd.engine import Engine
    ctc = types.SimpleNamespace(criterion="ctc")
    Engine._check_label_width(ctc, 0)
    Engine._check_label_width(ctc, 512)
    Engine._check_label_width(ctc, 2047)
    with pytest.raises(ValueError, match="CTC_LOSS_MAX_LABEL = 2047"):
        Engine._check_label_width(ctc, 2048)
    Engine._check_label_width(types.SimpleNamespace(criterion="asg"), 2048)  # (sl_asg_loss_grad states its own limit)
    import inspect
    for method in (Engine.set_labels, Engine.set_labels_resident):
        assert "_check_label_width" in inspect.getsource(method)


def test_loss_bound_covers_fp32_logq():
    """The absolute term T * 1.2e-6 of the GPU tests' loss bound: the oracle on float64 logq and on logq rounded to fp32 (what
    the kernel reads), in the regime where the loss is near 0 and the relative term gives nothing."""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    from fuzz_ctc import regime_logits
    rng = np.random.RandomState(3)
    k, n = 29, 600
    label = list(rng.randint(0, k - 1, size=n))
    for regime, t in (("learnt", 900), ("learnt", 640), ("collapse", 700)):
        logits = regime_logits(rng, label, t, k, regime)
        probs = o.softmax(logits.astype(np.float32)).astype(np.float32).astype(np.float64)
        log_q = o.ctc_log_q(probs[None], 1e-8)[0]
        assert np.abs(log_q).max() <= 18.5
        exact, _ = o.ctc_single(log_q, label, k - 1)
        rounded, _ = o.ctc_single(log_q.astype(np.float32).astype(np.float64), label, k - 1)
        assert np.isfinite(exact)
        assert abs(rounded - exact) <= 0.5 * t * 1.2e-6, (regime, t, exact, rounded)
