"""The generators, the integer reference and the comparator of tests/exact_ints.py on the CPU: every case it builds for GPU
tests of the kernels respects its bit budget ON THE REFERENCE (conditions, not measurements), the family-A stack does not
degenerate, and the comparator finds a single planted difference."""
import numpy as np
import pytest

import exact_ints as xi
from oracle import w2l_oracle as o

CHAIN_LENGTHS = (47, 48, 49, 63, 64, 65, 77, 95, 96, 97, 128, 129, 300)


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("taps,stride,t", [(7, 1, 21), (32, 1, 40), (1, 1, 9), (48, 2, 31), (48, 2, 30), (5, 1, 3)])
def test_integer_reference_against_the_float64_oracle(taps, stride, t):
    """the int64 reference restates the oracle's float64 convolution and its gradients (independent code, same numbers)"""
    rng = np.random.RandomState(taps + t)
    x = rng.randint(-3, 4, size=(2, t, 6))
    w = rng.randint(-3, 4, size=(taps, 6, 5))
    bias = rng.randint(-2, 3, size=5)
    z = xi.reference_preactivation(x, w, bias, stride)
    assert z.dtype == np.int64
    assert np.array_equal(z, o.conv1d_preactivation(x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), stride))
    assert np.array_equal(xi.reference_forward(x, w, bias, stride), np.maximum(z, 0))
    g = rng.randint(-3, 4, size=z.shape)
    dx, dw, db = o.conv1d_backward(x.astype(np.float64), w.astype(np.float64), stride, g.astype(np.float64))
    assert np.array_equal(xi.reference_weight_gradient(x, g, taps, stride), dw)
    assert np.array_equal(xi.reference_bias_gradient(g), db)
    if stride == 1:
        assert np.array_equal(xi.reference_input_gradient(g, w), dx)
        mask = rng.randint(0, 2, size=x.shape)
        assert np.array_equal(xi.reference_input_gradient(g, w, mask), dx * (mask > 0))


def test_integer_reference_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError):
        xi.reference_preactivation(np.full((1, 3, 2), 0.5), np.ones((1, 2, 2)), np.zeros(2))
    with pytest.raises(OverflowError):
        xi.reference_preactivation(np.full((1, 3, 2), 2 ** 40), np.full((1, 2, 2), 2 ** 20), np.zeros(2))


# ------------------------------------------------------------------------------------------ the comparator
def test_comparator_reports_a_single_planted_difference_at_its_coordinate():
    want = np.arange(2 * 130 * 256, dtype=np.int64).reshape(2, 130, 256) % 200
    got = want.astype(np.float32)
    xi.assert_exact(got, want, "clean")
    assert xi.mismatch_report(got, want, "clean") is None
    for delta in (1, -1):
        got = want.astype(np.float32)
        got[1, 113, 201] += delta
        with pytest.raises(xi.NotExact) as err:
            xi.assert_exact(got, want, "planted")
        text = str(err.value)
        assert "planted: 1 of {} elements differ".format(want.size) in text
        assert "(1, 113, 201, {}, {})".format(float(want[1, 113, 201] + delta), int(want[1, 113, 201])) in text
        assert "by t mod 16: 1: 1" in text and "by t mod 48: 17: 1" in text and "by t mod 64: 49: 1" in text
        assert "by c // 64: 3: 1" in text
    # more than ten: all counted, ten listed; other ranks: index tuples and the channel-block histogram only
    got = want.astype(np.float32)
    got[0, 64:80, 0] += 1
    text = xi.mismatch_report(got, want, "many")
    assert "16 of" in text and text.count("\n    (") == 10 and "by t mod 64: " + ", ".join("{}: 1".format(i) for i in range(16)) in text
    text = xi.mismatch_report(np.array([1.0, 2.0, float("nan")]), np.array([1.0, 3.0, 4.0]), "vector")
    assert "2 of 3" in text and "t mod" not in text and "(1, 2.0, 3.0)" in text
    assert "shape" in xi.mismatch_report(np.zeros((2, 3)), np.zeros((3, 2)), "shape")


# ------------------------------------------------------------------------------------------ family A
def test_family_a_weights_have_exactly_p_plus_and_n_minus_per_column():
    rng = np.random.RandomState(1)
    w = xi.family_a_weights(rng, 7, 250, 250, p=2, n=2)
    assert w.shape == (7, 250, 250) and set(np.unique(w)) == {-1, 0, 1}
    assert ((w == 1).sum(axis=(0, 1)) == 2).all() and ((w == -1).sum(axis=(0, 1)) == 2).all()
    wt = xi.family_a_weights(rng, 7, 250, 300, p=3, n=1, by_input=True)
    assert wt.shape == (7, 250, 300)
    assert ((wt == 1).sum(axis=(0, 2)) == 3).all() and ((wt == -1).sum(axis=(0, 2)) == 1).all()
    x = xi.family_a_input(rng, (3, 300, 250))
    assert set(np.unique(x)) == {0, 1} and 0.49 < x.mean() < 0.51
    assert set(np.unique(xi.family_a_bias(rng, 250))) == {0, 1}


@pytest.fixture(scope="module")
def stack_a():
    x, weights = xi.family_a_stack(seed=7, batch=3, t=300)
    return x, weights, xi.run_stack(x, weights)


def test_family_a_stack_respects_the_bit_budget_and_does_not_degenerate(stack_a):
    """the seven-layer recipe (250 channels, 7 taps, P = N = 2, bias in {0, 1}, density 0.5, fixed seed): max_out <= P * max_in
    + 1 layer by layer, everything bf16 stores at most 255, and at EVERY layer 25-75 % non-zero outputs and >= 10 % negative
    pre-activations; at least 16 distinct values at the top"""
    x, weights, layers = stack_a
    max_in = int(x.max())
    for i, ((w, b), (z, y)) in enumerate(zip(weights, layers)):
        assert int(y.max()) <= 2 * max_in + 1, i                      # the bound by construction
        assert int(y.max()) <= xi.BF16_MAX_EXACT and xi.is_bf16_exact(y), i
        # sum |w| max |x| + |b|: four unit weights per column, so one bound per layer without another convolution
        assert int(np.abs(w).sum(axis=(0, 1)).max()) * max_in + int(b.max()) < xi.FP32_BUDGET, i
        assert 0.25 <= (y != 0).mean() <= 0.75, (i, (y != 0).mean())
        assert (z < 0).mean() >= 0.10, (i, (z < 0).mean())
        max_in = int(y.max())
    assert len(np.unique(layers[-1][1])) >= 16


@pytest.mark.parametrize("t_out", CHAIN_LENGTHS)
def test_family_a_backward_run_respects_the_bit_budget(t_out):
    """the input-gradient direction of the run at every length around the 48- and 64-row tile edges: gradient at the top in {-1, 0, 1}, weights
    with P = N = 2 per INPUT channel (the output columns of that launch), masks = the forward activations"""
    x, weights = xi.family_a_stack(seed=t_out, batch=3, t=t_out)
    layers = xi.run_stack(x, weights)
    assert max(int(y.max()) for _, y in layers) <= xi.BF16_MAX_EXACT
    g_top, wts, masks = xi.family_a_backward_run(t_out, x, layers)
    gs = xi.run_stack_backward(g_top, wts, masks)
    g_in = g_top
    for i, g in enumerate(gs):
        assert np.abs(g).max() <= xi.BF16_MAX_EXACT and xi.is_bf16_exact(g), i
        assert np.abs(g).max() <= 4 * np.abs(g_in).max(), i
        assert (g != 0).mean() > 0.05, i
        g_in = g
    assert len(np.unique(gs[-1])) >= 16


# ------------------------------------------------------------------------------------------ family B
@pytest.mark.parametrize("t_out", CHAIN_LENGTHS)
def test_family_b_run_keeps_its_impulse_count_and_bit_budget(t_out):
    """impulses at both utterance ends and on both sides of every 48- and 64-row tile edge; at most floor(255 / 6) of them
    in any receptive field of the dense layer -- wherever it sits in the run, after the shifting layers in front of it moved
    them by up to three frames each -- and every stored value of every layer at most 255"""
    frames = xi.tile_edge_frames(t_out)
    assert 0 in frames and t_out - 1 in frames
    for tile in (48, 64):
        for edge in range(tile, t_out, tile):
            assert edge - 1 in frames and edge in frames
    for dense_at in (0, 6):
        x, weights = xi.family_b_stack(seed=t_out, batch=3, t_out=t_out, dense_at=dense_at)
        assert x[:, frames][:, :, [0, 249]].all() and not np.delete(x, frames, axis=1).any() and x.max() <= xi.FAMILY_B_MAX_X
        layers = xi.run_stack(x, weights)
        dense_in = x if dense_at == 0 else layers[dense_at - 1][1]
        assert xi.max_impulses_in_field(dense_in, 7) <= xi.FAMILY_B_MAX_IMPULSES
        w = weights[dense_at][0]
        assert np.abs(w).max() == 3 and (w != 0).mean() > 0.8  # dense: every (tap, cin) position carries weight
        for i, (z, y) in enumerate(layers):
            assert y.max() <= xi.BF16_MAX_EXACT and xi.is_bf16_exact(y), (dense_at, i)
        assert (layers[-1][1] != 0).sum() > 100  # the impulses reach the top of the run
        g_top, wts, masks = xi.family_b_backward_run(t_out, 3, t_out, dense_at)
        gs = xi.run_stack_backward(g_top, wts, masks)
        assert all(np.abs(g).max() <= xi.BF16_MAX_EXACT and xi.is_bf16_exact(g) for g in gs) and (gs[-1] != 0).sum() > 100


@pytest.mark.parametrize("taps,t_out,batch", [(7, 300, 3), (32, 140, 2), (5, 129, 5)])
@pytest.mark.parametrize("family", ["A", "B"])
def test_single_launch_cases_respect_the_bit_budget(family, taps, t_out, batch):
    case = xi.nt_case(family, taps, t_out, batch, seed=taps)
    assert (case["x"][:, :, -1] == 1).all() and not case["w"][:, -1].any() and not case["w"][:, :, xi.NT_REAL:].any()
    assert xi.reference_accumulator_bound(case["x"], case["w"], case["bias"]) < xi.FP32_BUDGET
    if family == "B":
        assert xi.max_impulses_in_field(case["x"][:, :, :-1], taps) <= xi.FAMILY_B_MAX_IMPULSES
        assert case["x"][:, 0, [0, 249, 254]].all() and case["x"][:, t_out - 1, [0, 249, 254]].all()
        assert case["x"][:, 63, 254].all() and case["x"][:, 64, 254].all()
    want = xi.nt_expected(case)
    for name, y in want.items():
        assert np.abs(y).max() <= xi.BF16_MAX_EXACT and xi.is_bf16_exact(y), name
        assert not y[:, :, xi.NT_REAL:-1].any() and (y[:, :, -1] == (1 if name == "bias_relu" else 0)).all()
    assert (want["none"] < 0).mean() > 0.02 and (want["bias_relu"] > 0)[:, :, :xi.NT_REAL].mean() > 0.05


# ------------------------------------------------------------------------------------------ the whole stack (engine level)
def test_engine_case_respects_the_bit_budget_through_the_depth():
    """P = N = 2 in all eleven layers keeps every stored activation of layers 0-9 at most 255 (stride-2 first layer, 48 taps;
    2000-channel layers) and non-degenerate"""
    x, weights, strides = xi.engine_case()
    layers = xi.run_stack(x, weights, strides)
    x_in = x
    for i, ((w, b), (z, y)) in enumerate(zip(weights, layers)):
        assert xi.reference_accumulator_bound(x_in, w, b, strides[i]) < xi.FP32_BUDGET
        if i < 10:
            assert y.max() <= xi.BF16_MAX_EXACT and xi.is_bf16_exact(y), (i, y.max())
            assert 0.25 <= (y != 0).mean() <= 0.75, (i, (y != 0).mean())
        x_in = y
    assert layers[0][1].shape == (2, 77, 250) and layers[9][1].shape == (2, 77, 2000)


# ------------------------------------------------------------------------------------------ planes
@pytest.mark.parametrize("name", ["bf16x3", "f16x3"])
def test_plane_operands_split_exactly_and_only_where_they_should(name):
    fmt = xi.PLANE_FORMATS[name]
    rng = np.random.RandomState(3)
    wide = xi.wide_ints(rng, (4000,), fmt.wide_bits, signed=True)
    narrow = rng.randint(-2, 3, size=4000)
    for unit, scale in ((fmt.act_unit, 1.0), (fmt.w_unit, fmt.w_scale)):
        assert fmt.planes_exact(wide * unit * scale) and not fmt.lo_is_zero(wide * unit * scale)
        assert np.abs(wide * unit * scale).max() < 6e4
    assert fmt.planes_exact(narrow) and fmt.lo_is_zero(narrow) and fmt.lo_is_zero(narrow * fmt.w_scale)
    g_wide = xi.wide_ints(rng, (4000,), fmt.g_wide_bits, signed=True)
    assert fmt.planes_exact(g_wide * fmt.g_unit * fmt.g_scale) and not fmt.lo_is_zero(g_wide * fmt.g_unit * fmt.g_scale)
    # a family-A sum of wide values (two plus, two minus, a bias of one activation unit) still fits the planes
    sums = wide[:1000] + wide[1000:2000] - wide[2000:3000] - wide[3000:] + 1
    assert fmt.planes_exact(sums * fmt.act_unit) and np.abs(sums * fmt.act_unit).max() < 6e4
    g_sums = g_wide[:1000] + g_wide[1000:2000] - g_wide[2000:3000] - g_wide[3000:]
    assert fmt.planes_exact(g_sums * fmt.g_unit * fmt.g_scale) and np.abs(g_sums * fmt.g_unit * fmt.g_scale).max() < 65504
    # one bit more than the budget does not split exactly: the check can fail
    assert not fmt.planes_exact(int("10" * (fmt.bits // 2 + 1) + "1", 2) * fmt.act_unit)  # (bits + 3 bits, alternating)
    if name == "f16x3":  # the denormal case: 2^6 * w = n * 2^-24 with n around 2^20: hi normal, lo below 2^-14
        w, n = xi.denormal_weights(rng, 7, 250, 250)
        w = w[w != 0]
        assert np.abs(n).max() < 2 ** 21 and 4 * 2 * np.abs(n).max() < xi.FP32_BUDGET  # four weights per column, x <= 2
        hi, lo = fmt.split(w * fmt.w_scale)
        assert fmt.planes_exact(w * fmt.w_scale) and float(lo.float().abs().max()) < 2.0 ** -14 and bool(lo.float().all())
        assert abs(np.log2(np.abs(w)).mean() + 10) < 0.01


def test_sparse_columns_bound_a_wide_weight_gradient():
    rng = np.random.RandomState(5)
    g = xi.sparse_columns(rng, 3, 75, 256, 8, [-1, 1])
    assert ((g != 0).sum(axis=(0, 1)) == 8).all()
    x = xi.wide_ints(rng, (3, 75, 64), 19)
    assert xi.reference_weight_gradient(np.abs(x), np.abs(g), 7).max() < xi.FP32_BUDGET
