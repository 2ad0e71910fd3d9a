"""Gradient clipping and learning-rate decay of the optimizer, without a GPU: the float64 restatement of what Keras 2.0.x does
with `clipnorm`, `clipvalue` and `decay` (the GPU tests in test_gpu_optimizer_clip.py hold the engine to it), checked against
values worked out by hand, and the public `Adam` object / attribute pick-up of speechless_amd.net.

Restated from knowledge of Keras 2.0.x (optimizers.py: Optimizer.get_gradients, clip_norm, Adam.get_updates), like the Adam
row of oracle/w2l_oracle.py; it cannot be checked against Keras offline."""
import numpy as np
import pytest

from oracle import w2l_oracle as o


def keras_clipped_gradients(grads, clipnorm=0.0, clipvalue=0.0):
    """grads: list of arrays (the trainable tensors).  Returns (clipped list, global norm n).
    clipnorm > 0:  n = sqrt(sum over ALL tensors of sum(g * g));  g = g * clipnorm / n  if n >= clipnorm  else g
    clipvalue > 0: g = clip(g, -clipvalue, +clipvalue), after the norm clip.
    A NaN norm compares false: g passes through."""
    grads = [np.asarray(g, dtype=np.float64) for g in grads]
    n = float(np.sqrt(sum(float(np.sum(g * g)) for g in grads)))
    if clipnorm > 0 and n >= clipnorm:
        grads = [g * clipnorm / n for g in grads]
    if clipvalue > 0:
        grads = [np.clip(g, -clipvalue, clipvalue) for g in grads]
    return grads, n


def keras_decayed_lr(lr, decay, iterations):
    """iterations = updates completed BEFORE this one"""
    return lr * (1.0 / (1.0 + decay * iterations)) if decay > 0 else lr


def keras_adam_step_clipped(params, grads, ms, vs, iterations, lr=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0.0,
                            clipnorm=0.0, clipvalue=0.0):
    """One Keras 2.0 Adam update of a list of tensors with clipping and decay; iterations = updates completed before this one.
    Returns (params, ms, vs, n) -- n the unclipped global norm."""
    clipped, n = keras_clipped_gradients(grads, clipnorm, clipvalue)
    lr_now = keras_decayed_lr(lr, decay, iterations)
    out = [o.keras_adam_step(p, g, m, v, iterations + 1, lr_now, beta_1, beta_2, epsilon)
           for p, g, m, v in zip(params, clipped, ms, vs)]
    return [t[0] for t in out], [t[1] for t in out], [t[2] for t in out], n


G = [np.array([3.0, -4.0]), np.array([12.0])]  # n = sqrt(9 + 16 + 144) = 13


def test_norm_clip_above_below_and_at_the_boundary():
    got, n = keras_clipped_gradients(G, clipnorm=6.5)  # n > clipnorm: every element halved
    assert n == 13.0
    np.testing.assert_allclose(np.concatenate(got), [1.5, -2.0, 6.0], rtol=1e-15)
    got, n = keras_clipped_gradients(G, clipnorm=26.0)  # n < clipnorm: untouched, bit for bit
    assert n == 13.0 and all(np.array_equal(a, b) for a, b in zip(got, G))
    got, _ = keras_clipped_gradients(G, clipnorm=13.0)  # n == clipnorm: the branch is taken and multiplies by 13 / 13
    np.testing.assert_allclose(np.concatenate(got), [3.0, -4.0, 12.0], rtol=1e-15)
    got, n = keras_clipped_gradients(G)  # off
    assert n == 13.0 and all(np.array_equal(a, b) for a, b in zip(got, G))


def test_value_clip_comes_after_the_norm_clip():
    # norm clip first: (1.5, -2, 6); then the clamp at 1.75 -> (1.5, -1.75, 1.75).  The other order would give
    # clip(G, 1.75) = (1.75, -1.75, 1.75), norm 3.03 < 6.5: unchanged -> 1.75 in the first element.
    got, _ = keras_clipped_gradients(G, clipnorm=6.5, clipvalue=1.75)
    np.testing.assert_allclose(np.concatenate(got), [1.5, -1.75, 1.75], rtol=1e-15)
    got, _ = keras_clipped_gradients(G, clipvalue=3.5)  # the clamp alone
    np.testing.assert_allclose(np.concatenate(got), [3.0, -3.5, 3.5], rtol=1e-15)


def test_a_nan_norm_lets_the_gradient_pass():
    got, n = keras_clipped_gradients([np.array([np.nan, 1.0, 2.0])], clipnorm=0.5)
    assert np.isnan(n) and got[0][1] == 1.0 and got[0][2] == 2.0 and np.isnan(got[0][0])


def test_decay_at_iterations_0_1_2():
    assert keras_decayed_lr(1e-2, 0.5, 0) == 1e-2
    assert keras_decayed_lr(1e-2, 0.5, 1) == pytest.approx(1e-2 / 1.5, rel=1e-15)
    assert keras_decayed_lr(1e-2, 0.5, 2) == pytest.approx(5e-3, rel=1e-15)
    assert keras_decayed_lr(1e-2, 0.0, 7) == 1e-2


def test_clipped_adam_steps_by_hand():
    """three elements, first update from zero moments: m = 0.1 g', v = 0.001 g'^2, lr_t = lr * sqrt(0.001) / 0.1, so
    p moves by lr * g' / (|g'| + eps * sqrt(0.001)... ) ~ lr * sign(g') -- worked out per element below; the second update
    (iterations = 1) uses lr / 1.5."""
    p0 = [np.array([1.0, 2.0]), np.array([3.0])]
    zeros = [np.zeros(2), np.zeros(1)]
    lr, eps = 1e-2, 1e-8
    p1, m1, v1, n = keras_adam_step_clipped(p0, G, zeros, zeros, 0, lr=lr, decay=0.5, clipnorm=6.5, clipvalue=1.75)
    gc = np.array([1.5, -1.75, 1.75])
    assert n == 13.0
    np.testing.assert_allclose(np.concatenate(m1), 0.1 * gc, rtol=1e-12)
    np.testing.assert_allclose(np.concatenate(v1), 0.001 * gc * gc, rtol=1e-12)
    lr_t = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
    want = np.array([1.0, 2.0, 3.0]) - lr_t * (0.1 * gc) / (np.sqrt(0.001) * np.abs(gc) + eps)
    np.testing.assert_allclose(np.concatenate(p1), want, rtol=1e-12)
    np.testing.assert_allclose(np.concatenate(p1), [0.99, 2.01, 2.99], rtol=1e-7)  # |step| = lr on the first update
    # second update, same gradient: m = 0.19 g', v = 0.001999 g'^2, t = 2, lr = 1e-2 / 1.5
    p2, m2, v2, _ = keras_adam_step_clipped(p1, G, m1, v1, 1, lr=lr, decay=0.5, clipnorm=6.5, clipvalue=1.75)
    np.testing.assert_allclose(np.concatenate(m2), 0.19 * gc, rtol=1e-12)
    np.testing.assert_allclose(np.concatenate(v2), 0.001999 * gc * gc, rtol=1e-12)
    lr_t2 = (lr / 1.5) * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)
    want2 = np.concatenate(p1) - lr_t2 * (0.19 * gc) / (np.sqrt(0.001999) * np.abs(gc) + eps)
    np.testing.assert_allclose(np.concatenate(p2), want2, rtol=1e-12)
    # with everything off it is the plain Adam row
    q1, _, _, _ = keras_adam_step_clipped(p0, G, zeros, zeros, 0, lr=lr)
    r1 = o.keras_adam_step(p0[0], G[0], zeros[0], zeros[0], 1, lr)[0]
    assert np.array_equal(q1[0], r1)


def test_adam_defaults_and_attribute_pick_up():
    from speechless_amd.net import Adam, optimizer_settings
    a = Adam()
    assert (a.lr, a.beta_1, a.beta_2, a.epsilon, a.decay, a.clipnorm, a.clipvalue) == (1e-4, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0)
    a = Adam(1e-3, clipnorm=5.0, decay=0.25)
    assert optimizer_settings(a) == dict(lr=1e-3, beta_1=0.9, beta_2=0.999, adam_epsilon=1e-8, decay=0.25, clipnorm=5.0,
                                         clipvalue=0.0)

    class KerasLike:  # a Keras optimizer has clipnorm / clipvalue only when they were passed
        lr, beta_1, beta_2, epsilon = 2e-4, 0.8, 0.99, 1e-7
        clipvalue = np.float32(0.5)

    got = optimizer_settings(KerasLike())
    assert got == dict(lr=2e-4, beta_1=0.8, beta_2=0.99, adam_epsilon=1e-7, decay=0.0, clipnorm=0.0, clipvalue=0.5)
    assert all(type(got[k]) is float for k in ("decay", "clipnorm", "clipvalue"))

    class FourOnly:
        lr, beta_1, beta_2, epsilon = 1e-4, 0.9, 0.999, 1e-8
        clipnorm = None  # (an attribute that is there but unset)

    got = optimizer_settings(FourOnly())
    assert (got["decay"], got["clipnorm"], got["clipvalue"]) == (0.0, 0.0, 0.0)


def test_the_library_validates_the_new_entry_points_without_a_gpu(hip_lib):
    """argument checks run before any launch"""
    from speechless_amd import _lib
    ranges = (_lib.NormRange * 2)()
    ranges[0].offset, ranges[0].count = 3, 16384 - 3 + 1  # spans two chunks from its aligned start
    ranges[1].offset, ranges[1].count = 40001, 5
    assert hip_lib.raw("sl_grad_sqnorm_workspace_bytes")(ranges, 2) == 3 * 8
    assert hip_lib.raw("sl_grad_sqnorm_workspace_bytes")(ranges, 17) == 0
    assert hip_lib.raw("sl_grad_sqnorm")(None, ranges, 2, 0.0, None, None, None, None, 0, None) == -1
    assert "null pointer" in hip_lib.last_error()
    assert hip_lib.raw("sl_adam_step_clipped")(16, 16, 16, 16, 4, 1, 1e-4, 0.9, 0.999, 1e-8, None, -1.0, None) == -1
    assert "clipvalue" in hip_lib.last_error()
    assert hip_lib.raw("sl_clip_scale")(None, 1, 1.0, None, None, None) == -1
