"""The Keras 2.0.x optimizers beside Adam -- SGD, RMSprop, Adagrad, Adadelta, Adamax -- without a GPU: their float64 restatement
(the GPU tests in test_gpu_optimizers.py hold the kernels and the engine to it), checked against two-element examples worked
out by hand and against torch.optim where the two definitions coincide; the public optimizer classes and the attribute
pick-up of speechless_amd.net; the optimizer-state file of a one-slot and a two-slot rule.

Restated from knowledge of Keras 2.0.x (optimizers.py: the get_updates of each class), like the Adam row of
oracle/w2l_oracle.py; it cannot be checked against Keras offline."""
import numpy as np
import pytest

from test_optimizer_clip import keras_clipped_gradients, keras_decayed_lr

RULES = ("sgd", "rmsprop", "adagrad", "adadelta", "adamax")
SLOTS = {"sgd": 1, "rmsprop": 1, "adagrad": 1, "adadelta": 2, "adamax": 2}
KERAS_DEFAULTS = {
    "sgd": dict(lr=0.01, momentum=0.0, nesterov=False),
    "rmsprop": dict(lr=0.001, rho=0.9, epsilon=1e-8),
    "adagrad": dict(lr=0.01, epsilon=1e-8),
    "adadelta": dict(lr=1.0, rho=0.95, epsilon=1e-8),
    "adamax": dict(lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-8),
}


def keras_optimizer_step(rule, params, grads, slots, iterations, decay=0.0, clipnorm=0.0, clipvalue=0.0, **hyper):
    """One Keras 2.0 update of a list of tensors by `rule`, in float64.  slots: one list of tensors per state slot of the rule
    (SGD: [m]; RMSprop, Adagrad: [a]; Adadelta: [a, d]; Adamax: [m, u]), zeros at the start; iterations = updates completed
    before this one; hyper: the rule's Keras keyword arguments (KERAS_DEFAULTS for those left out).
    Returns (params, slots, n) -- n the unclipped global norm."""
    h = dict(KERAS_DEFAULTS[rule], **hyper)
    clipped, n = keras_clipped_gradients(grads, clipnorm, clipvalue)
    lr = keras_decayed_lr(h["lr"], decay, iterations)
    t = iterations + 1
    new_p, new_slots = [], [[] for _ in range(SLOTS[rule])]
    for i, (p, g) in enumerate(zip(params, clipped)):
        p = np.asarray(p, dtype=np.float64)
        s = [np.asarray(slot[i], dtype=np.float64) for slot in slots]
        if rule == "sgd":
            v = h["momentum"] * s[0] - lr * g
            p = p + h["momentum"] * v - lr * g if h["nesterov"] else p + v
            s = [v]
        elif rule == "rmsprop":
            a = h["rho"] * s[0] + (1.0 - h["rho"]) * g * g
            p = p - lr * g / (np.sqrt(a) + h["epsilon"])
            s = [a]
        elif rule == "adagrad":
            a = s[0] + g * g
            p = p - lr * g / (np.sqrt(a) + h["epsilon"])
            s = [a]
        elif rule == "adadelta":
            a = h["rho"] * s[0] + (1.0 - h["rho"]) * g * g
            u = g * np.sqrt(s[1] + h["epsilon"]) / np.sqrt(a + h["epsilon"])
            p = p - lr * u
            s = [a, h["rho"] * s[1] + (1.0 - h["rho"]) * u * u]
        elif rule == "adamax":
            m = h["beta_1"] * s[0] + (1.0 - h["beta_1"]) * g
            u = np.maximum(h["beta_2"] * s[1], np.abs(g))
            p = p - (lr / (1.0 - h["beta_1"] ** t)) * m / (u + h["epsilon"])
            s = [m, u]
        else:
            raise ValueError(rule)
        new_p.append(p)
        for k, value in enumerate(s):
            new_slots[k].append(value)
    return new_p, new_slots, n


def two_steps(rule, g1, g2, **hyper):
    """two updates of p = (1, 2) from zero state with decay 0.5: lr at it = 0, lr / 1.5 at it = 1"""
    p, slots = [np.array([1.0, 2.0])], [[np.zeros(2)] for _ in range(SLOTS[rule])]
    p1, slots1, _ = keras_optimizer_step(rule, p, [np.array(g1)], slots, 0, decay=0.5, **hyper)
    p2, slots2, _ = keras_optimizer_step(rule, p1, [np.array(g2)], slots1, 1, decay=0.5, **hyper)
    return p1[0], [s[0] for s in slots1], p2[0], [s[0] for s in slots2]


G = [0.5, -1.0]


# ------------------------------------------------------------------------------------------ the restatement by hand
def test_sgd_with_momentum_by_hand():
    p1, (m1,), p2, (m2,) = two_steps("sgd", G, G, lr=0.1, momentum=0.9)
    # it = 0: v = -0.1 g = (-0.05, 0.1)
    np.testing.assert_allclose(m1, [-0.05, 0.1], rtol=1e-14)
    np.testing.assert_allclose(p1, [0.95, 2.1], rtol=1e-14)
    # it = 1: lr = 0.1 / 1.5; v = 0.9 (-0.05, 0.1) - (0.5, -1) / 15 = (-0.045 - 1/30, 0.09 + 1/15)
    np.testing.assert_allclose(m2, [-0.045 - 1 / 30, 0.09 + 1 / 15], rtol=1e-14)
    np.testing.assert_allclose(p2, [0.95 - 0.045 - 1 / 30, 2.1 + 0.09 + 1 / 15], rtol=1e-14)
    np.testing.assert_allclose(p2, [0.871666666666667, 2.256666666666667], rtol=1e-14)


def test_sgd_nesterov_by_hand():
    p1, (m1,), p2, (m2,) = two_steps("sgd", G, G, lr=0.1, momentum=0.9, nesterov=True)
    # it = 0: v = (-0.05, 0.1); p = p + 0.9 v - 0.1 g = (1 - 0.045 - 0.05, 2 + 0.09 + 0.1)
    np.testing.assert_allclose(m1, [-0.05, 0.1], rtol=1e-14)
    np.testing.assert_allclose(p1, [0.905, 2.19], rtol=1e-14)
    # it = 1: v = (-0.0783333, 0.1566667) as without nesterov; p = p + 0.9 v - g / 15
    np.testing.assert_allclose(m2, [-0.045 - 1 / 30, 0.09 + 1 / 15], rtol=1e-14)
    np.testing.assert_allclose(p2, [0.905 - 0.9 * (0.045 + 1 / 30) - 1 / 30, 2.19 + 0.9 * (0.09 + 1 / 15) + 1 / 15], rtol=1e-14)
    np.testing.assert_allclose(p2, [0.801166666666667, 2.397666666666667], rtol=1e-14)
    # plain SGD: no momentum, the slot holds the last step
    q1, (v1,), _, _ = two_steps("sgd", G, G, lr=0.1)
    np.testing.assert_allclose(q1, [0.95, 2.1], rtol=1e-14)
    np.testing.assert_allclose(v1, [-0.05, 0.1], rtol=1e-14)


def test_rmsprop_by_hand():
    p1, (a1,), p2, (a2,) = two_steps("rmsprop", G, G, lr=0.1, rho=0.75, epsilon=0.25)
    # it = 0: a = 0.25 g^2 = (0.0625, 0.25), sqrt = (0.25, 0.5), + eps = (0.5, 0.75); step = 0.1 g / that = (0.1, -0.1333...)
    np.testing.assert_allclose(a1, [0.0625, 0.25], rtol=1e-14)
    np.testing.assert_allclose(p1, [0.9, 2.0 + 0.1 / 0.75], rtol=1e-14)
    # it = 1: a = 0.75 a + 0.25 g^2 = 0.4375 g^2 = (0.109375, 0.4375); lr = 0.1 / 1.5
    np.testing.assert_allclose(a2, [0.109375, 0.4375], rtol=1e-14)
    want = [0.9 - (0.1 / 1.5) * 0.5 / (np.sqrt(0.109375) + 0.25), 2.0 + 0.1 / 0.75 + (0.1 / 1.5) / (np.sqrt(0.4375) + 0.25)]
    np.testing.assert_allclose(p2, want, rtol=1e-14)
    np.testing.assert_allclose(p2, [0.842599826, 2.206477844], rtol=1e-6)  # (decimals carried by hand to seven digits)


def test_adagrad_by_hand():
    p1, (a1,), p2, (a2,) = two_steps("adagrad", G, G, lr=0.1, epsilon=0.25)
    # it = 0: a = g^2 = (0.25, 1), sqrt + eps = (0.75, 1.25); step = (0.05 / 0.75, -0.1 / 1.25)
    np.testing.assert_allclose(a1, [0.25, 1.0], rtol=1e-14)
    np.testing.assert_allclose(p1, [1.0 - 0.05 / 0.75, 2.08], rtol=1e-14)
    # it = 1: a = 2 g^2 = (0.5, 2); lr = 0.1 / 1.5
    np.testing.assert_allclose(a2, [0.5, 2.0], rtol=1e-14)
    want = [1.0 - 0.05 / 0.75 - (0.1 / 1.5) * 0.5 / (np.sqrt(0.5) + 0.25), 2.08 + (0.1 / 1.5) / (np.sqrt(2.0) + 0.25)]
    np.testing.assert_allclose(p2, want, rtol=1e-14)
    np.testing.assert_allclose(p2, [0.898506721, 2.120059234], rtol=1e-6)  # (decimals carried by hand to seven digits)


def test_adadelta_by_hand():
    p1, (a1, d1), p2, (a2, d2) = two_steps("adadelta", G, G, lr=1.0, rho=0.75, epsilon=0.25)
    # it = 0: a = 0.25 g^2 = (0.0625, 0.25); u = g sqrt(0 + 0.25) / sqrt(a + 0.25) = (0.25 / sqrt(0.3125), -0.5 / sqrt(0.5))
    u1 = np.array([0.25 / np.sqrt(0.3125), -0.5 / np.sqrt(0.5)])
    np.testing.assert_allclose(u1, [0.447213595, -0.707106781], rtol=1e-6)  # (decimals carried by hand to seven digits)
    np.testing.assert_allclose(a1, [0.0625, 0.25], rtol=1e-14)
    np.testing.assert_allclose(p1, [1.0 - u1[0], 2.0 - u1[1]], rtol=1e-14)
    # d = 0.25 u^2 = (0.25 * 0.2, 0.25 * 0.5) = (0.05, 0.125)
    np.testing.assert_allclose(d1, [0.05, 0.125], rtol=1e-14)
    # it = 1: a = (0.109375, 0.4375); u = g sqrt(d + 0.25) / sqrt(a + 0.25); lr = 1 / 1.5; d = 0.75 d + 0.25 u^2
    u2 = np.array([0.5 * np.sqrt(0.3) / np.sqrt(0.359375), -np.sqrt(0.375) / np.sqrt(0.6875)])
    np.testing.assert_allclose(a2, [0.109375, 0.4375], rtol=1e-14)
    np.testing.assert_allclose(p2, [1.0 - u1[0] - u2[0] / 1.5, 2.0 - u1[1] - u2[1] / 1.5], rtol=1e-14)
    np.testing.assert_allclose(d2, [0.0375 + 0.25 * 0.25 * 0.3 / 0.359375, 0.09375 + 0.25 * 0.375 / 0.6875], rtol=1e-14)
    # by hand: u2 = (0.5 * 0.547723 / 0.599479, -0.612372 / 0.829156) = (0.456832, -0.738549); / 1.5 = (0.304555, -0.492366)
    np.testing.assert_allclose(p2, [0.552786 - 0.304555, 2.707107 + 0.492366], rtol=5e-6)  # (six digits carried by hand)


def test_adamax_by_hand():
    p1, (m1, u1), p2, (m2, u2) = two_steps("adamax", G, [0.1, -3.0], lr=0.1, beta_1=0.5, beta_2=0.5, epsilon=0.25)
    # it = 0: m = 0.5 g = (0.25, -0.5); u = max(0, |g|) = (0.5, 1); lr_t = 0.1 / (1 - 0.5) = 0.2
    np.testing.assert_allclose(m1, [0.25, -0.5], rtol=1e-14)
    np.testing.assert_allclose(u1, [0.5, 1.0], rtol=1e-14)
    np.testing.assert_allclose(p1, [1.0 - 0.2 * 0.25 / 0.75, 2.0 + 0.2 * 0.5 / 1.25], rtol=1e-14)
    # it = 1, g = (0.1, -3): m = (0.125 + 0.05, -0.25 - 1.5); u = (max(0.25, 0.1), max(0.5, 3)): the decayed u wins once, |g| once
    np.testing.assert_allclose(m2, [0.175, -1.75], rtol=1e-14)
    np.testing.assert_allclose(u2, [0.25, 3.0], rtol=1e-14)
    lr_t = (0.1 / 1.5) / (1.0 - 0.25)
    np.testing.assert_allclose(p2, [1.0 - 0.2 / 3 - lr_t * 0.175 / 0.5, 2.08 + lr_t * 1.75 / 3.25], rtol=1e-14)
    np.testing.assert_allclose(p2, [0.902222222, 2.127863248], rtol=1e-6)  # (decimals carried by hand to seven digits)


def test_clipping_comes_first_and_defaults_are_keras():
    # clipnorm 6.5 halves (3, -4, 12) (n = 13), clipvalue 1.75 then clamps: (1.5, -1.75, 1.75); plain SGD moves by -lr g'
    p = [np.array([1.0, 2.0]), np.array([3.0])]
    g = [np.array([3.0, -4.0]), np.array([12.0])]
    got, (v,), n = keras_optimizer_step("sgd", p, g, [[np.zeros(2), np.zeros(1)]], 0, clipnorm=6.5, clipvalue=1.75)
    assert n == 13.0
    np.testing.assert_allclose(np.concatenate(got), [1.0 - 0.015, 2.0 + 0.0175, 3.0 - 0.0175], rtol=1e-14)  # lr = 0.01
    np.testing.assert_allclose(np.concatenate(v), [-0.015, 0.0175, -0.0175], rtol=1e-14)


# ------------------------------------------------------------------------------------------ against torch.optim
def torch_steps(make, p0, grads):
    import torch
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = make([p])
    out = []
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        out.append(p.detach().numpy().copy())
    return out


@pytest.mark.parametrize("name,rule,hyper,make", [
    ("momentum", "sgd", dict(lr=0.1, momentum=0.9), lambda torch, p: torch.optim.SGD(p, lr=0.1, momentum=0.9)),
    ("nesterov", "sgd", dict(lr=0.1, momentum=0.9, nesterov=True),
     lambda torch, p: torch.optim.SGD(p, lr=0.1, momentum=0.9, nesterov=True)),
    ("rmsprop", "rmsprop", dict(lr=0.01, rho=0.9, epsilon=1e-8),
     lambda torch, p: torch.optim.RMSprop(p, lr=0.01, alpha=0.9, eps=1e-8)),
    ("adagrad", "adagrad", dict(lr=0.1, epsilon=1e-8), lambda torch, p: torch.optim.Adagrad(p, lr=0.1, eps=1e-8)),
    ("adadelta", "adadelta", dict(lr=1.0, rho=0.95, epsilon=1e-8),
     lambda torch, p: torch.optim.Adadelta(p, lr=1.0, rho=0.95, eps=1e-8)),
    # torch puts eps inside the max (max(b2 u, |g| + eps)): the two definitions coincide for eps = 0 on gradients without zeros
    ("adamax", "adamax", dict(lr=0.01, beta_1=0.9, beta_2=0.999, epsilon=0.0),
     lambda torch, p: torch.optim.Adamax(p, lr=0.01, betas=(0.9, 0.999), eps=0.0)),
])
def test_three_steps_equal_torch_optim_where_the_definitions_coincide(name, rule, hyper, make):
    import torch
    rng = np.random.RandomState(7)
    p0 = rng.randn(64)
    grads = [rng.randn(64) * 10.0 ** rng.uniform(-3, 1, size=64) for _ in range(3)]
    assert all((g != 0).all() for g in grads)
    want = torch_steps(lambda p: make(torch, p), p0, grads)
    p, slots = [p0], [[np.zeros(64)] for _ in range(SLOTS[rule])]
    for it in range(3):
        p, slots, _ = keras_optimizer_step(rule, p, [grads[it]], slots, it, **hyper)
        np.testing.assert_allclose(p[0], want[it], rtol=1e-12, atol=1e-12, err_msg="{} step {}".format(name, it))
    assert np.abs(p[0] - p0).max() > 1e-3


# ------------------------------------------------------------------------------------------ the public classes
def test_each_optimizer_class_maps_to_its_rule_and_hyper_parameters():
    """fails on the commit before the rules existed: optimizer_settings read beta_1 off everything"""
    from speechless_amd import net
    import speechless_amd
    off = dict(decay=0.0, clipnorm=0.0, clipvalue=0.0)
    assert net.optimizer_settings(net.SGD()) == dict(optimizer="sgd", lr=0.01, momentum=0.0, nesterov=False, **off)
    assert net.optimizer_settings(net.SGD(0.1, momentum=0.9, nesterov=True, decay=0.5, clipnorm=2.0)) == dict(
        optimizer="sgd", lr=0.1, momentum=0.9, nesterov=True, decay=0.5, clipnorm=2.0, clipvalue=0.0)
    assert net.optimizer_settings(net.RMSprop()) == dict(optimizer="rmsprop", lr=0.001, rho=0.9, adam_epsilon=1e-8, **off)
    assert net.optimizer_settings(net.Adagrad()) == dict(optimizer="adagrad", lr=0.01, adam_epsilon=1e-8, **off)
    assert net.optimizer_settings(net.Adadelta()) == dict(optimizer="adadelta", lr=1.0, rho=0.95, adam_epsilon=1e-8, **off)
    assert net.optimizer_settings(net.Adamax(clipvalue=0.5)) == dict(
        optimizer="adamax", lr=0.002, beta_1=0.9, beta_2=0.999, adam_epsilon=1e-8, decay=0.0, clipnorm=0.0, clipvalue=0.5)
    for name in ("SGD", "RMSprop", "Adagrad", "Adadelta", "Adamax", "Adam"):
        assert getattr(speechless_amd, name) is getattr(net, name)


def test_a_keras_object_is_recognised_by_its_class_name_and_only_its_attributes_are_read():
    from speechless_amd.net import optimizer_settings

    class SGD:  # what a Keras 2.0 SGD carries: no beta_1, no epsilon; clipnorm only when it was passed
        lr, momentum, decay, nesterov = 0.05, 0.8, 0.1, True

    assert optimizer_settings(SGD()) == dict(optimizer="sgd", lr=0.05, momentum=0.8, nesterov=True, decay=0.1, clipnorm=0.0,
                                             clipvalue=0.0)

    class RMSprop:  # carries Adam's attribute names on top: still RMSprop
        lr, rho, epsilon, beta_1, beta_2 = 0.002, 0.8, 1e-7, 0.9, 0.999

    assert optimizer_settings(RMSprop())["optimizer"] == "rmsprop" and "beta_1" not in optimizer_settings(RMSprop())


def test_nadam_and_unknown_classes_raise_and_adam_is_what_it_was():
    from speechless_amd.net import Adam, optimizer_settings

    class Nadam:
        lr, beta_1, beta_2, epsilon, schedule_decay = 0.002, 0.9, 0.999, 1e-8, 0.004

    with pytest.raises(ValueError, match="Nadam"):
        optimizer_settings(Nadam())

    class Ftrl:
        lr = 0.1

    with pytest.raises(ValueError) as err:
        optimizer_settings(Ftrl())
    for name in ("Ftrl", "Adam", "SGD", "RMSprop", "Adagrad", "Adadelta", "Adamax"):
        assert name in str(err.value)
    assert optimizer_settings(Adam(1e-3, clipnorm=5.0, decay=0.25)) == dict(
        lr=1e-3, beta_1=0.9, beta_2=0.999, adam_epsilon=1e-8, decay=0.25, clipnorm=5.0, clipvalue=0.0)


# ------------------------------------------------------------------------------------------ the optimizer-state file
LAYERS = ["conv_a", "conv_b"]


def _state(rule, slots):
    rng = np.random.RandomState(len(rule))
    state = {"iterations": 7, "dropout_steps": 3}
    if rule != "adam":
        state["optimizer"] = rule
    for slot in ("m", "v")[:slots]:
        state[slot] = [(rng.randn(3, 4, 5).astype(np.float32), rng.randn(5).astype(np.float32)) for _ in LAYERS]
    return state


@pytest.mark.parametrize("rule,slots", [("sgd", 1), ("adadelta", 2), ("adam", 2)])
def test_optimizer_state_round_trip_through_an_npz_file(tmp_path, rule, slots):
    from speechless_amd.net import optimizer_state_from_arrays, optimizer_state_to_arrays
    state = _state(rule, slots)
    arrays = optimizer_state_to_arrays(state, LAYERS)
    assert ("optimizer" in arrays) == (rule != "adam")  # (an Adam file is what it always was)
    assert ("conv_a/kernel/v" in arrays) == (slots == 2)
    np.savez(str(tmp_path / "state.opt.npz"), **arrays)
    back = optimizer_state_from_arrays(np.load(str(tmp_path / "state.opt.npz")), LAYERS)
    assert sorted(back) == sorted(state)
    assert back.get("optimizer", "adam") == rule and back["iterations"] == 7 and back["dropout_steps"] == 3
    for slot in ("m", "v")[:slots]:
        for (w, b), (w2, b2) in zip(state[slot], back[slot]):
            assert np.array_equal(w, w2) and np.array_equal(b, b2)


def test_a_file_without_the_rule_key_is_adam_and_a_rule_mismatch_raises(tmp_path):
    from speechless_amd.engine import Engine
    from speechless_amd.net import optimizer_state_from_arrays, optimizer_state_to_arrays
    arrays = optimizer_state_to_arrays(_state("adam", 2), LAYERS)
    arrays.pop("optimizer", None)
    np.savez(str(tmp_path / "old.opt.npz"), **arrays)
    back = optimizer_state_from_arrays(np.load(str(tmp_path / "old.opt.npz")), LAYERS)
    assert "optimizer" not in back and "v" in back

    class Stub:  # Engine.set_optimizer_state up to its rule check, without a device
        optimizer = "sgd"

    with pytest.raises(ValueError) as err:
        Engine.set_optimizer_state(Stub(), back)
    assert "adam" in str(err.value) and "sgd" in str(err.value)
    Stub.optimizer = "adam"
    with pytest.raises(ValueError) as err:
        Engine.set_optimizer_state(Stub(), _state("adadelta", 2))
    assert "adam" in str(err.value) and "adadelta" in str(err.value)


def test_the_library_validates_the_optimizer_entry_points_without_a_gpu(hip_lib):
    """argument checks run before any launch"""
    from speechless_amd import _lib
    rule = _lib.OptRule()
    rule.rule, rule.lr, rule.momentum = _lib.OPT_RULES["sgd"], 0.01, 0.9
    step = hip_lib.raw("sl_optimizer_step")
    assert step(16, 16, 16, 16, 4, rule, None, 0.0, None) == -1  # a one-slot rule takes no second state pointer
    assert "s1" in hip_lib.last_error()
    assert step(16, 16, None, None, 4, rule, None, 0.0, None) == -1 and "null pointer" in hip_lib.last_error()
    assert step(16, 16, 16, None, 6, rule, None, 0.0, None) == -1 and "multiple of 4" in hip_lib.last_error()
    assert step(16, 16, 16, None, 4, rule, None, -1.0, None) == -1 and "clipvalue" in hip_lib.last_error()
    rule.rule = _lib.OPT_RULES["adadelta"]
    assert step(16, 16, 16, None, 4, rule, None, 0.0, None) == -1 and "s1" in hip_lib.last_error()
    rule.rule = _lib.OPT_RULES["adam"]
    assert step(16, 16, 16, 16, 4, rule, None, 0.0, None) == -1 and "sl_adam" in hip_lib.last_error()
    rule.rule = 17
    assert step(16, 16, 16, 16, 4, rule, None, 0.0, None) == -1 and "unknown rule" in hip_lib.last_error()
    table = (_lib.AdamLayer * 1)()
    rule.rule = _lib.OPT_RULES["rmsprop"]
    for name, args in (("sl_optimizer_pack_layers", (table, 17, _lib.SL_BF16, rule, None, 0.0, None)),
                       ("sl_split3_optimizer_pack_layers", (table, 0, rule, None, 0.0, None)),
                       ("sl_splitf16_optimizer_pack_layers", (table, 17, rule, 64.0, None, 0.0, None))):
        assert hip_lib.raw(name)(16, 16, 16, None, *args) == -1 and "layers per call" in hip_lib.last_error(), name
    assert hip_lib.raw("sl_optimizer_pack_layers")(16, 16, 16, None, table, 1, _lib.SL_BF16, rule, None, 0.0, None) == -1
    assert "w_fwd" in hip_lib.last_error()  # (the table's own checks: an empty layer entry)
