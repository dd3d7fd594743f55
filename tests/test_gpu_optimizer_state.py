"""GPU: the device optimiser's state through ``DGP_Base.optimizer_state`` / ``set_optimizer_state`` (dcgp_model_get_adam_state, _set_adam_state,
_get_adam_t, _set_adam_t; csrc/optim.hip): a fresh model's zeros, the moments after two steps against NumPy Adam on the device's own fetched
gradients, a transplant of parameters and state into a second model that then takes the same third step to the bit, and the refusals."""
import copy

import numpy as np
import pytest

import live_specs as ls
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import Gaussian
from deepcgp_amd.models import build_from_spec

pytestmark = pytest.mark.gpu

HWC, N, LR = (12, 12, 1), 4, 0.05
B1, B2 = 0.9, 0.999


def _spec(**kw):
    return syn.make_spec(HWC, [(3, 1, 2)], (3, 1), 8, S=2, conv_q_sqrt_scale=0.3, **kw)


def _data(spec, seed=3):
    X, Y = syn.make_batch(HWC, N, seed=seed)
    return X, Y, [syn.make_noise(spec, N, seed=50 + t) for t in range(4)]


def _spec_follows(spec, model):
    """The spec's values <- the device's (the mirror then starts every step from the numbers the kernel starts from)."""
    model.pull_parameters()
    for l, now in zip(spec["convs"] + [spec["head"]], ls.model_values(model)):
        for name, val in now.items():
            l[ls.SPEC_KEY[name]] = val


def _moments(m, v, g, x=None):
    """One Adam moment update from the ascent gradient g (softplus factor for a positive parameter at x)."""
    g = -np.asarray(g, np.float64)
    if x is not None:
        g = g * (1.0 - np.exp(-(x - 1e-6)))
    return B1 * m + (1 - B1) * g, B2 * v + (1 - B2) * g * g


def _hyper(state, li, k):
    return np.array([state[(li, "variance")][k], state[(li, "lengthscales")][k], 0.0])      # (an RBF layer's third slot never moves)


def test_fresh_model_reports_zeros(ctx):
    spec = _spec()
    X, Y, _ = _data(spec)
    model = build_from_spec(spec, X, Y)
    st = model.optimizer_state()
    assert st["t"] == 0
    want = {"layers/%d/%s/%s" % (li, g, k) for li in (0, 1) for g in ("Z", "q_mu", "q_sqrt", "hyper") for k in "mv"} | {"layers/1/w/m", "layers/1/w/v", "t"}
    assert set(st) == want
    for li, l in enumerate(model.layers):
        assert st["layers/%d/Z/m" % li].shape == np.shape(l.feature.Z) and st["layers/%d/q_sqrt/v" % li].shape == np.shape(l.q_sqrt)
        assert st["layers/%d/hyper/m" % li].shape == (3,)
    assert all(not np.any(v) for k, v in st.items() if k != "t")
    model.close()


def test_moments_after_two_steps_match_numpy_adam(ctx):
    spec = copy.deepcopy(_spec())
    X, Y, zs = _data(spec)
    model = build_from_spec(spec, X, Y)
    state = {}
    for t in (1, 2):
        _spec_follows(spec, model)
        _, g = model.compute_gradients(X, Y, zs=zs[t])
        model.train_step(X, Y, LR, zs=zs[t])
        ls.adam_numpy_step(spec, g, state, LR, t)
    st = model.optimizer_state()
    assert st["t"] == 2
    worst = 0.0
    for li in (0, 1):
        pairs = [("Z", "Z"), ("q_mu", "q_mu"), ("q_sqrt", "q_sqrt")] + ([("w", "patch_weights")] if li == 1 else [])
        for k, which in enumerate("mv"):
            for group, name in pairs:
                got, want = st["layers/%d/%s/%s" % (li, group, which)], state[(li, name)][k]
                worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))))
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg="L%d %s %s" % (li, group, which))
            np.testing.assert_allclose(st["layers/%d/hyper/%s" % (li, which)], _hyper(state, li, k), rtol=1e-12, atol=0)
    print("moments after two steps: worst relative difference %.3e" % worst)
    assert np.any(st["layers/0/Z/m"]) and np.any(st["layers/1/w/v"])
    model.close()


def test_likelihood_and_mean_filter_moments(ctx):
    """The two groups live_specs' mirror does not know: the Gaussian variance's slot and a trainable LinearConv2dMean's filter."""
    spec = _spec(head_outputs=3)
    spec["convs"][0]["mean_filter"] = 0.1 * np.random.default_rng(1).standard_normal((3, 3, 1, 2))
    spec["convs"][0]["mean_trainable"] = True
    X, _, zs = _data(spec)
    Y = np.random.default_rng(2).standard_normal((N, 3))
    model = build_from_spec(spec, X, Y, likelihood=Gaussian(0.8))
    assert not np.any(model.optimizer_state()["likelihood/m"]) and model.optimizer_state()["layers/0/mean_filter/m"].shape == (3, 3, 1, 2)
    mW, vW, ml, vl = 0.0, 0.0, 0.0, 0.0
    for t in (1, 2):
        model.pull_parameters()
        s2 = float(model.likelihood.variance)
        _, g = model.compute_gradients(X, Y, zs=zs[t])
        model.train_step(X, Y, LR, zs=zs[t])
        mW, vW = _moments(mW, vW, g[0]["mean_filter"])
        ml, vl = _moments(ml, vl, g[-1]["likelihood_variance"], x=s2)
    st = model.optimizer_state()
    assert st["t"] == 2
    np.testing.assert_allclose(st["layers/0/mean_filter/m"], mW, rtol=1e-12, atol=0)
    np.testing.assert_allclose(st["layers/0/mean_filter/v"], vW, rtol=1e-12, atol=0)
    np.testing.assert_allclose(st["likelihood/m"], [ml], rtol=1e-12, atol=0)
    np.testing.assert_allclose(st["likelihood/v"], [vl], rtol=1e-12, atol=0)
    assert np.any(mW) and ml != 0.0
    model.close()


def _copy_values(dst, src):
    for a, b in zip(dst.layers, src.layers):
        head = b is src.layers[-1]
        ka, kb = (a.kern.base_kernel, b.kern.base_kernel) if head else (a.base_kernel, b.base_kernel)
        a.feature.Z, a.q_mu, a.q_sqrt = np.array(b.feature.Z), np.array(b.q_mu), np.array(b.q_sqrt)
        ka.variance, ka.lengthscales = float(kb.variance), float(kb.lengthscales)
        if head:
            a.kern.patch_weights = np.array(b.kern.patch_weights)
    dst.sync_parameters()


def _everything(model):
    model.pull_parameters()
    out = {"L%d/%s" % (li, k): np.asarray(v) for li, d in enumerate(ls.model_values(model)) for k, v in d.items()}
    out.update({"opt/" + k: np.asarray(v) for k, v in model.optimizer_state().items()})
    return out


def test_transplanted_state_continues_to_the_bit(ctx):
    spec = _spec()
    X, Y, zs = _data(spec)
    a = build_from_spec(spec, X, Y)
    for t in (1, 2):
        a.train_step(X, Y, LR, zs=zs[t])
    a.pull_parameters()
    b, c = build_from_spec(copy.deepcopy(spec), X, Y), build_from_spec(copy.deepcopy(spec), X, Y)
    _copy_values(b, a)
    _copy_values(c, a)
    b.set_optimizer_state(a.optimizer_state())
    elbos = [m.train_step(X, Y, LR, zs=zs[3]) for m in (a, b, c)]
    assert elbos[0] == elbos[1] == elbos[2]                  # the same parameters went in
    ea, eb, ec = _everything(a), _everything(b), _everything(c)
    assert ea["opt/t"] == 3 and eb["opt/t"] == 3 and ec["opt/t"] == 1
    for k in ea:
        np.testing.assert_array_equal(eb[k], ea[k], err_msg=k)
    # without the state the same step goes elsewhere: zero moments and t = 1
    assert not np.array_equal(ec["L0/q_mu"], ea["L0/q_mu"]) and not np.array_equal(ec["L1/q_mu"], ea["L1/q_mu"])
    for m in (a, b, c):
        m.close()


def test_refusals_leave_the_state_alone(ctx):
    spec = _spec()
    X, Y, zs = _data(spec)
    model = build_from_spec(spec, X, Y)
    model.train_step(X, Y, LR, zs=zs[1])
    before = model.optimizer_state()
    L = dev.lib()
    big = np.ones(4096)

    def refused(rc, word):
        assert rc == dev.ERR_ARG
        msg = L.dcgp_last_error(model._ctx.handle).decode()
        assert word in msg, msg

    nZ = before["layers/0/Z/m"].size
    for fn in (L.dcgp_model_set_adam_state, L.dcgp_model_get_adam_state):
        refused(fn(model._model, 0, b"Z", big.ctypes.data, big.ctypes.data, nZ + 1), "expected")
        refused(fn(model._model, 0, b"momentum", big.ctypes.data, big.ctypes.data, 3), "unknown")
        refused(fn(model._model, 0, b"w", big.ctypes.data, big.ctypes.data, 100), "only the head")
        refused(fn(model._model, 0, b"likelihood", big.ctypes.data, big.ctypes.data, 1), "likelihood")      # a MultiClass model has no slot
        refused(fn(model._model, 7, b"Z", big.ctypes.data, big.ctypes.data, nZ), "no layer")
        refused(fn(model._model, 0, b"mean_filter", big.ctypes.data, big.ctypes.data, 18), "no mean filter")
    refused(L.dcgp_model_set_adam_t(model._model, -1), ">= 0")
    for bad, word in (({k: v for k, v in before.items() if k != "layers/1/w/v"}, "layers/1/w/v"),
                      (dict(before, extra=np.zeros(1)), "extra"),
                      (dict(before, **{"layers/0/q_mu/m": np.zeros((8, 3))}), "layers/0/q_mu/m")):
        with pytest.raises(ValueError, match=word):
            model.set_optimizer_state(bad)
    after = model.optimizer_state()
    assert set(after) == set(before)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    model.close()
