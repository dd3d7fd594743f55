"""GPU: clipping by global norm in the device optimiser (dcgp_model_set_grad_clip / dcgp_model_grad_norms; csrc/optim.hip's two norm kernels and
the clipped instance of the update).  Adam at t = 1 moves every element by -+lr whatever the gradient's scale, so the evidence is the moments
(``optimizer_state``), the reported norm, and SGD's parameter steps -- never Adam's parameters."""
import numpy as np
import pytest

import live_specs as ls
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec

pytestmark = pytest.mark.gpu

HWC, N, LR = (12, 12, 1), 4, 0.01
B1, B2 = 0.9, 0.999
# small: a few blocks per group, groups of 3 and 1 ... elements, no count a multiple of 256.  wide: a head alone, M = 96, R = 10 -- q_sqrt has
# 92 160 elements = 360 blocks, more partial sums than the final stage's block has threads
SHAPES = {"small": dict(convs=[(3, 1, 2)], M=8), "wide": dict(convs=[], M=96)}


def _case(shape):
    k = SHAPES[shape]
    spec = syn.make_spec(HWC, k["convs"], (3, 1), k["M"], S=2, conv_q_sqrt_scale=0.3)
    X, Y = syn.make_batch(HWC, N, seed=3)
    return spec, X, Y, [syn.make_noise(spec, N, seed=70 + t) for t in range(4)]


def _factor(x):
    return -np.expm1(-(x - 1e-6))


def _g_u(model, grads, frozen=()):
    """{group key: g_u} on the host from fetched gradients and the parameters they were taken at: the lower triangle of q_sqrt, the softplus
    factor on the positive parameters, frozen groups left out.  Second value: the number of summed elements."""
    out, n = {}, 0
    for li, (g, now) in enumerate(zip(grads, ls.model_values(model))):
        per = {"Z": g["Z"], "q_mu": g["q_mu"], "q_sqrt": np.tril(g["q_sqrt"])}
        if "patch_weights" in g:
            per["w"] = g["patch_weights"]
        per["hyper"] = np.array([g["variance"] * _factor(now["variance"]), g["lengthscales"] * _factor(now["lengthscales"]), 0.0])
        for name, val in per.items():
            if (li, name) in frozen:
                continue
            out["layers/%d/%s" % (li, name)] = np.asarray(val, np.float64)
            if name == "q_sqrt":
                n += val.shape[0] * val.shape[1] * (val.shape[1] + 1) // 2
            else:
                n += 2 if name == "hyper" else int(np.size(val))
    return out, n


def _norm(gu):
    return float(np.sqrt(sum(np.sum(np.square(v)) for v in gu.values())))


def _everything(model):
    model.pull_parameters()
    out = {"L%d/%s" % (li, k): np.asarray(v) for li, d in enumerate(ls.model_values(model)) for k, v in d.items()}
    out.update({"opt/" + k: np.asarray(v) for k, v in model.optimizer_state().items()})
    return out


@pytest.mark.parametrize("shape", ["small", "wide"])
@pytest.mark.parametrize("freeze", [False, True])
def test_reported_norm_is_numpys(ctx, shape, freeze):
    spec, X, Y, zs = _case(shape)
    model = build_from_spec(spec, X, Y)
    last = len(model.layers) - 1
    frozen = [(0, "Z"), (last, "q_sqrt")] if freeze else []
    for li, name in frozen:
        model.set_trainable(li, name, False)
    model.set_grad_clip(np.inf)
    assert model.last_grad_norms.size == 0
    _, g = model.compute_gradients(X, Y, zs=zs[1])
    model.adam_step(LR)
    got = model.last_grad_norms
    gu, n = _g_u(model, g, frozen)          # (the Python-side values are still the ones the gradient was taken at: nothing was pulled)
    want, bound = _norm(gu), 8 * n * 2.0 ** -53
    print("norm %s freeze=%d: device %.17g numpy %.17g rel %.3e bound %.3e (n = %d)" % (shape, freeze, got[0], want, abs(got[0] - want) / want, bound, n))
    assert got.shape == (1,) and abs(got[0] - want) <= bound * want
    model.close()


def _run(route, model, X, Y, zs, steps=3):
    """`steps` steps through one of the four routes; (ELBOs, norms per step)."""
    elbos, norms = [], []
    if route == "train_run":
        model.attach_dataset()
        idx = np.array([[0, 1, 2, 3], [2, 3, 1, 0], [3, 0, 2, 1]])[:steps]
        elbos = list(model.train_run(idx, LR, seed=5))
        return elbos, list(model.last_grad_norms)
    for t in range(1, steps + 1):
        if route == "train_step":
            elbos.append(model.train_step(X, Y, LR, zs=zs[t]))
        else:
            elbos.append(model.compute_gradients(X, Y, zs=zs[t], fetch=False)[0])
            model.adam_step(LR) if route == "adam_step" else model.sgd_step(1e-7)
        norms.extend(model.last_grad_norms)
    return elbos, norms


@pytest.mark.parametrize("shape", ["small", "wide"])
@pytest.mark.parametrize("route", ["adam_step", "train_step", "sgd_step", "train_run"])
def test_scale_one_is_the_unclipped_step_to_the_bit(ctx, shape, route):
    spec, X, Y, zs = _case(shape)
    plain = build_from_spec(spec, X, Y)
    e0, n0 = _run(route, plain, X, Y, zs)
    assert n0 == []
    want = _everything(plain)
    plain.close()
    seen = None
    for which in ("inf", "twice the largest"):
        twin = build_from_spec(spec, X, Y)
        twin.set_grad_clip(np.inf if seen is None else 2.0 * max(seen))
        e1, n1 = _run(route, twin, X, Y, zs)
        assert len(n1) == 3 and all(np.isfinite(n1)) and all(v > 0 for v in n1)
        assert seen is None or n1 == seen
        seen = n1
        assert e1 == e0, which
        got = _everything(twin)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (which, k))
        twin.close()


@pytest.mark.parametrize("shape", ["small", "wide"])
def test_clipped_adam_step_leaves_the_scaled_gradient_in_the_moments(ctx, shape):
    spec, X, Y, zs = _case(shape)
    probe = build_from_spec(spec, X, Y)
    probe.set_grad_clip(np.inf)
    probe.compute_gradients(X, Y, zs=zs[1], fetch=False)
    probe.adam_step(LR)
    max_norm = 0.1 * probe.last_grad_norms[0]
    probe.close()
    model = build_from_spec(spec, X, Y)
    model.set_grad_clip(max_norm)
    _, g = model.compute_gradients(X, Y, zs=zs[1])
    model.adam_step(LR)
    norm = model.last_grad_norms[0]
    c = max_norm / max(norm, max_norm)
    assert abs(c - 0.1) < 1e-12
    gu, _ = _g_u(model, g)
    st = model.optimizer_state()
    for key, val in gu.items():
        np.testing.assert_allclose(st[key + "/m"], (1 - B1) * c * -val, rtol=1e-14, atol=0, err_msg=key)
        np.testing.assert_allclose(st[key + "/v"], (1 - B2) * (c * val) ** 2, rtol=1e-14, atol=0, err_msg=key)
    model.close()


@pytest.mark.parametrize("shape", ["small", "wide"])
def test_clipped_sgd_step_moves_by_the_scaled_gradient(ctx, shape):
    """Identity-transform groups: p_new - p_old against lr c g.  The difference carries p_new's own rounding, half an ulp of |p| < 8, i.e. up to
    8.9e-16 absolute, whatever the step; so lr is chosen to make the clipped step 0.5 long (its largest element is then >= 0.5 / sqrt(n) > 1e-3)
    and the 1e-12 is taken relative to the largest element of lr c g over all groups."""
    spec, X, Y, zs = _case(shape)
    model = build_from_spec(spec, X, Y)
    model.set_grad_clip(np.inf)
    _, g = model.compute_gradients(X, Y, zs=zs[1])
    model.sgd_step(1e-12)
    max_norm = 0.1 * model.last_grad_norms[0]
    model.close()
    model = build_from_spec(spec, X, Y)
    model.set_grad_clip(max_norm)
    _, g = model.compute_gradients(X, Y, zs=zs[1])
    before = ls.model_values(model)
    lr = 0.5 / max_norm
    model.sgd_step(lr)
    c = max_norm / max(model.last_grad_norms[0], max_norm)
    model.pull_parameters()
    after = ls.model_values(model)
    diff, want = [], []
    for li in range(len(after)):
        for name in ("Z", "q_mu", "q_sqrt") + (("patch_weights",) if "patch_weights" in after[li] else ()):
            gr = np.tril(g[li][name]) if name == "q_sqrt" else g[li][name]
            diff.append((after[li][name] - before[li][name]).ravel())
            want.append((lr * c * gr).ravel())
    diff, want = np.concatenate(diff), np.concatenate(want)
    err = np.max(np.abs(diff - want)) / np.max(np.abs(want))
    print("clipped SGD %s: c %.6f, largest step %.3e, error relative to it %.3e" % (shape, c, np.max(np.abs(want)), err))
    assert c < 0.11 and err <= 1e-12
    model.close()


def test_train_run_with_clipping_is_the_per_step_loop(ctx):
    spec, X, Y, zs = _case("small")
    probe = build_from_spec(spec, X, Y)
    probe.set_grad_clip(np.inf)
    _, norms = _run("train_run", probe, X, Y, zs)
    probe.close()
    max_norm = 0.5 * min(norms)
    a, b = build_from_spec(spec, X, Y), build_from_spec(spec, X, Y)
    a.set_grad_clip(max_norm), b.set_grad_clip(max_norm)
    ea, na = _run("train_run", a, X, Y, zs)
    idx = np.array([[0, 1, 2, 3], [2, 3, 1, 0], [3, 0, 2, 1]])
    eb, nb = [], []
    for i in range(3):
        eb.append(b.train_step(X[idx[i]], Y[idx[i]], LR, seed=5 + i))
        nb.extend(b.last_grad_norms)
    assert len(na) == 3 and na == nb and ea == eb and all(v > max_norm for v in na)
    wa, wb = _everything(a), _everything(b)
    for k in wa:
        np.testing.assert_array_equal(wa[k], wb[k], err_msg=k)
    a.close(), b.close()


def test_refusals_and_the_off_state(ctx):
    spec, X, Y, zs = _case("small")
    model = build_from_spec(spec, X, Y)
    model.compute_gradients(X, Y, zs=zs[1], fetch=False)
    model.adam_step(LR)
    assert model.last_grad_norms.size == 0                     # off: nothing is measured
    with pytest.raises(ValueError):
        model.set_grad_clip(-1.0)
    with pytest.raises(ValueError):
        model.set_grad_clip(float("nan"))
    L = dev.lib()
    assert L.dcgp_model_set_grad_clip(model._model, -1.0) == dev.ERR_ARG and L.dcgp_model_set_grad_clip(model._model, float("nan")) == dev.ERR_ARG
    model.set_grad_clip(3.0)
    before = _everything(model)
    model.compute_gradients(X, Y, zs=zs[2], fetch=False)
    with pytest.raises(dev.DcgpError, match="shard"):
        model.debug_sharded_adam(2, LR)
    after = _everything(model)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    model.set_grad_clip(0.0)
    model.adam_step(LR)
    assert model.last_grad_norms.size == 0
    model.close()
