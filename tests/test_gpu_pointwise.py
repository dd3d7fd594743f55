"""GPU: the shared kernels of the four per-output likelihoods (csrc/pointwise.hip: Gaussian, Bernoulli, StudentT, Poisson) at the head
widths where their element mapping changes shape -- against the references the per-likelihood tests use (test_gpu_gaussian.numpy_elbo,
tests/bernoulli_ref.py, tests/quad_ref.py, compose_ref.torch_reference) at those tests' tolerances.

Head-only models, M = 8, images 6 x 6 x 1, S = 2: the head has S N rows over N label rows, so a row reads y[row % N].  The ELBO tail gives a
workgroup max(1, 256 / K) whole rows, the reverse tail 256 flat elements:

    K = 1,    N = 129   258 rows: 256 per workgroup, a second, partial workgroup; the rows' sum runs over more than 256 of them
    K = 3,    N = 43    86 rows: 85 per workgroup (255 live threads, one idle), one row in the second; 258 flat elements in the reverse
                        tail = two workgroups, so the parameter's gradient (Gaussian variance, StudentT scale) is reduced across partials
    K = 10,   N = 13    26 rows: 25 per workgroup
    K = 256, 300, N = 3 one row per workgroup; at 300 the element loop is longer than the workgroup
    K = 1030, N = 3     a row wider than the tail's 1024 doubles of LDS: two chunks, the row's sum carried across them
"""
import numpy as np
import pytest

import bernoulli_ref as br
import compose_ref
import quad_ref as qr
from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
from test_gpu_gaussian import numpy_elbo

pytestmark = pytest.mark.gpu

HWC, M, S = (6, 6, 1), 8, 2
SHAPES = {1: 129, 3: 43, 10: 13, 256: 3, 300: 3, 1030: 3}      # K -> N
LIKS = [("gaussian", 0.7), ("bernoulli",), ("studentt", 0.7, 4.5), ("poisson", 2.5)]
_CASES = {}


def lik_id(lik):
    return "-".join(str(t) for t in lik)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def make_case(K, lik):
    """(spec, X, Ylab, Y, zs), made once per (K, likelihood); the per-likelihood tests' targets: standard normal (StudentT: one outlier at 8),
    fair coin flips, poisson(2.5) with a 0."""
    if (K, lik) in _CASES:
        return _CASES[(K, lik)]
    N = SHAPES[K]
    spec = syn.make_spec(HWC, [], (3, 1), M, S=S, num_data=300, seed=7, conv_q_sqrt_scale=0.3, variance=2.0, ls=1.5, head_outputs=K)
    X, Ylab = syn.make_batch(HWC, N, seed=7)
    rng = np.random.default_rng(7)
    if lik[0] == "bernoulli":
        Y = (rng.random((N, K)) < 0.5).astype(np.float64)
    elif lik[0] == "poisson":
        Y = rng.poisson(2.5, (N, K)).astype(np.float64)
        Y[0, 0] = 0.0
    else:
        Y = rng.standard_normal((N, K))
        if lik[0] == "studentt":
            Y[N // 2, K // 2] = 8.0
    for a in (X, Y):
        a.setflags(write=False)
    _CASES[(K, lik)] = (spec, X, Ylab, Y, syn.make_noise(spec, N, seed=7))
    return _CASES[(K, lik)]


def reference_elbo(lik, spec, X, Ylab, Y, zs, K):
    if lik[0] == "gaussian":
        return numpy_elbo(spec, X, Ylab, Y, zs, lik[1])
    if lik[0] == "bernoulli":
        return br.elbo(spec, X, Ylab, Y, zs)
    return qr.elbo(lik, spec, X, Ylab, Y, zs, key=("pointwise", K))


@pytest.mark.parametrize("lik", LIKS, ids=lik_id)
@pytest.mark.parametrize("K", sorted(SHAPES))
def test_elbo_and_predict_y(ctx, K, lik):
    spec, X, Ylab, Y, zs = make_case(K, lik)
    want, wdata, wkl = reference_elbo(lik, spec, X, Ylab, Y, zs, K)
    model = build_from_spec(spec, X, Y, likelihood=compose_ref.make_likelihood(lik))
    e, data, kl = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    print("K=%d %s: data term rel %.3e, ELBO rel %.3e" % (K, lik[0], abs(data - wdata) / abs(wdata), abs(e - want) / abs(want)))
    assert abs(data - wdata) <= 1e-10 * abs(wdata), (data, wdata)
    assert abs(e - want) <= 1e-10 * abs(want), (e, want)
    assert abs(kl - wkl) <= 1e-10 * abs(wkl)
    # predict_y on the device's own marginals, as the per-likelihood tests compare it
    fm, fv = model.predict_f(X, S, zs=zs)
    pm, pv = model.predict_y(X, S, zs=zs)
    assert pm.shape == pv.shape == (S, SHAPES[K], K)
    if lik[0] == "gaussian":
        assert np.array_equal(pm, fm) and np.array_equal(pv, fv + lik[1])
    else:
        wm, wv = br.predict_mean_and_var(fm, fv) if lik[0] == "bernoulli" else qr.predict_mean_and_var(lik, fm, fv)
        assert rel(pm, wm) < 1e-12 and rel(pv, wv) < 1e-12
    model.close()


@pytest.mark.parametrize("lik", LIKS, ids=lik_id)
@pytest.mark.parametrize("K", sorted(SHAPES))
def test_evaluate_equals_a_predict_density_loop(ctx, K, lik):
    """evaluate's per-image log density: the bits of predict_density's per-output values added in index order."""
    spec, X, Ylab, Y, zs = make_case(K, lik)
    N = SHAPES[K]
    model = build_from_spec(spec, X, Y, likelihood=compose_ref.make_likelihood(lik))
    for batch in (1, 4):
        out = model.evaluate(X, Y, S=S, batch_size=batch, seed=21, per_image=True)
        loop, ym = [], []
        for i, lo in enumerate(range(0, N, batch)):
            sl = slice(lo, lo + batch)
            ld = model.predict_density(X[sl], Y[sl], S, seed=21 + i)
            assert ld.shape == (len(X[sl]), K)
            loop.append(np.cumsum(ld, axis=1)[:, -1])          # (index order: the device's)
            ym.append(model.predict_y(X[sl], S, seed=21 + i)[0].mean(0))
        loop, ym = np.concatenate(loop), np.concatenate(ym)
        assert np.array_equal(out["log_density"], loop), (batch, rel(out["log_density"], loop))
        assert abs(out["mean_log_density"] - loop.mean()) <= 1e-12 * abs(loop.mean())
        got = out["p_mean"] if lik[0] == "bernoulli" else out["y_mean"]
        assert rel(got, ym) < 1e-12 and out["n"] == N
        if lik[0] == "bernoulli":
            assert out["accuracy"] == np.mean((got > 0.5) == (Y == 1))
        else:
            rmse = np.sqrt(np.mean(np.square(got - Y)))
            assert abs(out["rmse"] - rmse) <= 1e-12 * rmse
    model.close()


@pytest.mark.parametrize("lik", LIKS, ids=lik_id)
@pytest.mark.parametrize("K", [3, 10])
def test_gradient_vs_torch_autograd(ctx, K, lik):
    pytest.importorskip("torch")
    spec, X, Ylab, Y, zs = make_case(K, lik)
    parts, want, dlik = compose_ref.torch_reference(spec, X, Y, zs, lik)
    model = build_from_spec(spec, X, Y, likelihood=compose_ref.make_likelihood(lik))
    e, g = model.compute_gradients(X, Y, zs=zs)
    assert abs(e - parts[0]) <= 1e-10 * abs(parts[0])
    for li, groups in enumerate(want):
        for name, w in groups.items():
            got = np.tril(g[li][name]) if name == "q_sqrt" else g[li][name]
            assert np.abs(got - w).max() <= 1e-8 * max(1.0, np.abs(w).max()), (li, name)
    if lik[0] in compose_ref.LIK_PARAM:      # reduced across the reverse tail's workgroups (two at K = 3)
        got = g[-1][compose_ref.LIK_PARAM[lik[0]]]
        print("K=%d %s: d / d parameter %.12g, autograd %.12g" % (K, lik[0], got, float(dlik)))
        assert float(dlik) != 0.0 and abs(got - float(dlik)) <= 1e-8 * max(1.0, abs(float(dlik)))
    else:
        assert dlik is None and not any(n in g[-1] for n in compose_ref.LIK_PARAM.values())
    model.close()
