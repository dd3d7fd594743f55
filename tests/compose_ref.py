"""Test helper: ONE torch forward (float64, CPU) for every combination of likelihood, base kernel, padding, per-layer M and whitening, and
mean function (tests/test_host_compose.py, tests/test_gpu_compose.py).

The layers are tests/torch_ref.py's ``forward`` -- padding, the RBF / Matern / ArcCosine Gram matrices, Conv2dMean's centre pixel, the mean
filter as a leaf -- and the likelihood term is a rule ``ve(m, v)`` on the head's marginals [S, N, D], D the
head width of the spec.  Every rule is the one the repository already has:

    ("robustmax", K)             test_oracle_autograd._robustmax_ve (torch_ref.forward's own tail)
    ("softmax", K, Q, seed)      test_gpu_softmax._torch_rule on likelihoods.Softmax(K, Q, seed).nodes
    ("gaussian", s2)             test_gpu_gaussian._torch_gauss_rule, s2 a leaf
    ("bernoulli",)               test_gpu_bernoulli._torch_bern_rule (tests/bernoulli_ref.py's probit rule at the device's 20 nodes)
    ("studentt", scale, nu)      quad_ref.torch_ve, the scale a leaf
    ("poisson", binsize)         quad_ref.torch_ve

Predictive mean, variance and log density come from the NumPy references (softmax_ref, bernoulli_ref, quad_ref; RobustMax:
test_oracle_autograd._robustmax_predict; Gaussian: the closed form tests/test_gpu_gaussian.py::test_predictions writes) fed with the torch
marginals.  Test infrastructure only."""
import numpy as np

import torch_ref as tr

LIK_PARAM = {"gaussian": "likelihood_variance", "studentt": "likelihood_scale"}      # the names DGP_Base.compute_gradients uses
FLOAT_TARGETS = ("gaussian", "bernoulli", "studentt", "poisson")


def make_likelihood(lik):
    """The library's likelihood object of a tuple."""
    from deepcgp_amd import likelihoods as L
    kind = lik[0]
    if kind == "robustmax":
        return L.MultiClass(lik[1])
    if kind == "softmax":
        return L.Softmax(lik[1], lik[2], seed=lik[3])
    if kind == "gaussian":
        return L.Gaussian(lik[1])
    if kind == "bernoulli":
        return L.Bernoulli()
    if kind == "studentt":
        return L.StudentT(lik[1], lik[2])
    assert kind == "poisson", lik
    return L.Poisson(binsize=lik[1])


def softmax_nodes(lik):
    return np.array(make_likelihood(lik).nodes, np.float64)


def rule(lik, Y):
    """(ve or None, the likelihood's own leaf or None): ``ve(m, v)`` as torch_ref.forward takes it; None = its RobustMax tail."""
    import torch
    kind = lik[0]
    if kind == "robustmax":
        return None, None
    if kind == "softmax":
        from test_gpu_softmax import _torch_rule
        nodes = softmax_nodes(lik)
        return (lambda m, v: _torch_rule(m, v, Y, nodes, "elbo")), None
    Yf = np.asarray(Y, np.float64)
    assert Yf.ndim == 2, Yf.shape
    yt = torch.tensor(Yf, dtype=torch.float64)[None]
    if kind == "gaussian":
        from test_gpu_gaussian import _torch_gauss_rule
        s2 = torch.tensor(lik[1], dtype=torch.float64, requires_grad=True)
        return (lambda m, v: _torch_gauss_rule(m, v, yt, s2)), s2
    if kind == "bernoulli":
        from test_gpu_bernoulli import _torch_bern_rule
        return (lambda m, v: _torch_bern_rule(m, v, Yf)), None
    import quad_ref as qr
    scale = torch.tensor(lik[1], dtype=torch.float64, requires_grad=True) if kind == "studentt" else None
    return (lambda m, v: qr.torch_ve(lik, m, v, yt.expand(m.shape), scale)), scale


def torch_forward(spec, X, Y, zs, lik, x_leaf=False):
    """torch_ref.forward's dict with the likelihood's rule as its tail, plus ``lik_leaf`` (the variance / scale tensor or None)."""
    D = spec["head"]["R"]
    assert lik[0] not in ("robustmax", "softmax") or lik[1] == D, (lik, D)
    ve, leaf = rule(lik, Y)
    out = tr.forward(spec, X, Y, zs, x_leaf=x_leaf, ve=ve)
    assert out["mean"].shape[2] == D
    out["lik_leaf"] = leaf
    return out


def _gradients(out):
    want, extra = tr.gradients(out, [] if out["lik_leaf"] is None else [out["lik_leaf"]])
    return want, (extra[0] if extra else None)


def torch_reference(spec, X, Y, zs, lik):
    """((ELBO, data term, KL), [per-layer {group: gradient}] in compute_gradients' names -- ``mean_filter`` among a conv layer's, q_sqrt's cut to
    the lower triangle --, d ELBO / d the likelihood's own parameter or None)."""
    out = torch_forward(spec, X, Y, zs, lik)
    want, dlik = _gradients(out)
    return (out["elbo"].item(), out["data"].sum().item(), out["kl"].item()), want, dlik


def torch_input_gradient(spec, X, Y, zs, lik):
    """(J [N], dX [N, H W C]) of DGP_Base.input_gradient(objective="elbo"): J_n = 1/S sum_s E_q[log p(y_n | f_sn)]."""
    return tr.input_gradient(spec, X, Y, zs, tr.data_term, ve=rule(lik, Y)[0])


def _logmeanexp(l):
    from scipy.special import logsumexp
    return logsumexp(l, axis=0) - np.log(l.shape[0])


def predictions(lik, m, v, Y):
    """(E_y, V_y [S, N, D], log density) from the head's marginals m, v [S, N, D] (NumPy): what ``predict_y`` and ``predict_density`` return --
    the density [N, 1] for the label likelihoods, [N, D] for the float-target ones."""
    kind = lik[0]
    S, N, D = m.shape
    if kind == "robustmax":
        import torch
        from test_oracle_autograd import _robustmax_predict
        p = _robustmax_predict(torch.tensor(m.reshape(S * N, D)), torch.tensor(v.reshape(S * N, D))).numpy().reshape(S, N, D)
        return p, p - p * p, _logmeanexp(np.log(p[:, np.arange(N), np.reshape(Y, (-1,))]))[:, None]
    if kind == "softmax":
        import softmax_ref as sr
        nodes = softmax_nodes(lik)
        p, pv = sr.predict_mean_and_var(m, v, nodes)
        return p, pv, sr.predict_density(m, v, Y, nodes)[:, None]
    Y = np.asarray(Y, np.float64)
    if kind == "gaussian":
        s2 = lik[1]
        l = -0.5 * (np.log(2 * np.pi) + np.log(v + s2)) - 0.5 * np.square(Y[None] - m) / (v + s2)
        return m, v + s2, _logmeanexp(l)
    if kind == "bernoulli":
        import bernoulli_ref as br
        p, pv = br.predict_mean_and_var(m, v)
        return p, pv, br.predict_density(m, v, Y)
    import quad_ref as qr
    e, ev = qr.predict_mean_and_var(lik, m, v)
    return e, ev, qr.predict_density(lik, m, v, Y)


def reference(spec, X, Y, zs, lik):
    """Everything the GPU test compares, from ONE forward: dict(parts (ELBO, data, KL), want [per-layer groups, the likelihood's parameter
    under its ``compute_gradients`` name in the head's], J [N], dX, py_mean, py_var [S, N, D], density)."""
    import torch
    out = torch_forward(spec, X, Y, zs, lik, x_leaf=True)
    want, dlik = _gradients(out)
    if dlik is not None:
        want[-1][LIK_PARAM[lik[0]]] = dlik
    (dX,) = torch.autograd.grad(out["data"].sum(), out["X"])
    m, v = out["mean"].detach().numpy(), out["var"].detach().numpy()
    e, ev, ld = predictions(lik, m, v, Y)
    return dict(parts=(out["elbo"].item(), out["data"].sum().item(), out["kl"].item()), want=want, J=out["data"].detach().numpy(),
                dX=dX.numpy(), py_mean=e, py_var=ev, density=ld)
