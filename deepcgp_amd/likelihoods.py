"""Likelihoods of the model path: MultiClass with the RobustMax inverse link -- the gpflow.likelihoods.MultiClass(10) the
reference builds at /root/reference/conv_gp/models.py:67 (20 Gauss-Hermite points, epsilon 1e-3) -- Gaussian, Bernoulli, Softmax, StudentT
and Poisson."""
import numpy as np

from . import device as dev


class MultiClass:
    def __init__(self, num_classes=10, epsilon=1e-3):
        self.num_classes = int(num_classes)
        self.epsilon = float(epsilon)

    def variational_expectations(self, Fmu, Fvar, Y):
        ctx = dev.get_context()
        Fmu = np.ascontiguousarray(Fmu, np.float64)
        n, K = Fmu.shape
        if K != self.num_classes:
            raise ValueError("expected %d latent functions, got %d" % (self.num_classes, K))
        Y = np.ascontiguousarray(np.reshape(Y, -1), np.int32)
        if Y.shape[0] != n or Y.min(initial=0) < 0 or Y.max(initial=0) >= K:
            raise ValueError("labels must be %d integers in [0, %d)" % (n, K))
        if n == 0:
            return np.zeros((0,))
        dmu, dvar, dy = ctx.to_device(Fmu), ctx.to_device(Fvar), ctx.to_device(Y, np.int32)
        out = ctx.empty((n,))
        ctx._check(dev.lib().dcgp_robustmax_varexp(ctx.handle, dmu.ptr, dvar.ptr, dy.ptr, n, K, self.epsilon, out.ptr))
        return out.numpy()

    def predict_mean_and_var(self, Fmu, Fvar):
        ctx = dev.get_context()
        Fmu = np.ascontiguousarray(Fmu, np.float64)
        n, K = Fmu.shape
        if n == 0:
            return np.zeros((0, K)), np.zeros((0, K))
        dmu, dvar = ctx.to_device(Fmu), ctx.to_device(Fvar)
        out = ctx.empty((n, K))
        ctx._check(dev.lib().dcgp_robustmax_predict(ctx.handle, dmu.ptr, dvar.ptr, n, K, self.epsilon, out.ptr))
        ps = out.numpy()
        return ps, ps - np.square(ps)

    @staticmethod
    def predictive_uncertainty(ps):
        """The closed forms of ``DGP_Base.evaluate_uncertainty`` on host arrays: ``ps`` S x N x K class probabilities per sample
        (``predict_y``'s mean).  Returns {"p_mean" N x K, "predictive_entropy", "expected_entropy", "mutual_information", "confidence",
        "prediction"}, each N, in nats: H(pbar), 1/S sum_s H(p_s), their raw difference, max_k pbar and its first index."""
        ps = np.asarray(ps, np.float64)
        pbar = ps.sum(0) / ps.shape[0]
        h = -(pbar * np.log(pbar)).sum(-1)
        e = -(ps * np.log(ps)).sum(-1).sum(0) / ps.shape[0]
        return {"p_mean": pbar, "predictive_entropy": h, "expected_entropy": e, "mutual_information": h - e,
                "confidence": pbar.max(-1), "prediction": pbar.argmax(-1).astype(np.int32)}


class Gaussian:
    """gpflow 1.x likelihoods.Gaussian(variance) as DS-DGP's BroadcastingLikelihood applies it: one variance shared by every output,
    kept positive by transforms.positive (softplus + 1e-6) when trained.  Targets are float64 N x D.  On the model path
    (DGP_Base with this likelihood) every tail runs on the device (csrc/pointwise.hip); these methods are the closed forms of the
    same quantities on host arrays."""

    def __init__(self, variance=1.0):
        self.variance = float(variance)
        if not self.variance > 1e-6:
            raise ValueError("the Gaussian variance must be > 1e-6, got %r" % (variance,))

    def logp(self, F, Y):
        F, Y = np.asarray(F, np.float64), np.asarray(Y, np.float64)
        return -0.5 * np.log(2 * np.pi * self.variance) - 0.5 * np.square(Y - F) / self.variance

    def variational_expectations(self, Fmu, Fvar, Y):
        Fmu, Fvar, Y = (np.asarray(a, np.float64) for a in (Fmu, Fvar, Y))
        return -0.5 * np.log(2 * np.pi * self.variance) - 0.5 * (np.square(Y - Fmu) + Fvar) / self.variance

    def predict_mean_and_var(self, Fmu, Fvar):
        Fmu, Fvar = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
        return Fmu.copy(), Fvar + self.variance

    def predict_density(self, Fmu, Fvar, Y):
        Fmu, Fvar, Y = (np.asarray(a, np.float64) for a in (Fmu, Fvar, Y))
        v = Fvar + self.variance
        return -0.5 * np.log(2 * np.pi * v) - 0.5 * np.square(Y - Fmu) / v


def _probit(x):
    """gpflow 1.x likelihoods.probit: Phi(x) jittered into [1e-3, 1 - 1e-3], so that every log is finite."""
    from math import erf
    x = np.asarray(x, np.float64)
    return 0.5 * (1.0 + np.vectorize(erf, otypes=[np.float64])(x / np.sqrt(2.0))) * (1 - 2e-3) + 1e-3


class Bernoulli:
    """gpflow 1.x likelihoods.Bernoulli(invlink=probit) as DS-DGP's BroadcastingLikelihood applies it: every output an independent
    binary label, float64 targets N x D with Y == 1 positive and anything else negative (gpflow's logdensities.bernoulli).  No
    trainable parameters.  On the model path (DGP_Base with this likelihood) every tail runs on the device (csrc/pointwise.hip);
    these methods are the same quantities on host arrays, the variational expectations by gpflow's 20-point Gauss-Hermite rule."""
    num_gauss_hermite_points = 20

    def __init__(self, invlink="probit"):
        if invlink != "probit":
            raise ValueError("Bernoulli: only the probit link is supported, got %r" % (invlink,))
        self.invlink = invlink

    def conditional_mean(self, F):
        return _probit(F)

    def conditional_variance(self, F):
        p = _probit(F)
        return p - np.square(p)

    def logp(self, F, Y):
        p, Y = _probit(F), np.asarray(Y, np.float64)
        return np.where(Y == 1, np.log(p), np.log(1 - p))

    def variational_expectations(self, Fmu, Fvar, Y):
        """sum_i w_i / sqrt(pi) logp(Fmu + sqrt(2 Fvar) x_i, Y) (gpflow's ndiagquad)."""
        Fmu, Fvar, Y = (np.asarray(a, np.float64) for a in (Fmu, Fvar, Y))
        x, w = np.polynomial.hermite.hermgauss(self.num_gauss_hermite_points)
        F = Fmu[..., None] + np.sqrt(np.maximum(2 * Fvar, 1e-10))[..., None] * x
        return (self.logp(F, Y[..., None]) * (w / np.sqrt(np.pi))).sum(-1)

    def predict_mean_and_var(self, Fmu, Fvar):
        Fmu, Fvar = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
        p = _probit(Fmu / np.sqrt(1 + Fvar))
        return p, p - np.square(p)

    def predict_density(self, Fmu, Fvar, Y):
        p = self.predict_mean_and_var(Fmu, Fvar)[0]
        Y = np.asarray(Y, np.float64)
        return np.where(Y == 1, np.log(p), np.log(1 - p))

    @staticmethod
    def predictive_uncertainty(ps):
        """The closed forms of ``DGP_Base.evaluate_uncertainty`` on host arrays: ``ps`` S x N x D per-sample p(y = 1) (``predict_y``'s
        mean).  Returns {"p_mean", "predictive_entropy", "expected_entropy", "mutual_information", "confidence", "prediction"}, each
        N x D, in nats, with the binary entropy h(q) = -q log q - (1 - q) log(1 - q): h(pbar), 1/S sum_s h(p_s), their raw difference,
        max(pbar, 1 - pbar) and pbar > 0.5."""
        ps = np.asarray(ps, np.float64)
        h2 = lambda q: -q * np.log(q) - (1 - q) * np.log(1 - q)      # noqa: E731
        pbar = ps.sum(0) / ps.shape[0]
        h, e = h2(pbar), h2(ps).sum(0) / ps.shape[0]
        return {"p_mean": pbar, "predictive_entropy": h, "expected_entropy": e, "mutual_information": h - e,
                "confidence": np.maximum(pbar, 1 - pbar), "prediction": (pbar > 0.5).astype(np.int32)}


class _Quadrature:
    """What StudentT and Poisson share: the 20-node Gauss-Hermite rule of gpflow's ndiagquad applied to a per-element log density.  With
    x_i, w_i the nodes and weights, c_i = w_i / sqrt(pi), s = sqrt(max(2 Fvar, 1e-10)) and f_i = Fmu + s x_i:
      variational expectation  sum_i c_i logp(f_i, Y),
      predictive mean E_y = sum_i c_i conditional_mean(f_i), variance sum_i c_i (conditional_variance(f_i) + conditional_mean(f_i)^2) - E_y^2,
      predictive density logsumexp_i (logp(f_i, Y) + log c_i).
    On the model path (DGP_Base with such a likelihood) every tail runs on the device (csrc/pointwise.hip);
    ``variational_expectations`` on arrays goes through the device too (dcgp_quad_varexp), the other methods are NumPy."""
    num_gauss_hermite_points = 20
    kind = None

    def _params(self):
        raise NotImplementedError

    def _nodes(self, Fmu, Fvar):
        Fmu, Fvar = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
        x, w = np.polynomial.hermite.hermgauss(self.num_gauss_hermite_points)
        return Fmu[..., None] + np.sqrt(np.maximum(2 * Fvar, 1e-10))[..., None] * x, w / np.sqrt(np.pi)

    def predict_mean_and_var(self, Fmu, Fvar):
        F, c = self._nodes(Fmu, Fvar)
        cm = self.conditional_mean(F)
        e = (cm * c).sum(-1)
        return e, ((self.conditional_variance(F) + np.square(cm)) * c).sum(-1) - np.square(e)

    def predict_density(self, Fmu, Fvar, Y):
        F, c = self._nodes(Fmu, Fvar)
        t = self.logp(F, np.asarray(Y, np.float64)[..., None]) + np.log(c)
        mx = t.max(-1)
        return mx + np.log(np.exp(t - mx[..., None]).sum(-1))

    def variational_expectations(self, Fmu, Fvar, Y):
        ctx = dev.get_context()
        Fmu, Fvar, Y = (np.ascontiguousarray(a, np.float64) for a in (Fmu, Fvar, Y))
        if Fmu.ndim != 2 or Fvar.shape != Fmu.shape or Y.shape != Fmu.shape:
            raise ValueError("Fmu, Fvar and Y must be N x D arrays of one shape, got %r, %r, %r" % (Fmu.shape, Fvar.shape, Y.shape))
        n, K = Fmu.shape
        if Fmu.size == 0:
            return np.zeros((n, K))
        par = np.ascontiguousarray(self._params(), np.float64)
        dmu, dvar, dy = ctx.to_device(Fmu), ctx.to_device(Fvar), ctx.to_device(Y)
        out = ctx.empty((n, K))
        ctx._check(dev.lib().dcgp_quad_varexp(ctx.handle, self.kind, par.ctypes.data, dmu.ptr, dvar.ptr, dy.ptr, n, K, out.ptr))
        return out.numpy()


def _lgamma(x):
    from math import lgamma
    return np.vectorize(lgamma, otypes=[np.float64])(np.asarray(x, np.float64))


class StudentT(_Quadrature):
    """gpflow 1.x likelihoods.StudentT(scale, deg_free) as DS-DGP's BroadcastingLikelihood applies it: robust regression, float64 targets
    N x D, logp(f, y) = c_nu - log scale - (nu + 1) / 2 log1p(((y - f) / scale)^2 / nu) with c_nu = lgamma((nu + 1) / 2) - lgamma(nu / 2) -
    log(nu pi) / 2.  ``scale`` is trainable, kept positive by transforms.positive (softplus + 1e-6); ``deg_free`` (> 2, so that the
    predictive variance exists) is fixed at construction, as in gpflow."""
    kind = 4

    def __init__(self, scale=1.0, deg_free=3.0):
        self.scale, self.deg_free = float(scale), float(deg_free)
        if not (self.scale > 1e-6 and np.isfinite(self.scale)):
            raise ValueError("the StudentT scale must be > 1e-6, got %r" % (scale,))
        if not (self.deg_free > 2.0 and np.isfinite(self.deg_free)):
            raise ValueError("the StudentT deg_free must be > 2, got %r" % (deg_free,))

    def _params(self):
        return [self.scale, self.deg_free]

    def logp(self, F, Y):
        from math import lgamma, log, pi
        F, Y = np.asarray(F, np.float64), np.asarray(Y, np.float64)
        nu = self.deg_free
        c = lgamma(0.5 * (nu + 1)) - lgamma(0.5 * nu) - 0.5 * log(nu * pi)
        return c - np.log(self.scale) - 0.5 * (nu + 1) * np.log1p(np.square((Y - F) / self.scale) / nu)

    def conditional_mean(self, F):
        return np.array(F, np.float64)

    def conditional_variance(self, F):
        return np.full(np.shape(F), self.scale ** 2 * self.deg_free / (self.deg_free - 2.0))


class Poisson(_Quadrature):
    """gpflow 1.x likelihoods.Poisson(invlink=exp, binsize) as DS-DGP's BroadcastingLikelihood applies it: count targets (non-negative
    integer values, float64 N x D), logp(f, y) = y (f + log b) - b e^f - lgamma(y + 1).  The variational expectation is gpflow's closed form
    for the exp link, y Fmu - b exp(Fmu + Fvar / 2) - lgamma(y + 1) + y log b.  No trainable parameters."""
    kind = 5

    def __init__(self, invlink="exp", binsize=1.0):
        if invlink != "exp":
            raise ValueError("Poisson: only the exp link is supported, got %r" % (invlink,))
        self.invlink, self.binsize = invlink, float(binsize)
        if not (self.binsize > 0 and np.isfinite(self.binsize)):
            raise ValueError("the Poisson binsize must be > 0, got %r" % (binsize,))

    def _params(self):
        return [self.binsize]

    def logp(self, F, Y):
        F, Y = np.asarray(F, np.float64), np.asarray(Y, np.float64)
        return Y * (F + np.log(self.binsize)) - self.binsize * np.exp(F) - _lgamma(Y + 1.0)

    def conditional_mean(self, F):
        return self.binsize * np.exp(np.asarray(F, np.float64))

    conditional_variance = conditional_mean


def softmax_nodes(num_classes, num_points, rng):
    """[Q, K] nodes of the Softmax rule: Q // 2 rows of standard-normal draws followed by their negations (antithetic pairs: the odd
    moments of the rule are exact), an odd Q with one more unpaired row at the end."""
    Q, K = int(num_points), int(num_classes)
    half = rng.standard_normal((Q // 2, K))
    rows = [half, -half]
    if Q % 2:
        rows.append(rng.standard_normal((1, K)))
    return np.ascontiguousarray(np.concatenate(rows, 0), np.float64)


class Softmax:
    """gpflow 1.x likelihoods.SoftMax(num_classes) -- p(y | f) = softmax(f)[y], a MonteCarloLikelihood -- with gpflow's fresh draw per call
    replaced by a FIXED table of nodes ``nodes`` [Q, K] of standard-normal draws, the same for every row (a Q-node rule, used the way the
    Gauss-Hermite nodes are used for RobustMax and Bernoulli): with s = sqrt(max(Fvar, 1e-10)) and f_q = Fmu + s * nodes[q],
      variational expectation  1/Q sum_q (f_q[y] - logsumexp f_q),   predictive mean  p = 1/Q sum_q softmax(f_q), variance p - p^2,
      predictive density log p[y].
    The objective is deterministic (same bits on two calls, whatever the rank count); ``resample()`` between steps gives gpflow's fresh
    noise.  Labels are integers in [0, num_classes).  No trainable parameters; the table is not saved in checkpoints.  On the model path
    (DGP_Base with this likelihood) every tail runs on the device (csrc/softmax.hip); ``variational_expectations`` on arrays goes through
    the device too (dcgp_softmax_varexp), the other methods are NumPy on the same table."""

    def __init__(self, num_classes=10, num_monte_carlo_points=100, seed=0, nodes=None):
        self.num_classes = int(num_classes)
        if self.num_classes < 2:
            raise ValueError("Softmax needs num_classes >= 2, got %r" % (num_classes,))
        self._models = []
        if nodes is not None:
            nodes = np.ascontiguousarray(nodes, np.float64)
            if nodes.ndim != 2 or nodes.shape[1] != self.num_classes or nodes.shape[0] < 1:
                raise ValueError("nodes must be Q x %d with Q >= 1, got shape %r" % (self.num_classes, nodes.shape))
            self.nodes = nodes
        else:
            if int(num_monte_carlo_points) < 1:
                raise ValueError("num_monte_carlo_points must be >= 1, got %r" % (num_monte_carlo_points,))
            self.nodes = softmax_nodes(self.num_classes, num_monte_carlo_points, np.random.RandomState(seed))
        if self.nodes.size > 4096:
            raise ValueError("Softmax: Q * K = %d * %d > 4096 (the device tails keep the table in 32 KB of LDS)" % self.nodes.shape)

    @property
    def num_monte_carlo_points(self):
        return self.nodes.shape[0]

    def _attach(self, model):
        import weakref
        self._models = [r for r in self._models if r() is not None and r() is not model] + [weakref.ref(model)]

    def resample(self, rng=None):
        """Redraw the table (same Q, antithetic pairs again) from ``rng`` -- a RandomState, a seed, or None for a fresh RandomState -- and
        push it to every built model this likelihood is attached to."""
        if not isinstance(rng, np.random.RandomState):
            rng = np.random.RandomState(rng)
        self.nodes = softmax_nodes(self.num_classes, self.nodes.shape[0], rng)
        for r in self._models:
            m = r()
            if m is not None:
                m.push_likelihood_nodes()
        return self.nodes

    # ---- host closed forms on the table ------------------------------------------------------------
    @staticmethod
    def _log_softmax(F):
        F = np.asarray(F, np.float64)
        mx = F.max(-1, keepdims=True)
        return F - (mx + np.log(np.exp(F - mx).sum(-1, keepdims=True)))

    def _labels(self, Y, shape):
        Y = np.asarray(Y)
        if Y.ndim == len(shape) + 1 and Y.shape[-1] == 1:
            Y = Y[..., 0]
        Y = np.broadcast_to(Y, shape).astype(np.int64)
        if Y.size and (Y.min() < 0 or Y.max() >= self.num_classes):
            raise ValueError("labels must be integers in [0, %d)" % self.num_classes)
        return Y

    def _F(self, Fmu, Fvar):
        """[..., Q, K]: f_q = Fmu + sqrt(max(Fvar, 1e-10)) * nodes[q]"""
        Fmu, Fvar = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
        if Fmu.shape[-1] != self.num_classes:
            raise ValueError("expected %d latent functions, got %d" % (self.num_classes, Fmu.shape[-1]))
        return Fmu[..., None, :] + np.sqrt(np.maximum(Fvar, 1e-10))[..., None, :] * self.nodes

    def logp(self, F, Y):
        """log softmax(F)[Y]: F [..., K], Y [...] integer labels."""
        ls = self._log_softmax(F)
        Y = self._labels(Y, ls.shape[:-1])
        return np.take_along_axis(ls, Y[..., None], -1)[..., 0]

    def conditional_mean(self, F):
        return np.exp(self._log_softmax(F))

    def conditional_variance(self, F):
        p = self.conditional_mean(F)
        return p - np.square(p)

    def predict_mean_and_var(self, Fmu, Fvar):
        p = np.exp(self._log_softmax(self._F(Fmu, Fvar))).sum(-2) / self.nodes.shape[0]
        return p, p - np.square(p)

    def predict_density(self, Fmu, Fvar, Y):
        p = self.predict_mean_and_var(Fmu, Fvar)[0]
        Y = self._labels(Y, p.shape[:-1])
        return np.log(np.take_along_axis(p, Y[..., None], -1)[..., 0])

    def variational_expectations(self, Fmu, Fvar, Y):
        ctx = dev.get_context()
        Fmu = np.ascontiguousarray(Fmu, np.float64)
        n, K = Fmu.shape
        if K != self.num_classes:
            raise ValueError("expected %d latent functions, got %d" % (self.num_classes, K))
        Y = np.ascontiguousarray(np.reshape(Y, -1), np.int32)
        if Y.shape[0] != n or Y.min(initial=0) < 0 or Y.max(initial=0) >= K:
            raise ValueError("labels must be %d integers in [0, %d)" % (n, K))
        if n == 0:
            return np.zeros((0,))
        dmu, dvar, dy, dn = ctx.to_device(Fmu), ctx.to_device(Fvar), ctx.to_device(Y, np.int32), ctx.to_device(self.nodes)
        out = ctx.empty((n,))
        ctx._check(dev.lib().dcgp_softmax_varexp(ctx.handle, dmu.ptr, dvar.ptr, dy.ptr, n, K, dn.ptr, self.nodes.shape[0], out.ptr))
        return out.numpy()

    predictive_uncertainty = staticmethod(MultiClass.predictive_uncertainty)
