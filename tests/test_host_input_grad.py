"""Host-side checks of the input-gradient feature: the autograd reference of tests/input_grad_ref.py against the float64 oracle (values and
central differences), ``adversarial_examples`` arithmetic on a stub model, and the argument validation that needs no device."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import input_grad_ref as R                                                    # noqa: E402
from deepcgp_amd.likelihoods import Bernoulli, Gaussian                        # noqa: E402
from deepcgp_amd.models import AdversarialAccuracyLogger, adversarial_examples   # noqa: E402

FAMILIES = ["conv_small", "three_ragged", "cifar3", "acos", "identity_mean", "dense_ard", "additive", "head_small"]


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-30)


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("white", [False, True])
def test_reference_forward_reproduces_the_oracle(name, white):
    """The helper's per-image density and E_log_p_Y against the oracle's predict_y / E_log_p_Y, 1e-9 relative (the model-level tolerance)."""
    spec, X, Y, zs = R.make_case(name, white=white, N=3, S=2)
    ref = R.oracle_for(spec, X, Y)
    for obj in ("density", "elbo"):
        with torch.no_grad():
            J = R.objective(spec, R._t(X), Y, zs, objective=obj).numpy()
        assert rel(J, R.oracle_objective(ref, spec, X, Y, zs, objective=obj)) <= 1e-9, (name, white, obj)


@pytest.mark.parametrize("like", ["gaussian", "bernoulli"])
def test_reference_forward_reproduces_the_oracle_float_targets(like):
    spec, X, Ylab, zs = R.make_case("conv_small", N=3, S=2, head_outputs=3)
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((3, 3)) if like == "gaussian" else (rng.random((3, 3)) > 0.5).astype(np.float64)
    kw = dict(objective="elbo", likelihood=like, s2=0.7 if like == "gaussian" else None)
    with torch.no_grad():
        J = R.objective(spec, R._t(X), Y, zs, **kw).numpy()
    assert rel(J, R.oracle_objective(R.oracle_for(spec, X, Ylab), spec, X, Y, zs, **kw)) <= 1e-9


H_STEP, FD_BOUND = 1e-4, 5e-8


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("objective", ["density", "elbo"])
def test_autograd_agrees_with_central_differences_of_the_oracle(name, objective):
    """Directional derivatives g . d of the helper's autograd dX against (J(X + h d) - J(X - h d)) / 2h of the ORACLE's objective, four random
    directions with max |d| = 1, both whitenings.
    Step: h = 1e-4, chosen by a scan over {1e-3, 1e-4, 1e-5} on these very cases: the disagreement relative to max(1, |g . d|) falls as h^2
    from 1e-3 (up to 1.7e-6) to 1e-4 (up to 1.8e-8, dense_ard unwhitened; 4e-9 and below elsewhere) and stops falling at 1e-5 (up to 5.7e-9:
    rounding of the objective, ~1e-15 |J| / h), so 1e-4 sits at the bottom of the curve with truncation and rounding both below 2e-8.
    Asserted: 5e-8, under three times the largest disagreement observed at h = 1e-4 (1.8e-8)."""
    rng = np.random.default_rng(0)
    for white in (False, True):
        spec, X, Y, zs = R.make_case(name, white=white, N=3, S=2)
        ref = R.oracle_for(spec, X, Y)
        _, g = R.autograd_input_gradient(spec, X, Y, zs, objective=objective)
        worst = 0.0
        for _ in range(4):
            d = rng.standard_normal(X.shape)
            d /= np.abs(d).max()
            fd = (R.oracle_objective(ref, spec, X + H_STEP * d, Y, zs, objective=objective)
                  - R.oracle_objective(ref, spec, X - H_STEP * d, Y, zs, objective=objective)) / (2 * H_STEP)
            an = (g * d).sum(1)
            worst = max(worst, np.abs(fd - an).max() / max(1.0, np.abs(an).max()))
        print("%s %s white=%d: central differences vs autograd %.2e" % (name, objective, white, worst))
        assert worst <= FD_BOUND, (name, objective, white, worst)


class _Stub:
    """input_gradient with a known gradient: J = sum(c * x), dJ/dx = c."""

    def __init__(self, c):
        self.c, self.calls = np.asarray(c, np.float64), []

    def input_gradient(self, X, Y, S=None, objective="density", zs=None, seed=0):
        self.calls.append((np.array(X), S, objective, seed))
        return (X * self.c).sum(1), np.broadcast_to(self.c, X.shape).copy()


def test_adversarial_examples_arithmetic():
    c = np.array([[2.0, -3.0, 0.0, 0.5]])
    X = np.array([[0.1, 0.2, 0.3, 0.95], [0.0, 1.0, 0.5, 0.5]])
    m = _Stub(c)
    adv = adversarial_examples(m, X, [0, 1], 0.1, S=4, seed=9, objective="elbo")            # FGSM: x - eps sign(g)
    assert np.allclose(adv, X - 0.1 * np.sign(c), rtol=0, atol=1e-16) and len(m.calls) == 1
    assert m.calls[0][1:] == (4, "elbo", 9)
    assert np.array_equal(adv[:, 2], X[:, 2])                                               # zero gradient: the pixel stays
    adv = adversarial_examples(m, X, [0, 1], 0.1, clip=(0.0, 1.0))
    assert adv.min() >= 0.0 and adv.max() <= 1.0 and np.isclose(adv[1, 0], 0.0) and np.isclose(adv[1, 1], 1.0)
    m = _Stub(c)
    it = adversarial_examples(m, X, [0, 1], 0.1, steps=4)                                   # default step eps / steps: ends on the ball's surface
    assert len(m.calls) == 4 and np.allclose(it, X - 0.1 * np.sign(c), atol=1e-15)
    assert np.allclose(m.calls[1][0], X - 0.025 * np.sign(c), atol=1e-15)                   # step 2 starts from step 1's images
    it = adversarial_examples(_Stub(c), X, [0, 1], 0.1, steps=5, step_size=0.07)            # projection onto the ball
    assert np.abs(it - X).max() <= 0.1 + 1e-15 and np.allclose(it, X - 0.1 * np.sign(c), atol=1e-15)
    img = X.reshape(2, 2, 2, 1)
    assert adversarial_examples(_Stub(c), img, [0, 1], 0.1).shape == img.shape
    for bad in (dict(epsilon=-1.0), dict(epsilon=0.1, steps=0), dict(epsilon=0.1, clip=(1.0, 0.0)), dict(epsilon=0.1, step_size=-0.1)):
        with pytest.raises(ValueError):
            adversarial_examples(_Stub(c), X, [0, 1], **bad)


def _bare_model(X, likelihood=None, K=10):
    """A DGP_Base with only what the host-side checks read: building its layers needs the device."""
    from types import SimpleNamespace
    from deepcgp_amd.dgp import DGP_Base
    m = object.__new__(DGP_Base)
    m.X, m.num_samples, m.dedup_layer0 = X, 2, False
    m.gaussian, m.bernoulli = isinstance(likelihood, Gaussian), isinstance(likelihood, Bernoulli)
    m.float_targets = m.gaussian or m.bernoulli
    m.layers = [SimpleNamespace(num_outputs=K)]
    m._model = m._ctx = None
    return m


def test_argument_validation_without_a_device():
    spec, X, Y, zs = R.make_case("conv_small", N=3, S=2)
    model = _bare_model(X)
    with pytest.raises(ValueError):
        model.input_gradient(X, Y, objective="logit")
    with pytest.raises(ValueError):
        model.input_gradient(X, Y, S=0)
    J, g = model.input_gradient(X[:0], Y[:0])                                               # N = 0: empty arrays, no device call
    assert J.shape == (0,) and g.shape == (0, X.shape[1])
    bad = Y.copy()
    bad[0] = -1
    with pytest.raises(ValueError):
        model.input_gradient(X, bad)
    bad[0] = 10
    with pytest.raises(ValueError):
        model.input_gradient(X, bad)
    with pytest.raises(ValueError):
        model.input_gradient(X[:, :-1], Y)
    with pytest.raises(ValueError):
        model.input_gradient(X, Y[:2])
    for like in (Gaussian(0.5), Bernoulli()):
        m = _bare_model(X, like, K=3)
        with pytest.raises(NotImplementedError):
            m.input_gradient(X, np.zeros((3, 3)), objective="density")
        with pytest.raises(ValueError):
            m.saliency(X)
    assert AdversarialAccuracyLogger.title == "adversarial_accuracy"
    lg = AdversarialAccuracyLogger(X, Y, 0.05, steps=2)
    assert (lg.epsilon, lg.steps, lg.batch_size, lg.num_samples) == (0.05, 2, 32, 5)
