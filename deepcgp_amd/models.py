"""Model assembly -- the counterpart of /root/reference/conv_gp/models.py (ModelBuilder) plus a builder
from the neutral model spec used by the benchmarks and parity tests (deepcgp_amd.synthetic)."""
import numpy as np

from . import kernels as _kernels
from .dgp import DGP_Base
from .kernels import JITTER, RBF, ArcCosine, Matern32, Matern52, ConvKernel, AdditivePatchKernel, PatchInducingFeatures, InducingPoints
from .layers import ConvLayer, SVGP_Layer, mixing_matrix
from .likelihoods import MultiClass, Softmax
from .mean_functions import Conv2dMean, IdentityConv2dMean  # noqa: F401  (the names conv_gp/models.py:11 imports)
from .mean_functions import MEAN_FILTERS, LinearConv2dMean, conv_mean_filter
from .views import FullView
from .arguments import parse_dilations, parse_inducing_init, parse_latent_gps, parse_paddings


def parse_ints(int_string):
    """conv_gp/models.py:14-18."""
    if int_string == '':
        return []
    return [int(i) for i in int_string.split(',')]


# --likelihood values (the ten-class likelihood ModelBuilder puts on the head)
LIKELIHOODS = {"robustmax": MultiClass, "softmax": Softmax}

# --base-kernel values (conv layers); "acos" takes gpflow's default parameters (a spec may carry its own three), the others (variance, lengthscales)
BASE_KERNELS = {"rbf": RBF, "acos": ArcCosine, "matern32": Matern32, "matern52": Matern52}


def build_layers_from_spec(spec):
    """Layers of a neutral model spec.  An entry's optional ``pad`` is the zero padding of its input; its ``H``, ``W`` stay unpadded.  A conv
    entry's optional ``dil`` is its dilation (taps that many pixels apart, stride 1).  A conv
    entry's optional ``mix_W`` [R, Rout] mixes its R GPs into Rout maps (``mix_trainable``, default True: whether the optimiser moves it); its
    mean function then has Rout maps and the next entry's ``C`` is Rout."""
    if spec["head"].get("kernel", "conv") == "rbf" and spec["head"].get("pad", 0):
        raise ValueError("--paddings: the dense head of --last-kernel rbf takes no padding (pad %d)" % spec["head"]["pad"])
    layers = []
    for c in spec["convs"]:
        view = FullView((c["H"], c["W"]), c["f"], c["C"], c["s"], padding=c.get("pad", 0), dilation=c.get("dil", 1))
        kind = c.get("base", "rbf")
        if kind not in BASE_KERNELS:
            raise ValueError("Not a valid base-kernel value")
        if kind == "acos":      # optional key acos = (variance, weight_variances, bias_variance); absent: gpflow's defaults
            av, aw, ab = c.get("acos", (1.0, 1.0, 1.0))
            base = ArcCosine(view.patch_length, order=0, variance=av, weight_variances=aw, bias_variance=ab)
        elif kind == "rbf" and np.ndim(c["ls"]) > 0:      # ls [L]: one lengthscale per patch element (--ard)
            base = RBF(view.patch_length, c["variance"], c["ls"], ARD=True)
        else:
            base = BASE_KERNELS[kind](view.patch_length, c["variance"], c["ls"])
        mix_W = None if c.get("mix_W") is None else np.array(c["mix_W"], np.float64)
        if mix_W is not None and (mix_W.ndim != 2 or mix_W.shape[0] != c["R"]):
            raise ValueError("a conv entry's mix_W must be [R, Rout] = [%d, Rout], got shape %r" % (c["R"], mix_W.shape))
        Rout = c["R"] if mix_W is None else int(mix_W.shape[1])      # maps leaving the layer
        mf = c.get("mean_function")
        if mf == "conv2d":      # --identity-mean: Conv2dMean(filter_size, NHWC[3], feature_map, stride=stride), conv_gp/models.py:95-97
            mf = Conv2dMean(c["f"], c["C"], Rout, stride=c["s"])
            mf.set_trainable(False)                                                            # models.py:100
        if c.get("mean_filter") is not None:      # a linear convolutional mean on the device: its filter [f, f, C, R] (or [f f C, R]) and whether it is trained
            if mf is not None:
                raise ValueError("a conv entry takes mean_function or mean_filter, not both")
            W = np.array(c["mean_filter"], np.float64).reshape(c["f"], c["f"], c["C"], Rout)
            mf = LinearConv2dMean(c["f"], c["C"], Rout, stride=c["s"], filter=W, trainable=bool(c.get("mean_trainable", False)))
        if mix_W is None:
            layer = ConvLayer(base, mf,
                              feature=PatchInducingFeatures(c["Z"]), view=view, white=c["white"], gp_count=c["R"],
                              q_mu=c["q_mu"], q_sqrt=c["q_sqrt"])
        else:
            layer = ConvLayer(base, mf,
                              feature=PatchInducingFeatures(c["Z"]), view=view, white=c["white"], gp_count=c["R"],
                              q_mu=c["q_mu"], q_sqrt=c["q_sqrt"], mixing=mix_W)
            layer.mixing_trainable = bool(c.get("mix_trainable", True))
        layer.Z_prior = np.array(c.get("Z0", c["Z"]), np.float64)
        layer._build_prior_cholesky()
        layers.append(layer)
    h = spec["head"]
    view = FullView((h["H"], h["W"], h["C"]), h["f"], h["C"], h["s"], padding=h.get("pad", 0))
    if h.get("kernel", "conv") == "rbf":   # dense RBF-ARD head (--last-kernel rbf)
        layers.append(SVGP_Layer(kern=RBF(h["Z"].shape[1], h["variance"], h["ls_ard"], ARD=True), num_outputs=h["R"],
                                 feature=InducingPoints(h["Z"]), mean_function=None, white=h["white"], q_mu=h["q_mu"],
                                 q_sqrt=h["q_sqrt"]))
        return layers
    cls = AdditivePatchKernel if h.get("kernel", "conv") == "add" else ConvKernel
    kern = cls(RBF(view.patch_length, h["variance"], h["ls"]), view, patch_weights=h.get("w"))
    layers.append(SVGP_Layer(kern=kern, num_outputs=h["R"], feature=PatchInducingFeatures(h["Z"]),
                             mean_function=None, white=h["white"], q_mu=h["q_mu"], q_sqrt=h["q_sqrt"]))
    return layers


def build_from_spec(spec, X, Y, likelihood=None):
    """DGP_Base on the HIP path from a model spec (see deepcgp_amd.synthetic); ``likelihood`` None = MultiClass(10)."""
    return DGP_Base(X, Y, likelihood=MultiClass(10) if likelihood is None else likelihood, layers=build_layers_from_spec(spec),
                    num_samples=spec["S"], minibatch_size=None, num_data=spec["num_data"], name='DGP')


def save_model_parameters(model, path, global_step=0):
    """Write the reference's checkpoint: ``np.save(path, {param.pathname: value, 'global_step': int})``
    (Experiment._save_model_parameters, conv_gp/experiment.py:56-64) -- readable by ``--load-model`` on either side
    (ModelBuilder._load_layer_parameters, conv_gp/models.py:200-240)."""
    params = {p.pathname: np.array(p.value) for p in model.parameters}
    params['global_step'] = int(global_step)
    np.save(path, params)
    return params


OPTIMIZER_STATE_FORMAT = 1


def save_optimizer_state(model, path, global_step, rng=None):
    """Write the sidecar of a checkpoint (``--keep-optimizer``): an ``.npz`` with ``format``, ``global_step``, the arrays of
    ``model.optimizer_state()`` under ``opt/<key>``, and -- with ``rng``, a ``numpy.random.Generator`` -- its bit generator's state as a JSON
    string (``rng``).  It also holds what a later step depends on and the reference's checkpoint has no key for: every conv layer's prior
    inducing patches (``prior/<i>/Z``; the checkpoint's Z is the trained one, a model built from it alone takes that for its prior).
    Nothing in it is pickled.  Returns the dict that was written."""
    import json
    out = {"format": np.array(OPTIMIZER_STATE_FORMAT, np.int64), "global_step": np.array(int(global_step), np.int64)}
    for key, value in model.optimizer_state().items():
        out["opt/" + key] = np.asarray(value)
    for li, l in enumerate(getattr(model, "layers", [])[:-1]):
        out["prior/%d/Z" % li] = np.array(l.Z_prior, np.float64)
    if rng is not None:
        out["rng"] = np.array(json.dumps(rng.bit_generator.state))
    with open(path, "wb") as fh:      # (np.savez would append .npz to another suffix)
        np.savez(fh, **out)
    return out


def load_optimizer_state(path):
    """Read a sidecar ``save_optimizer_state`` wrote (``allow_pickle=False``): ``{"global_step": int, "state": the dict
    ``set_optimizer_state`` takes, "prior": {layer: Z}, "rng": the bit generator's state dict or None}``.  A missing file or another
    format raises ValueError naming the path."""
    import json
    import os
    if not os.path.exists(path):
        raise ValueError("optimizer state %s not found (written beside a checkpoint by --keep-optimizer)" % path)
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or int(z["format"]) != OPTIMIZER_STATE_FORMAT:
            raise ValueError("optimizer state %s: not format %d" % (path, OPTIMIZER_STATE_FORMAT))
        state = {k[len("opt/"):]: np.array(z[k]) for k in z.files if k.startswith("opt/")}
        prior = {int(k.split("/")[1]): np.array(z[k]) for k in z.files if k.startswith("prior/")}
        rng = json.loads(str(z["rng"][()])) if "rng" in z.files else None
        step = int(z["global_step"])
    if "t" in state:
        state["t"] = int(state["t"])
    return {"global_step": step, "state": state, "prior": prior, "rng": rng}


def restore_optimizer_state(model, path, global_step, rng=None):
    """``load_optimizer_state(path)`` into ``model`` (and ``rng``'s bit generator): the prior inducing patches, the moments and the step count.
    A sidecar of another ``global_step`` than the checkpoint's raises ValueError naming the path."""
    side = load_optimizer_state(path)
    if side["global_step"] != int(global_step):
        raise ValueError("optimizer state %s is of global_step %d, the checkpoint of %d" % (path, side["global_step"], int(global_step)))
    for li, Z in side["prior"].items():
        layer = model.layers[li]
        if np.shape(Z) != np.shape(layer.Z_prior):
            raise ValueError("optimizer state %s: prior/%d/Z has shape %r, the layer's is %r" % (path, li, np.shape(Z), np.shape(layer.Z_prior)))
        layer.Z_prior = np.array(Z, np.float64)
        layer._build_prior_cholesky()
    model.sync_parameters()      # (the prior's patches travel with the parameters)
    model.set_optimizer_state(side["state"])
    if rng is not None and side["rng"] is not None:
        rng.bit_generator.state = side["rng"]
    return side


def learning_rate(lr, global_step, lr_decay_steps, decay_rate=0.1):
    """tf.train.exponential_decay(..., staircase=True) of conv_gp/experiment.py:71-73."""
    return float(lr) * decay_rate ** (int(global_step) // int(lr_decay_steps))


def natgrad_gamma(global_step, gamma0=0.001, steps_back=0, gamma_step=1e-3, back_step=0.2, gamma_max=1.0):
    """The NatGrad step-size schedule of conv_gp/experiment.py:74-81."""
    t = float(global_step) / 100.0
    return min((t * gamma_step + gamma0) * back_step ** steps_back, gamma_max)


def index_table(rng, n, batch, steps):
    """[steps, batch] int32: the minibatches of ``steps`` successive steps, one ``rng.choice(n, batch, replace=False)`` per step in step order
    -- the draws the per-step loop makes."""
    out = np.empty((int(steps), int(batch)), np.int32)
    for i in range(int(steps)):
        out[i] = rng.choice(n, size=batch, replace=False)
    return out


def lr_table(lr, global_step, steps, lr_decay_steps):
    """``learning_rate`` of steps global_step .. global_step + steps - 1."""
    return np.array([learning_rate(lr, global_step + i, lr_decay_steps) for i in range(int(steps))], np.float64)


def _train_adam(model, steps, lr, lr_decay_steps, global_step, seed, callback, rng, n, bs):
    """The Adam branch of ``train``: the whole span through ``DGP_Base.train_run`` on the model's own X / Y, attached for the call (a set the
    model already holds resident, ``attach_dataset()`` without arguments, is used as it is).  With a callback one step per run: it may
    inspect the model at that step."""
    if steps < 1:
        return []
    idx = index_table(rng, n, bs, steps)
    lrs = lr_table(lr, global_step, steps, lr_decay_steps)
    own = model._dataset is not None and model._dataset[1] and model._dataset[0] == n
    if not own:
        model.attach_dataset()
    try:
        if callback is None:
            return [float(e) for e in model.train_run(idx, lrs, seed=seed + global_step)]
        history = []
        for i in range(steps):
            elbo = float(model.train_run(idx[i:i + 1], lrs[i:i + 1], seed=seed + global_step + i)[0])
            history.append(elbo)
            callback(global_step + i + 1, elbo)
        return history
    finally:
        if not own:
            model.detach_dataset()


def train(model, steps, lr=0.01, lr_decay_steps=50000, global_step=0, seed=0, callback=None, optimizer="Adam", gamma=0.001,
          max_retries=5, dedup_layer0=True, augment=None):
    """The reference's optimisation loop (conv_gp/experiment.py:84-108 + gpflow.actions.Loop at :44).  Every step draws a
    minibatch and evaluates the ELBO and its gradient on the device (``compute_gradients``), then
      "Adam":    one device Adam step on every parameter; the whole span is ONE call (``train_run``: the training set resident on the
                 device, the minibatches gathered there), one call per step when a ``callback`` wants to see every step;
      "SGD":     one plain gradient step;
      "NatGrad": a natural-gradient step on every layer's (q_mu, q_sqrt) (``DGP_Base.natgrad_step``, step size from
                 ``natgrad_gamma``), then -- as the reference's loop does, with the variational parameters switched to
                 non-trainable -- a fresh gradient and an Adam step on everything else.
    ``dedup_layer0`` (default on): propagate() tiles the minibatch S times, so the first layer sees S identical copies;
    its conditional and reverse pass are evaluated on the distinct images only -- same ELBO, same gradients, about half the
    step time at the headline configuration.
    ``augment``: an ``augment.Augmentation`` for the span (None: whatever the model has set stays); it is set on the model
    (``set_augmentation``) and the model's earlier one restored afterwards.  The step of global index g augments batch position b with the draw
    of (seed + g, b) under every optimiser -- inside ``train_run`` for Adam, through ``model.augment(X[idx], seed + g)`` for the others -- so the
    same flags give the same batches.
    Returns the list of ELBO values; the Python-side parameter objects are refreshed at the end (``pull_parameters``)."""
    if optimizer not in ("Adam", "NatGrad", "SGD"):
        raise ValueError("Not a supported optimizer. Try Adam or NatGrad.")     # experiment.py:109-110
    rng = np.random.default_rng(seed)
    n = model.X.shape[0]
    bs = min(model.minibatch_size or n, n)
    history = []
    steps_back = 0
    model._build()
    if getattr(model._ctx, "nranks", 1) > 1:
        # every rank would draw the same minibatch and the all-reduced gradients would count it once per rank
        raise NotImplementedError("train() drives one GPU; shard the minibatch per rank and call compute_gradients / adam_step yourself")
    dedup_before, model.dedup_layer0 = model.dedup_layer0, bool(dedup_layer0)
    augment_before = getattr(model, "augmentation", None)
    if augment is not None:
        model.set_augmentation(augment)
    augmenting = bool(getattr(model, "augmentation", None))
    nl = len(model.layers)
    for li in range(nl):
        for which in ("q_mu", "q_sqrt"):
            model.set_trainable(li, which, optimizer != "NatGrad")
    if optimizer == "Adam":          # value, gradient and update of a whole span in one device call (dcgp_model_train_run_adam)
        history = _train_adam(model, int(steps), lr, lr_decay_steps, global_step, seed, callback, rng, n, bs)
    for i in range(0 if optimizer == "Adam" else int(steps)):
        idx = rng.choice(n, size=bs, replace=False)
        step = global_step + i
        Xb = model.augment(model.X[idx], seed + step) if augmenting else model.X[idx]
        elbo, _ = model.compute_gradients(Xb, model.Y[idx], seed=seed + step, fetch=False)
        if optimizer == "NatGrad":
            # a step that leaves the positive-definite cone is retried with gamma scaled by 0.2, at most max_retries
            # times over the run -- the InvalidArgumentError / step_back_gamma handling of experiment.py:36-49
            while True:
                try:
                    model.natgrad_step(natgrad_gamma(step, gamma, steps_back))
                    break
                except np.linalg.LinAlgError:
                    steps_back += 1
                    if steps_back > max_retries:
                        raise
            model.compute_gradients(Xb, model.Y[idx], seed=seed + step, fetch=False)
        if optimizer == "SGD":
            model.sgd_step(learning_rate(lr, step, lr_decay_steps))
        else:
            model.adam_step(learning_rate(lr, step, lr_decay_steps))   # bias correction: the model's own step count
        history.append(elbo)
        if callback is not None:
            callback(step + 1, elbo)
    model.dedup_layer0 = dedup_before
    if augment is not None:
        model.set_augmentation(augment_before)
    model.pull_parameters()
    return history


class AccuracyLogger(object):
    """Test accuracy the way the reference's training log computes it (conv_gp/utils/log.py:50-67): batches of 32,
    five samples per image, arg-max of the sample-mean class probabilities.  Each batch is one device call
    (``predict_proba``); only N x num_classes probabilities cross the bus."""
    title = 'test_accuracy'

    def __init__(self, X_test, Y_test, batch_size=32, num_samples=5):
        self.X_test, self.Y_test = X_test, np.reshape(Y_test, (-1,))
        self.batch_size, self.num_samples = int(batch_size), int(num_samples)

    def __call__(self, model, seed=0):
        if getattr(model, "gaussian", False):
            raise ValueError("AccuracyLogger: accuracy needs a classification likelihood, this model is Gaussian")
        if getattr(model, "student_t", False) or getattr(model, "poisson", False):
            raise ValueError("AccuracyLogger: accuracy needs a classification likelihood, this model is %s" % model._lik_name())
        if getattr(model, "bernoulli", False):
            return self._binary(model, seed)
        correct = 0
        for i, lo in enumerate(range(0, len(self.Y_test), self.batch_size)):
            sl = slice(lo, lo + self.batch_size)
            p = model.predict_proba(self.X_test[sl], self.num_samples, seed=seed + i)
            correct += int((p.argmax(axis=1) == self.Y_test[sl]).sum())
        return correct / max(self.Y_test.size, 1)

    def _binary(self, model, seed):
        """Bernoulli likelihood: every (image, output) entry is a binary label, correct when it is 1 exactly where the sample-mean
        p(y = 1) is > 0.5 -- ``DGP_Base.evaluate``'s accuracy, with the same batches and seeds."""
        Y = np.reshape(self.Y_test, (len(self.X_test), -1)) == 1
        correct = 0
        for i, lo in enumerate(range(0, len(Y), self.batch_size)):
            sl = slice(lo, lo + self.batch_size)
            p = model.predict_proba(self.X_test[sl], self.num_samples, seed=seed + i)
            correct += int(((p > 0.5) == Y[sl]).sum())
        return correct / max(Y.size, 1)


class TTAAccuracyLogger(object):
    """Test accuracy under test-time augmentation: ``DGP_Base.evaluate(views=views)``'s accuracy -- the arg-max of the class probabilities
    averaged over the samples AND the views (``augment.views``) -- with AccuracyLogger's batching (32 images, five samples, batch i drawing from
    seed + i), the whole set in one device call.  The column keeps AccuracyLogger's title: the driver logs one or the other."""
    title = 'test_accuracy'

    def __init__(self, X_test, Y_test, views, batch_size=32, num_samples=5):
        self.X_test = X_test
        self.Y_test = Y_test if np.ndim(Y_test) == 2 and np.asarray(Y_test).dtype.kind == "f" else np.reshape(Y_test, (-1,))
        self.views = np.asarray(views)
        self.batch_size, self.num_samples = int(batch_size), int(num_samples)

    def __call__(self, model, seed=0):
        if getattr(model, "gaussian", False) or getattr(model, "student_t", False) or getattr(model, "poisson", False):
            raise ValueError("TTAAccuracyLogger: accuracy needs a classification likelihood, this model is %s" % model._lik_name())
        return model.evaluate(self.X_test, self.Y_test, S=self.num_samples, batch_size=self.batch_size, seed=seed, views=self.views)["accuracy"]


def adversarial_examples(model, X, Y, epsilon, steps=1, step_size=None, clip=None, objective="density", S=None, seed=0, zs=None):
    """Adversarial images in the L-infinity ball of radius ``epsilon`` around X, same shape as X.  ``steps=1`` is the fast gradient sign
    method, X - epsilon sign(dJ/dX): it lowers the objective (the log density of the true label) to first order; ``steps > 1`` is its
    iterated form with steps of ``step_size`` (default epsilon / steps), each followed by the projection onto the ball and onto
    ``clip=(lo, hi)`` if given.  A host loop over ``model.input_gradient`` with the same noise (``seed`` / ``zs``) at every step."""
    epsilon, steps = float(epsilon), int(steps)
    if not epsilon >= 0.0:
        raise ValueError("epsilon must be >= 0, got %r" % (epsilon,))
    if steps < 1:
        raise ValueError("steps must be >= 1, got %r" % (steps,))
    step = epsilon / steps if step_size is None else float(step_size)
    if not step >= 0.0:
        raise ValueError("step_size must be >= 0, got %r" % (step_size,))
    if clip is not None:
        lo, hi = float(clip[0]), float(clip[1])
        if not lo <= hi:
            raise ValueError("clip must be (lo, hi) with lo <= hi, got %r" % (clip,))
    X0 = np.asarray(X, np.float64)
    flat = X0.reshape(X0.shape[0], -1)
    adv = flat.copy()
    for _ in range(steps):
        _, g = model.input_gradient(adv, Y, S=S, objective=objective, zs=zs, seed=seed)
        adv = adv - step * np.sign(g)
        adv = np.minimum(np.maximum(adv, flat - epsilon), flat + epsilon)
        if clip is not None:
            adv = np.clip(adv, lo, hi)
    return adv.reshape(X0.shape)


class AdversarialAccuracyLogger(object):
    """Test accuracy on adversarial images, with AccuracyLogger's batching (32 images, five samples, batch i drawing from seed + i):
    each batch is attacked with ``adversarial_examples`` (FGSM for ``steps=1``) under the noise it is then classified with."""
    title = 'adversarial_accuracy'

    def __init__(self, X_test, Y_test, epsilon, steps=1, step_size=None, clip=None, objective="density", batch_size=32, num_samples=5):
        self.X_test, self.Y_test = X_test, np.reshape(Y_test, (-1,))
        self.epsilon, self.steps, self.step_size, self.clip, self.objective = float(epsilon), int(steps), step_size, clip, objective
        self.batch_size, self.num_samples = int(batch_size), int(num_samples)

    def __call__(self, model, seed=0):
        if getattr(model, "float_targets", False):
            raise ValueError("AdversarialAccuracyLogger: needs a multi-class (RobustMax or Softmax) model")
        correct = 0
        for i, lo in enumerate(range(0, len(self.Y_test), self.batch_size)):
            sl = slice(lo, lo + self.batch_size)
            adv = adversarial_examples(model, self.X_test[sl], self.Y_test[sl], self.epsilon, steps=self.steps, step_size=self.step_size,
                                       clip=self.clip, objective=self.objective, S=self.num_samples, seed=seed + i)
            p = model.predict_proba(adv, self.num_samples, seed=seed + i)
            correct += int((p.argmax(axis=1) == self.Y_test[sl]).sum())
        return correct / max(self.Y_test.size, 1)


class UncertaintyLogger(object):
    """Calibration and uncertainty of the test predictions with AccuracyLogger's batching (32 images, five samples, batch i drawing
    from seed + i): the dataset dict of ``DGP_Base.evaluate_uncertainty`` -- accuracy, mean log density, ECE, MCE, Brier score, mean
    predictive entropy, mean mutual information and the reliability table -- the whole set in one device call.  ``views``: test-time
    augmentation (``augment.views``; None: the images as they are)."""
    title = 'test_uncertainty'

    def __init__(self, X_test, Y_test, S=5, bins=15, batch_size=32, views=None):
        self.views = views
        self.X_test = X_test
        self.Y_test = Y_test if np.ndim(Y_test) == 2 and np.asarray(Y_test).dtype.kind == "f" else np.reshape(Y_test, (-1,))
        self.num_samples, self.bins, self.batch_size = int(S), int(bins), int(batch_size)

    def __call__(self, model, seed=0):
        kw = {} if self.views is None else {"views": self.views}      # (without views: the call it always made)
        return model.evaluate_uncertainty(self.X_test, self.Y_test, S=self.num_samples, batch_size=self.batch_size, seed=seed, bins=self.bins, **kw)


class TestLogDensityLogger(object):
    """Mean test log predictive density with AccuracyLogger's batching (32 images, five samples, batch i drawing from seed + i):
    ``DGP_Base.evaluate``, the whole set in one device call.  ``views``: test-time augmentation (``augment.views``; None: the images as they
    are) -- the log of the density averaged over samples and views."""
    title = 'test_log_likelihood'
    __test__ = False   # (not a pytest class despite the name)

    def __init__(self, X_test, Y_test, batch_size=32, num_samples=5, views=None):
        self.views = views
        # labels are flattened; float targets N x D (a Gaussian likelihood) are kept as they are
        self.X_test = X_test
        self.Y_test = Y_test if np.ndim(Y_test) == 2 and np.asarray(Y_test).dtype.kind == "f" else np.reshape(Y_test, (-1,))
        self.batch_size, self.num_samples = int(batch_size), int(num_samples)

    def __call__(self, model, seed=0):
        kw = {} if self.views is None else {"views": self.views}      # (without views: the call it always made)
        return model.evaluate(self.X_test, self.Y_test, S=self.num_samples, batch_size=self.batch_size, seed=seed, **kw)["mean_log_density"]


class GradNormLogger(object):
    """Mean pre-clip global gradient norm over the steps of the period that just ended (``--clip-norm``): ``norms()`` returns them, the driver
    collects them from ``DGP_Base.last_grad_norms`` after every optimiser call.  NaN for a period without a clipped step."""
    title = 'grad_norm'

    def __init__(self, norms):
        self.norms = norms

    def __call__(self, model, seed=0):
        norms = np.asarray(self.norms(), np.float64)
        return float(norms.mean()) if norms.size else float("nan")


class LogLikelihoodLogger(object):
    """The reference's ``train_log_likelihood`` column (conv_gp/utils/tensorboard.py:15-42): the ELBO of batches of 64 of the training
    set, ceil(min(5000, n) / 64) of them from row 0 on, summed and divided by batches * 64 (the reference's divisor, also for a short
    last batch).  Batch i draws its noise from seed + i; up to four batches are kept in flight (``enqueue_log_likelihood``)."""
    title = 'train_log_likelihood'
    batch_size = 64
    in_flight = 4      # dcgp_model::RING

    def __call__(self, model, seed=0):
        compute_on = min(5000, model.X.shape[0])
        batches = -(-compute_on // self.batch_size)
        total, tickets = 0.0, []
        for i in range(batches):
            sl = slice(i * self.batch_size, (i + 1) * self.batch_size)     # the reference's slices of model.X / model.Y
            if len(tickets) == self.in_flight:
                total += model.collect_log_likelihood(tickets.pop(0))
            tickets.append(model.enqueue_log_likelihood(model.X[sl], model.Y[sl], seed=seed + i))
        for t in tickets:
            total += model.collect_log_likelihood(t)
        return total / (batches * self.batch_size)


def zero_pad(NHWC_X, p):
    """[n, H, W, C] -> [n, H + 2p, W + 2p, C] with a zero border (the array itself when p == 0)."""
    return NHWC_X if not p else np.pad(NHWC_X, ((0, 0), (p, p), (p, p), (0, 0)))


def identity_conv(NHWC_X, filter_size, feature_maps_in, feature_maps_out, stride, count=1000, dilation=1):
    """Propagate random images through IdentityConv2dMean to initialise the next layer
    (conv_gp/models.py:29-33, conv_gp/mean_functions.py:6-26).  ``dilation`` d: the window spans d (f - 1) + 1 pixels, its centre tap sits
    at offset d * (f // 2)."""
    X = NHWC_X[np.random.choice(np.arange(NHWC_X.shape[0]), size=min(count, NHWC_X.shape[0]))]
    n, H, W, C = X.shape
    span = dilation * (filter_size - 1) + 1
    Ho, Wo = (H - span) // stride + 1, (W - span) // stride + 1
    c0 = dilation * (filter_size // 2)
    centre = X[:, c0:c0 + (Ho - 1) * stride + 1:stride, c0:c0 + (Wo - 1) * stride + 1:stride, :].sum(-1)
    return np.repeat(centre[..., None], feature_maps_out, axis=-1)


def filter_conv(NHWC_X, conv_filter, stride, count=1000, dilation=1):
    """``identity_conv`` for a layer with a ``LinearConv2dMean``: the same random-subset draw, propagated through ``conv_filter``
    [f, f, Cin, Cout] (VALID, NHWC) -- what the layer emits at initialisation, where q_mu is zero.  Host NumPy, one product per filter tap."""
    X = NHWC_X[np.random.choice(np.arange(NHWC_X.shape[0]), size=min(count, NHWC_X.shape[0]))]
    W = np.asarray(conv_filter, np.float64)
    f, _, Cin, Cout = W.shape
    n, H, Wd, C = X.shape
    d = int(dilation)                                   # taps d pixels apart
    Ho, Wo = (H - d * (f - 1) - 1) // stride + 1, (Wd - d * (f - 1) - 1) // stride + 1
    out = np.zeros((n, Ho, Wo, Cout))
    for kh in range(f):
        for kw in range(f):
            if np.any(W[kh, kw]):
                out += X[:, d * kh:d * kh + (Ho - 1) * stride + 1:stride, d * kw:d * kw + (Wo - 1) * stride + 1:stride, :] @ W[kh, kw]
    return out


# ---------------------------------------------------------------------------------------------------
# flags -> architecture -> neutral model spec -> layers  (the job of conv_gp/models.py:35-247)
# ---------------------------------------------------------------------------------------------------
# Checkpoint keys are gpflow path names, "DGP/layers/<i>/<suffix>" (conv_gp/experiment.py:56-64, notebooks/Inspect.ipynb cell 6).
# suffix -> field of the per-layer record the spec is filled from; the first matching row wins.
CHECKPOINT_FIELDS = (
    ("feature/Z", "Z"),
    ("q_mu", "q_mu"),
    ("q_sqrt", "q_sqrt"),
    ("base_kernel/variance", "variance"),          # conv_kernel/base_kernel/... (conv layers), kern/base_kernel/... (patch heads)
    ("base_kernel/lengthscales", "ls"),
    ("kern/patch_weights", "w"),
    ("mean_function/conv_filter", "mean_filter"),
    ("mixing/W", "mix_W"),                         # a mixed conv layer's W [G, R] (--latent-gps)  # a conv layer's LinearConv2dMean (--mean-filter / --train-mean)
    ("kern/variance", "variance"),                 # dense RBF head (--last-kernel rbf): the kernel sits directly under kern/
    ("kern/lengthscales", "ls"),
)


def read_checkpoint(path, n_layers):
    """``{'global_step': int, layer index: {field: array}}`` from a ``np.save``d ``{pathname: value}`` dict.  A checkpoint with
    fewer layers than the model being built keeps its conv layers in place and hands its LAST stored layer (the head it was
    trained with) to the model's last layer (conv_gp/models.py:231-238)."""
    raw = np.load(path, allow_pickle=True).item()
    records = {}
    for key, value in raw.items():
        parts = key.split("/")
        if len(parts) < 4 or parts[1] != "layers" or not parts[2].isdigit():
            continue
        suffix = "/".join(parts[3:])
        field = next((f for tail, f in CHECKPOINT_FIELDS if suffix.endswith(tail)), None)
        if field is not None:
            records.setdefault(int(parts[2]), {})[field] = np.asarray(value)
    stored = max(records) + 1 if records else 0
    if stored > n_layers:
        raise AssertionError("Can't load model if it has more layers than the one being built")
    if records and stored != n_layers:
        records[n_layers - 1] = records.pop(stored - 1)
    return int(raw.get("global_step", 0)), records


def draw_patches(NHWC_X, count, f, rng=np.random, dilation=1):
    """``count`` f x f patches, each cut at a random position of a random image: [count, f*f*C] in the (kh, kw, c) element order of
    FullView -- the sample PatchInducingFeatures.from_images clusters (conv_gp/kernels.py:139-164), drawn in one gather.  ``dilation`` d:
    the patches are dilated windows, taps d pixels apart (the same draws over the positions such a window fits)."""
    n, H, W, C = NHWC_X.shape
    d = int(dilation)
    span = d * (f - 1) + 1
    img = rng.randint(0, n, size=count)
    top, left = rng.randint(0, H - span, size=count), rng.randint(0, W - span, size=count)    # upper bound exclusive, as the reference draws them
    dy, dx = d * np.arange(f)[None, :, None], d * np.arange(f)[None, None, :]
    return NHWC_X[img[:, None, None], top[:, None, None] + dy, left[:, None, None] + dx, :].reshape(count, f * f * C)


class ModelBuilder(object):
    """``ModelBuilder(flags, NHWC_X_train, Y_train, model_path).build() -> DGP_Base`` (the interface of conv_gp/models.py:35-70).
    The flags are turned into a stage list, the stage list -- walking the initialisation images through the identity convolution,
    clustering patches for the inducing inputs, filling in what a checkpoint holds -- into the neutral model spec of
    ``deepcgp_amd.synthetic``, and the spec into layers by ``build_layers_from_spec``."""

    def __init__(self, flags, NHWC_X_train, Y_train, model_path=None):
        self.flags = flags
        self.X_train = NHWC_X_train
        self.Y_train = Y_train
        self.model_path = model_path
        self.global_step = None

    # ---- flags -> stages ---------------------------------------------------------------------------
    def stages(self):
        """[(M, filter, stride, feature maps)] per conv layer and (M, filter, stride) of the head.  The comma lists follow
        conv_gp/arguments.py:27-31: one M / filter size / stride per GP layer (head included), one feature-map count per conv layer.
        ``paddings()`` is the same list for --paddings."""
        fl = self.flags
        M, fmaps = parse_ints(fl.M), parse_ints(fl.feature_maps)
        filt, strd = parse_ints(fl.filter_sizes), parse_ints(fl.strides)
        assert len(strd) == len(filt)
        assert len(fmaps) == len(M) - 1
        convs = [(M[i], filt[i], strd[i], fmaps[i]) for i in range(len(fmaps))]
        return convs, (M[-1], filt[-1], strd[-1])

    def dilations(self):
        """--dilations: one dilation per conv layer (a head takes none); all ones without the flag."""
        return parse_dilations(self.flags, len(parse_ints(self.flags.M)) - 1)

    def paddings(self):
        """--paddings: one zero-padding width per GP layer (head included); all zeros without the flag."""
        return parse_paddings(self.flags, len(parse_ints(self.flags.M)))

    def mean_flags(self):
        """(mean kind, trainable) of --identity-mean / --mean-filter / --train-mean.  Kind None: no mean function; "conv2d": the reference's
        frozen Conv2dMean inside the layer launch (the flags' defaults under --identity-mean, exactly as before); otherwise a name of
        ``MEAN_FILTERS``: a ``LinearConv2dMean`` with that initial filter -- any non-default filter, and ``centre0`` itself with --train-mean.
        Either flag without --identity-mean and an unknown filter name raise ValueError naming the flag."""
        fl = self.flags
        identity = bool(getattr(fl, "identity_mean", False))
        kind = getattr(fl, "mean_filter", "centre0") or "centre0"
        train = bool(getattr(fl, "train_mean", False))
        if kind not in MEAN_FILTERS:
            raise ValueError("--mean-filter: expected %s, got %r" % (" | ".join(MEAN_FILTERS), kind))
        if not identity:
            if kind != "centre0":
                raise ValueError("--mean-filter %s: a mean filter needs --identity-mean" % kind)
            if train:
                raise ValueError("--train-mean: a trainable mean filter needs --identity-mean")
            return None, False
        if kind == "centre0" and not train:
            return "conv2d", False
        return kind, train

    def ard_flag(self):
        """--ard: every conv layer's RBF base kernel gets one lengthscale per patch element (gpflow's RBF(L, ARD=True)).  It needs
        --base-kernel rbf: with another base kernel ValueError names both flags."""
        ard = bool(getattr(self.flags, "ard", False))
        if ard and self.flags.base_kernel != "rbf":
            raise ValueError("--ard needs --base-kernel rbf, got --base-kernel %s (per-dimension lengthscales are provided for the RBF "
                             "base kernel only)" % self.flags.base_kernel)
        return ard

    def _conv_lengthscales(self, li, have, L, ard):
        """A conv layer's ``ls``: the checkpoint's value or the reference's initial 5.0 -- with --ard broadcast to the L patch elements; a
        stored vector without --ard raises ValueError naming the flag."""
        ls = np.asarray(have.get("ls", 5.0), np.float64)
        if ard:
            if ls.size not in (1, L):
                raise ValueError("--ard: layer %d's checkpoint holds %d lengthscales, its patches have %d elements" % (li, ls.size, L))
            return np.broadcast_to(ls.reshape(-1), (L,)).copy()
        if ls.size != 1:
            raise ValueError("layer %d's checkpoint holds %d lengthscales (a model trained with --ard): pass --ard to load it" % (li, ls.size))
        return float(ls.reshape(()))

    def _conv_base_kernel(self, li, have, L, ard):
        """The base kernel conv layer ``li`` starts with, as ``build_layers_from_spec`` will build it from the spec entry: what
        --inducing-init greedy selects its inducing patches under."""
        kind = self.flags.base_kernel
        if kind == "acos":
            return ArcCosine(L, order=0)
        variance, ls = float(have.get("variance", 5.0)), self._conv_lengthscales(li, have, L, ard)
        if ard:
            return RBF(L, variance, ls, ARD=True)
        return BASE_KERNELS[kind](L, variance, ls)

    @staticmethod
    def _report_stall(li, info, M):
        if info["n_greedy"] < M:
            print("layer {}: greedy selection stopped at {} of M = {} inducing points (conditional variance floor {}); "
                  "the rest are filled by residual.".format(li, info["n_greedy"], M, JITTER))

    def _greedy_patches(self, li, images, M, f, base_kernel, dilation=1):
        dil_kw = {"dilation": dilation} if dilation != 1 else {}
        feature = PatchInducingFeatures.from_images(images, M, f, method="greedy", base_kernel=base_kernel, **dil_kw)
        self._report_stall(li, feature.init_info, M)
        return feature.Z

    def _greedy_select(self, li, rows, M, base_kernel):
        Z, info = _kernels.greedy_variance(rows, M, base_kernel, return_info=True)
        self._report_stall(li, info, M)
        return Z

    # ---- stages -> spec ----------------------------------------------------------------------------
    def spec(self):
        fl = self.flags
        convs, (head_M, head_f, head_s) = self.stages()
        n_layers = len(convs) + 1
        pads = self.paddings()
        dils = self.dilations()
        stored = {}
        if getattr(fl, "load_model", None) is not None:
            self.global_step, stored = read_checkpoint(self.model_path, n_layers)
        if fl.base_kernel not in BASE_KERNELS:
            raise ValueError("Not a valid base-kernel value")
        if fl.last_kernel not in ("conv", "add", "rbf"):
            raise ValueError("Invalid last layer kernel")
        white = bool(fl.white)
        mean_kind, train_mean = self.mean_flags()
        latent = parse_latent_gps(fl, len(convs))         # --latent-gps: G per conv layer, 0 = unmixed
        ard = self.ard_flag()                              # --ard: per-dimension lengthscales on the conv layers
        init = parse_inducing_init(fl)                     # --inducing-init: kmeans (the reference's) | greedy
        spec = {"S": int(fl.num_samples), "num_data": int(self.X_train.shape[0]), "convs": []}
        images = self.X_train                              # what the next layer is initialised on
        for li, (M, f, s, R) in enumerate(convs):
            have = stored.get(li, {})
            _, H, W, C = images.shape                          # (H, W stay the unpadded size; "pad" carries the border)
            images = zero_pad(images, pads[li])                # inducing patches and the next layer's images: from what the window sees
            dil_kw = {"dilation": dils[li]} if dils[li] != 1 else {}      # (an undilated layer: the calls of before)
            if init == "kmeans" or "Z" in have:
                Z = have["Z"] if "Z" in have else PatchInducingFeatures.from_images(images, M, f, **dil_kw).Z
            else:               # --inducing-init greedy: M of the same candidates, by conditional variance under the kernel the layer starts with
                Z = self._greedy_patches(li, images, M, f, self._conv_base_kernel(li, have, f * f * C, ard), **dil_kw)
            G = latent[li] or R                                # the layer's GPs; R stays the maps it emits
            spec["convs"].append(dict(
                H=H, W=W, C=C, f=f, s=s, M=M, R=G, Z=Z, Z0=Z, white=white, base=fl.base_kernel, pad=pads[li], dil=dils[li],
                variance=float(have.get("variance", 5.0)), ls=self._conv_lengthscales(li, have, f * f * C, ard),     # models.py:114-117
                q_mu=have.get("q_mu"), q_sqrt=have.get("q_sqrt"),
                q_sqrt_scale=None if "q_sqrt" in have else 1e-5,                               # start with low variance (models.py:136-138)
                mean_function="conv2d" if mean_kind == "conv2d" else None))
            if latent[li]:      # a mixed layer: the checkpoint's W, else N(0, 1/G) entries seeded by the layer index
                W = have["mix_W"] if "mix_W" in have else mixing_matrix("random", G, R, seed=li)
                spec["convs"][-1].update(mix_W=mixing_matrix(W, G, R), mix_trainable=not bool(getattr(fl, "freeze_mixing", False)))
            if mean_kind not in (None, "conv2d"):             # LinearConv2dMean: the checkpoint's filter, else the named one
                W = have["mean_filter"] if "mean_filter" in have else conv_mean_filter(mean_kind, f, C, R)
                spec["convs"][-1].update(mean_filter=np.array(W, np.float64).reshape(f, f, C, R), mean_trainable=train_mean)
            if mean_kind in (None, "conv2d", "centre0"):
                images = identity_conv(images, f, C, R, s, **dil_kw)                            # models.py:29-33,104
            else:      # the same draw through the layer's own filter: the next layer's inducing patches are cut from what this one will emit
                images = filter_conv(images, spec["convs"][-1]["mean_filter"], s, **dil_kw)
        have = stored.get(n_layers - 1, {})
        _, H, W, C = images.shape
        images = zero_pad(images, pads[-1])
        if "Z" in have and fl.last_kernel != "rbf":
            stored_f = int(round(np.sqrt(have["Z"].shape[1] / C)))
            if stored_f != head_f:        # a head trained with another filter size starts afresh (models.py:152-158)
                print("filter_size {} != {} for last layer. Resetting parameters.".format(head_f, stored_f))
                have = {k: v for k, v in have.items() if k not in ("Z", "q_mu", "q_sqrt")}
        head = dict(H=H, W=W, C=C, f=head_f, s=head_s, M=head_M, R=10, white=white, kernel=fl.last_kernel, pad=pads[-1],
                    variance=float(have.get("variance", 5.0)), q_mu=have.get("q_mu"), q_sqrt=have.get("q_sqrt"))
        if fl.last_kernel == "rbf":
            # dense head on the flattened features: one lengthscale per dimension, k-means++ inducing points (models.py:24-27,160-168)
            flat = images.reshape(images.shape[0], -1)
            head["ls_ard"] = np.broadcast_to(np.asarray(have.get("ls", 5.0), np.float64), (flat.shape[1],)).copy()
            head["ls"] = 1.0
            if "Z" in have:
                head["Z"] = have["Z"]
            elif init == "greedy":      # all initialisation rows as candidates, a random 100 M of them when there are more
                rows = flat if flat.shape[0] <= 100 * head_M else flat[np.random.choice(flat.shape[0], 100 * head_M, replace=False)]
                head["Z"] = self._greedy_select(n_layers - 1, rows, head_M, RBF(flat.shape[1], head["variance"], head["ls_ard"], ARD=True))
            else:
                from sklearn import cluster
                head["Z"] = cluster.KMeans(n_clusters=head_M, init="k-means++", n_init=1).fit(flat).cluster_centers_
            head["w"] = np.ones(1)
        else:
            head["ls"] = float(have.get("ls", 5.0))
            if init == "kmeans" or "Z" in have:
                head["Z"] = have["Z"] if "Z" in have else PatchInducingFeatures.from_images(images, head_M, head_f).Z
            else:               # under the head's base kernel, its scalar RBF (not its weighted patch kernel)
                head["Z"] = self._greedy_patches(n_layers - 1, images, head_M, head_f, RBF(head_f * head_f * C, head["variance"], head["ls"]))
            head["w"] = have.get("w")
        spec["head"] = head
        return spec

    # ---- spec -> model -----------------------------------------------------------------------------
    def likelihood(self):
        """The ten-class likelihood --likelihood names: MultiClass(10) (RobustMax, the reference's) or Softmax(10)."""
        kind = getattr(self.flags, "likelihood", "robustmax")
        if kind not in LIKELIHOODS:
            raise ValueError("Not a valid likelihood value: %r (choices: %s)" % (kind, ", ".join(sorted(LIKELIHOODS))))
        return LIKELIHOODS[kind](10)

    def build(self):
        likelihood = self.likelihood()
        spec = self.spec()
        layers = build_layers_from_spec(spec)
        for layer, c in zip(layers, spec["convs"]):
            if c["q_sqrt_scale"] is not None:
                layer.q_sqrt = layer.q_sqrt * c["q_sqrt_scale"]
        X = self.X_train.reshape(-1, int(np.prod(self.X_train.shape[1:])))
        return DGP_Base(X, self.Y_train, likelihood=likelihood, num_samples=self.flags.num_samples,
                        layers=layers, minibatch_size=self.flags.batch_size, name='DGP')
