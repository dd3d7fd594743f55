"""Command-line flags of an experiment, as a table.

The flag NAMES and DEFAULTS are the reference's whole configuration system (/root/reference/conv_gp/arguments.py:9-43) and are
what its option files (results/*/options.toml) record, so they are kept to the letter; everything else here is this
repository's: one table, one loop, and a note per flag on what the device path does with it."""
import argparse
import math

# (flag, type or None for a switch, default, what it selects)
FLAGS = (
    ("--name", str, "experiment", "run name (log directory, checkpoint file name)"),
    ("--lr-decay-steps", int, 100000, "staircase period of the learning-rate decay (x 0.1 per period)"),
    ("--test-every", int, 50000, "optimisation steps between two test-set evaluations"),
    ("--test-size", int, 10000, "test images used per evaluation"),
    ("--num-samples", int, 10, "S: Monte-Carlo samples per image in the doubly-stochastic ELBO"),
    ("--log-dir", str, "results", "where logs and checkpoints go"),
    ("--lr", float, 0.01, "Adam / SGD learning rate (device optimiser: dcgp_model_adam_step / _sgd_step)"),
    ("--batch-size", int, 32, "minibatch size (images)"),
    ("--optimizer", str, "Adam", "Adam | SGD | NatGrad (NatGrad: variational parameters by natural gradient, rest by Adam)"),
    ("-M", str, "384,384", "inducing patches per layer, comma separated; one value = SVGP head only"),
    ("--feature-maps", str, "10", "outputs of each conv layer, comma separated ('' with a head-only model)"),
    ("--filter-sizes", str, "5,5", "patch size of each layer incl. the head"),
    ("--strides", str, "2,1", "patch stride of each layer incl. the head"),
    ("--paddings", str, "", "zero padding (pixels per side) of each layer's input incl. the head, comma separated; '' = no padding anywhere"),
    ("--dilations", str, "", "dilation (atrous rate) of each conv layer's window, comma separated, one per conv layer (the head takes none); '' = 1 everywhere"),
    ("--augment-shift", int, 0, "training images are shifted by up to this many pixels either way along both axes, zero fill ('pad and random-crop'); 0 = off"),
    ("--augment-flip", None, False, "training images are flipped left-right with probability one half"),
    ("--test-shift", int, 0, "test-time augmentation: the test images are also evaluated shifted by this many pixels (zero fill), the predictive distribution averaged over the views; 0 = off"),
    ("--test-flip", None, False, "test-time augmentation: every view also mirrored left-right"),
    ("--test-views", str, "cross", "which shifts --test-shift N takes: cross (0 and +-N along each axis, 5 views) | grid (all (2N+1)^2 shifts)"),
    ("--base-kernel", str, "rbf", "base kernel of the conv layers: rbf | acos | matern32 | matern52"),
    ("--ard", None, False, "per-dimension (ARD) lengthscales on the conv layers' base kernel: one per patch element, f*f*C a layer (needs --base-kernel rbf)"),
    ("--inducing-init", str, "kmeans", "how the inducing patches (dense head: inducing points) a checkpoint does not hold are chosen: kmeans (centres of 100 M random patches, the reference's) | greedy (M of the same candidates by greedy conditional variance under the layer's own kernel)"),
    ("--white", None, False, "whitened variational parameters"),
    ("--last-kernel", str, "conv", "head kernel: conv | add | rbf"),
    ("--likelihood", str, "robustmax", "multi-class likelihood: robustmax | softmax"),
    ("--gamma", float, 0.001, "NatGrad step size"),
    ("--identity-mean", None, False, "Conv2dMean identity mean function on the conv layers"),
    ("--mean-filter", str, "centre0", "initial filter of the conv layers' mean function (needs --identity-mean): centre0 (Conv2dMean's: channel 0 into map 0) | channels (every channel into its own map) | sum (every channel into every map)"),
    ("--train-mean", None, False, "train the mean function's filter with the other parameters (needs --identity-mean)"),
    ("--latent-gps", str, "", "mixed conv layers: latent GPs of each conv layer, comma separated; a layer with G > 0 holds G GPs and emits its --feature-maps count as a trainable linear mix of them; 0 = that layer unmixed; '' = no mixing anywhere"),
    ("--freeze-mixing", None, False, "keep the mixing matrices of --latent-gps at their initial values"),
    ("--load-model", str, None, "checkpoint (.npy, reference key set) to start from"),
    ("--keep-optimizer", None, False, "write the optimiser's state (Adam moments, step count, minibatch generator) beside every checkpoint as <name>.opt.npz; with --load-model X, continue from X.opt.npz: the resumed run is the interrupted one, bit for bit"),
    ("--reselect-every", int, 0, "every this many periods of --test-every, before the period's steps, choose every layer's inducing patches again (greedy conditional variance on what the layer receives now, under its trained kernel) and project q(u) onto them; 0 = off"),
    ("--reselect-images", int, 1000, "training images a re-selection propagates to cut its candidates from"),
    ("--clip-norm", float, 0.0, "clip every Adam / SGD step's gradient to this global norm on the device and log the period's mean pre-clip norm (grad_norm); 0 = off"),
)
REQUIRED = ("--name",)


def default_parser():
    """argparse parser over FLAGS (same namespace attributes as the reference's parser)."""
    parser = argparse.ArgumentParser(description="Deep convolutional GP experiment flags")
    for flag, kind, default, doc in FLAGS:
        if kind is None:
            parser.add_argument(flag, action="store_true", default=default, help=doc)
        else:
            parser.add_argument(flag, type=kind, default=default, required=flag in REQUIRED, help=doc)
    return parser


def parse_dilations(flags, n_convs):
    """The ``--dilations`` list of a model of ``n_convs`` conv layers: ``n_convs`` ints >= 1, all ones when the flag is absent or ''.  A
    wrong length, an entry < 1 or not an integer, and an entry > 1 on a layer whose ``--strides`` entry is not 1 raise ValueError."""
    text = getattr(flags, "dilations", "") or ""
    if not text.strip():
        return [1] * n_convs
    try:
        dils = [int(t) for t in text.split(",")]
    except ValueError:
        raise ValueError("--dilations: expected comma-separated integers, got %r" % (text,))
    if len(dils) != n_convs:
        raise ValueError("--dilations: %d entries for %d conv layers (one per conv layer, like --latent-gps: the head takes no dilation)"
                         % (len(dils), n_convs))
    if any(d < 1 for d in dils):
        raise ValueError("--dilations: entries must be >= 1, got %r" % (text,))
    strides = [int(t) for t in str(getattr(flags, "strides", "") or "").split(",") if t.strip()]
    for li, d in enumerate(dils):
        if d > 1 and li < len(strides) and strides[li] != 1:
            raise ValueError("--dilations: layer %d has dilation %d and --strides entry %d; a dilated layer needs stride 1" % (li, d, strides[li]))
    return dils


def parse_paddings(flags, n_layers):
    """The ``--paddings`` list of a model of ``n_layers`` GP layers (head included): ``n_layers`` ints >= 0, all zero when the flag is
    absent or ''.  A wrong length, a negative or non-integer entry, or padding on a dense (``--last-kernel rbf``) head raise ValueError."""
    text = getattr(flags, "paddings", "") or ""
    if text.strip() == "":
        return [0] * n_layers
    try:
        pads = [int(t) for t in text.split(",")]
    except ValueError:
        raise ValueError("--paddings: expected comma-separated integers, got %r" % (text,))
    if len(pads) != n_layers:
        raise ValueError("--paddings: %d entries for %d GP layers (one per layer, head included, like --strides)" % (len(pads), n_layers))
    if any(p < 0 for p in pads):
        raise ValueError("--paddings: entries must be >= 0, got %r" % (text,))
    if pads[-1] > 0 and getattr(flags, "last_kernel", "conv") == "rbf":
        raise ValueError("--paddings: the dense head of --last-kernel rbf takes no padding (last entry %d)" % pads[-1])
    return pads


def parse_latent_gps(flags, n_convs):
    """The ``--latent-gps`` list of a model of ``n_convs`` conv layers: ``n_convs`` ints >= 0 (0: that layer unmixed), all zero when the flag is
    absent or ''.  A wrong length, a negative or non-integer entry raise ValueError."""
    text = getattr(flags, "latent_gps", "") or ""
    if text.strip() == "":
        return [0] * n_convs
    try:
        gps = [int(t) for t in text.split(",")]
    except ValueError:
        raise ValueError("--latent-gps: expected comma-separated integers, got %r" % (text,))
    if len(gps) != n_convs:
        raise ValueError("--latent-gps: %d entries for %d conv layers (one per conv layer, like --feature-maps)" % (len(gps), n_convs))
    if any(g < 0 for g in gps):
        raise ValueError("--latent-gps: entries must be >= 0 (0 = unmixed), got %r" % (text,))
    return gps


def parse_augmentation(flags):
    """The ``augment.Augmentation`` of ``--augment-shift`` / ``--augment-flip`` (one that does nothing without them).  A negative shift raises
    ValueError; its upper bound, min(H, W) of the images, is checked where the geometry is known (``DGP_Base.set_augmentation``)."""
    from .augment import Augmentation
    shift = int(getattr(flags, "augment_shift", 0) or 0)
    if shift < 0:
        raise ValueError("--augment-shift: must be >= 0, got %d" % shift)
    return Augmentation(shift, bool(getattr(flags, "augment_flip", False)))


def parse_test_views(flags):
    """The views [V, 3] of ``--test-shift`` / ``--test-flip`` / ``--test-views`` (``augment.views``), or None with the flags at their defaults:
    the test set is then evaluated as it is.  A negative shift or an unknown pattern raise ValueError; the shift's upper bound, min(H, W) of the
    images, is checked where the geometry is known (``DGP_Base.evaluate``)."""
    from .augment import VIEW_PATTERNS, views
    shift = int(getattr(flags, "test_shift", 0) or 0)
    flip = bool(getattr(flags, "test_flip", False))
    pattern = getattr(flags, "test_views", "cross") or "cross"
    if shift < 0:
        raise ValueError("--test-shift: must be >= 0, got %d" % shift)
    if pattern not in VIEW_PATTERNS:
        raise ValueError("--test-views: expected %s, got %r" % (" | ".join(VIEW_PATTERNS), pattern))
    if shift == 0 and not flip:
        return None
    return views(shift, flip, pattern)


INDUCING_INITS = ("kmeans", "greedy")


def parse_inducing_init(flags):
    """``--inducing-init`` as one of ``INDUCING_INITS``: "kmeans" when the flag is absent; an unknown value raises ValueError naming the flag."""
    value = getattr(flags, "inducing_init", "kmeans") or "kmeans"
    if value not in INDUCING_INITS:
        raise ValueError("--inducing-init: expected %s, got %r" % (" | ".join(INDUCING_INITS), value))
    return value


def parse_clip_norm(flags):
    """``--clip-norm`` as a float: 0.0 (off) when the flag is absent; a negative value or NaN raises ValueError."""
    value = float(getattr(flags, "clip_norm", 0.0) or 0.0)
    if not value >= 0.0:
        raise ValueError("--clip-norm: must be >= 0 (0 = off), got %r" % (value,))
    return value


def parse_reselect(flags):
    """(``--reselect-every``, ``--reselect-images``) as ints: (0, 1000) when the flags are absent; 0 periods = off.  A negative period count or
    fewer than one image raises ValueError naming the flag."""
    every = getattr(flags, "reselect_every", 0)
    images = getattr(flags, "reselect_images", 1000)
    every, images = int(0 if every is None else every), int(1000 if images is None else images)
    if every < 0:
        raise ValueError("--reselect-every: must be >= 0 (0 = off), got %d" % every)
    if images < 1:
        raise ValueError("--reselect-images: must be >= 1, got %d" % images)
    return every, images


def reselect_due(every, global_step, test_every):
    """Whether the period that starts at ``global_step`` begins with a re-selection: its index ``global_step // test_every`` is a positive
    multiple of ``every`` (never the first period: the initialisation has just chosen the patches)."""
    period = int(global_step) // int(test_every)
    return every > 0 and period > 0 and period % every == 0


def train_steps(flags):
    """Number of test periods until the decayed learning rate reaches about 1e-5 (conv_gp/arguments.py:4-7)."""
    decades = math.log(5e-5 / flags.lr, 0.1)
    return math.ceil(decades * flags.lr_decay_steps / flags.test_every)
