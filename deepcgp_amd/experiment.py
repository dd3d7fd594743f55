"""The experiment driver -- the counterpart of conv_gp/experiment.py (``Experiment``) and of the script around it
(conv_gp/mnist.py): flags -> data -> model -> ``test_every`` optimiser steps per period -> a ``log.csv`` row and a checkpoint per period.

A period of Adam steps is ONE device call (``DGP_Base.train_run``) on a training set that is uploaded once, when the model is set up;
``--augment-shift`` / ``--augment-flip`` augment its batches on the device (SGD and NatGrad: the same batches, one device call per step).
``--test-shift`` / ``--test-flip`` / ``--test-views`` score the test set over shifted and mirrored views (test-time augmentation).
``--keep-optimizer`` writes the optimiser's state beside every checkpoint and, with ``--load-model``, continues from it: the resumed run is the
interrupted one bit for bit.  ``--clip-norm`` clips every Adam / SGD step's gradient by its global norm on the device.
``--reselect-every N`` starts every N-th period by choosing the inducing patches again from what each layer receives now and carrying q(u) over.

    python -m deepcgp_amd.experiment --name run --data digits.npz -M 16,16 --feature-maps 2 --filter-sizes 3,3 --strides 1,1
"""
import os

import numpy as np

from . import utils
from .arguments import default_parser, parse_augmentation, parse_clip_norm, parse_reselect, parse_test_views, reselect_due, train_steps
from .models import (ModelBuilder, index_table, learning_rate, lr_table, restore_optimizer_state, save_model_parameters, save_optimizer_state,
                     train)


class Experiment(object):
    """conv_gp/experiment.py:13-136.  A subclass provides ``_load_data``: ``X_train`` [n, H, W, C], ``Y_train``, ``X_test``, ``Y_test``."""

    def __init__(self, flags):
        self.flags = flags
        self.seed = int(getattr(flags, "seed", 0))
        self.augmentation = parse_augmentation(flags)     # --augment-shift / --augment-flip: training batches only
        self.test_views = parse_test_views(flags)         # --test-shift / --test-flip / --test-views: None = the test images as they are
        self.clip_norm = parse_clip_norm(flags)           # --clip-norm: 0.0 = off (no call into the model, no logger)
        self.keep_optimizer = bool(getattr(flags, "keep_optimizer", False))
        self.reselect_every, self.reselect_images = parse_reselect(flags)     # --reselect-every: 0 = off (no call into the model)
        self._period_norms = np.zeros(0)                  # pre-clip gradient norms of the period that just ended (--clip-norm)
        self._load_data()
        self._setup_model()
        self._setup_optimizer()
        self._setup_logger()

    def _load_data(self):
        raise NotImplementedError()

    def conclude(self):
        self.log.close()

    def train_step(self):
        self._reselect()
        self._optimize()
        self._log_step()
        self._save_model_parameters()

    def _reselect(self):
        """--reselect-every N: every N-th period (never the first) starts by choosing the inducing patches again and carrying q(u) over
        (``DGP_Base.reselect_inducing``), whatever the optimiser.  The seed follows the step count, so a resumed run re-selects as the
        interrupted one would have."""
        if not reselect_due(getattr(self, "reselect_every", 0), self.global_step, self.flags.test_every):
            return
        for r in self.model.reselect_inducing(images=self.reselect_images, seed=self.seed + self.global_step):
            print("step {}: layer {} re-selected: {} of {} greedy, Nystrom trace {:.6g} -> {:.6g}, KL {:.6g} -> {:.6g}".format(
                self.global_step, r["layer"], r["n_greedy"], len(r["rows"]), r["trace_old"], r["trace_new"], r["kl_before"], r["kl_after"]))

    def _log_step(self):
        entry = self.log.write_entry(self.model)
        print(entry)

    def _optimize(self):
        """``flags.test_every`` optimiser steps (Loop(self.loop, stop=numiter), experiment.py:38-49).  Adam: one ``train_run``; SGD and NatGrad:
        ``models.train`` over the same span (NatGrad's retry with a smaller gamma needs the host between steps)."""
        k = int(self.flags.test_every)
        fl = self.flags
        if fl.optimizer == "Adam":
            n = self.model.X.shape[0]
            bs = min(self.model.minibatch_size or n, n)
            idx = index_table(self._rng, n, bs, k)
            lrs = lr_table(fl.lr, self.global_step, k, fl.lr_decay_steps)
            self.last_elbos = self.model.train_run(idx, lrs, seed=self.seed + self.global_step)
            if self.clip_norm > 0:
                self._period_norms = np.array(self.model.last_grad_norms)
            self.model.pull_parameters()
        else:
            norms = []      # --clip-norm: one optimiser call per step here, its norm read behind each
            watch = (lambda step, elbo: norms.extend(self.model.last_grad_norms)) if self.clip_norm > 0 else None
            self.last_elbos = np.array(train(self.model, k, lr=fl.lr, lr_decay_steps=fl.lr_decay_steps, global_step=self.global_step,
                                             seed=self.seed + self.global_step, optimizer=fl.optimizer, gamma=fl.gamma,
                                             augment=self.augmentation, callback=watch))
            if self.clip_norm > 0:
                self._period_norms = np.array(norms)
        self.global_step += k
        self.model.global_step = self.global_step

    def learning_rate(self):
        """The rate of the next step (experiment.py:71-73)."""
        return learning_rate(self.flags.lr, self.global_step, self.flags.lr_decay_steps)

    def _model_path(self, model_name=None):
        if model_name is None:
            model_name = self.flags.name
        return os.path.join(self.flags.log_dir, model_name + '.npy')

    def _optimizer_path(self, model_name=None):
        """The sidecar of ``_model_path(model_name)`` (--keep-optimizer)."""
        return self._model_path(model_name)[:-len('.npy')] + '.opt.npz'

    def _save_model_parameters(self):
        utils.ensure_dir(self.flags.log_dir)
        save_model_parameters(self.model, self._model_path(), self.global_step)
        if self.keep_optimizer:
            save_optimizer_state(self.model, self._optimizer_path(), self.global_step, rng=self._rng)

    def _setup_model(self):
        model_builder = ModelBuilder(self.flags, self.X_train, self.Y_train, model_path=self._model_path(self.flags.load_model))
        self.model = model_builder.build()
        # global_step goes on from a loaded checkpoint; Adam's bias correction restarts with the optimiser (include/dcgp.h, dcgp_model_adam_step)
        # unless --keep-optimizer puts the optimiser's state back (_setup_optimizer)
        self.global_step = int(model_builder.global_step or 0)
        self.model.global_step = self.global_step
        self.model.dedup_layer0 = True     # as models.train: the first layer sees S identical copies of the batch
        if self.flags.optimizer == "Adam":
            self.model.attach_dataset()    # once: every period draws its minibatches from it on the device
            self.model.set_augmentation(self.augmentation)     # ... and shifts / flips them there (the shift's upper bound is checked here)
        if self.clip_norm > 0:
            self.model.set_grad_clip(self.clip_norm)

    def _setup_optimizer(self):
        if self.flags.optimizer not in ["Adam", "NatGrad", "SGD"]:
            raise ValueError("Not a supported optimizer. Try Adam or NatGrad.")
        self._rng = np.random.default_rng(self.seed)     # the minibatch draws
        if self.keep_optimizer and getattr(self.flags, "load_model", None) is not None:
            # the run goes on where the checkpoint's run stood: moments, step count, prior patches and the generator of the minibatch draws
            restore_optimizer_state(self.model, self._optimizer_path(self.flags.load_model), self.global_step, rng=self._rng)

    def _setup_logger(self):
        X_test = self.X_test.reshape(self.X_test.shape[0], -1)
        accuracy = (utils.AccuracyLogger(X_test, self.Y_test) if self.test_views is None
                    else utils.TTAAccuracyLogger(X_test, self.Y_test, self.test_views))
        loggers = [
            utils.GlobalStepLogger(),
            accuracy,
            utils.LogLikelihoodLogger(),
        ]
        if parse_clip_norm(self.flags) > 0:      # --clip-norm: the period's mean pre-clip gradient norm
            loggers.append(utils.GradNormLogger(lambda: getattr(self, "_period_norms", ())))
        self.log = utils.Log(self.flags.log_dir, self.flags.name, loggers)
        self.log.write_flags(self.flags)


def standardise(X_train, X_test):
    """sklearn's StandardScaler fitted on the training images and applied to both sets (conv_gp/mnist.py:40-45): per pixel, zero mean and
    unit variance over the training set; a constant pixel is only centred.  Shapes are kept."""
    Xa = np.asarray(X_train, np.float64)
    Xb = np.asarray(X_test, np.float64)
    flat = Xa.reshape(Xa.shape[0], -1)
    mean, std = flat.mean(axis=0), flat.std(axis=0)
    std = np.where(std == 0.0, 1.0, std)
    return ((flat - mean) / std).reshape(Xa.shape), ((Xb.reshape(Xb.shape[0], -1) - mean) / std).reshape(Xb.shape)


class ArrayExperiment(Experiment):
    """An experiment on arrays the caller holds: images [n, H, W, C] (or [n, H, W]), integer labels.  ``flags.test_size`` test points are
    drawn without replacement (conv_gp/mnist.py:34-38)."""

    def __init__(self, flags, X_train, Y_train, X_test, Y_test):
        self._arrays = (X_train, Y_train, X_test, Y_test)
        super().__init__(flags)

    def _load_data(self):
        X_train, Y_train, X_test, Y_test = self._arrays
        X_train, X_test = np.asarray(X_train, np.float64), np.asarray(X_test, np.float64)
        if X_train.ndim == 3:
            X_train, X_test = X_train[..., None], X_test[..., None]
        if X_train.ndim != 4 or X_test.shape[1:] != X_train.shape[1:]:
            raise ValueError("images must be [n, H, W, C]; got %r and %r" % (X_train.shape, X_test.shape))
        self.X_train, self.Y_train = X_train, np.asarray(Y_train).reshape(-1, 1)
        Y_test = np.asarray(Y_test).reshape(-1, 1)
        if len(self.Y_train) != len(X_train) or len(Y_test) != len(X_test):
            raise ValueError("one label per image")
        chosen = np.random.RandomState(self.seed).choice(np.arange(len(X_test)), min(int(self.flags.test_size), len(X_test)), replace=False)
        self.X_test, self.Y_test = X_test[chosen], Y_test[chosen]


class NpzExperiment(ArrayExperiment):
    """``--data file.npz`` with the keys X_train, Y_train, X_test, Y_test; the images are standardised as the reference's MNIST script does."""

    def __init__(self, flags):
        with np.load(flags.data) as z:
            X_train, Y_train, X_test, Y_test = (np.array(z[k]) for k in ("X_train", "Y_train", "X_test", "Y_test"))
        X_train, X_test = standardise(X_train, X_test)
        super().__init__(flags, X_train, Y_train, X_test, Y_test)


def read_args(argv=None):
    parser = default_parser()
    parser.add_argument('--data', type=str, required=True, help="local .npz with X_train, Y_train, X_test, Y_test")
    return parser.parse_args(argv)


def main(argv=None):
    """conv_gp/mnist.py:58-67."""
    flags = read_args(argv)
    experiment = NpzExperiment(flags)
    try:
        for i in range(train_steps(flags)):
            experiment.train_step()
    finally:
        experiment.conclude()


if __name__ == "__main__":
    main()
