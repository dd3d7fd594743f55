"""DGP_Base -- the model-level counterpart of doubly_stochastic_dgp.dgp.DGP_Base as the reference uses
it (/root/reference/conv_gp/models.py:65-70, conv_gp/utils/tensorboard.py:22-35, conv_gp/utils/log.py:62):
``propagate``, ``predict_y``, ``compute_log_likelihood`` and ``parameters``, plus DS-DGP's other prediction methods
(``predict_f``, ``predict_all_layers``, ``predict_density``) and a one-call test-set ``evaluate``.  The whole forward ELBO of a
minibatch is ONE call into the HIP library (``dcgp_elbo_forward``); parameters live on the device and
are pushed when changed (``sync_parameters``)."""
import contextlib
import ctypes as C

import numpy as np

from . import augment as _augment
from . import device as dev
from .kernels import JITTER
from .layers import ConvLayer, SVGP_Layer
from .mean_functions import conv_mean_filter
from .likelihoods import Bernoulli, Gaussian, Poisson, Softmax, StudentT


def batched_noise(zs, N, S, batch_size, dims=None, V=None):
    """Explicit noise of a whole set, per layer ``[S, N, D]`` (indexed by image, as ``dist.shard_batch`` slices it), in the layout
    ``dcgp_model_evaluate`` reads: per layer the batches' ``[S, n_b, D]`` tables back to back, batch b = images
    ``[b * batch_size, min((b + 1) * batch_size, N))``.  ``dims``: the layers' D (a table of another size raises).  Returns one
    flat array (or None) per layer.  ``V``: an evaluation over V views (dcgp_model_set_eval_views) -- per layer ``[S, V, N, D]``, the noise of
    view v of image i, into the batches' ``[S, V n_b, D]`` tables (row v n_b + i); a table of another size raises ValueError."""
    if zs is None:
        return None
    out = []
    for i, z in enumerate(zs):
        if z is None:
            out.append(None)
            continue
        if V is not None:
            D = -1 if dims is None else dims[i]
            if D > 0 and np.size(z) != S * V * N * D:
                raise ValueError("zs[%d]: %d values, an evaluation over views takes [S, V, N, D] = [%d, %d, %d, %d]" % (i, np.size(z), S, V, N, D))
            z = np.reshape(z, (S, V, N, D))
            out.append(np.concatenate([z[:, :, lo:lo + batch_size].reshape(-1) for lo in range(0, N, batch_size)]) if N else np.zeros(0))
            continue
        z = np.reshape(z, (S, N, -1 if dims is None else dims[i]))
        out.append(np.concatenate([z[:, lo:lo + batch_size].reshape(-1) for lo in range(0, N, batch_size)]) if N else np.zeros(0))
    return out


EVAL_MAX_SLOTS, UNC_EXTRA_SLOTS = 8192, 48      # csrc/layer.h: kEvalMaxSlots, kUncExtraSlots (the multi-class tails' LDS, in doubles)


class Parameter:
    """Minimal stand-in for a gpflow Param: ``pathname`` + value access (conv_gp/experiment.py:56-62)."""

    def __init__(self, pathname, getter, setter):
        self.pathname = pathname
        self._get, self._set = getter, setter

    @property
    def value(self):
        return self._get()

    def assign(self, v):
        self._set(v)


class DGP_Base:
    def __init__(self, X, Y, likelihood, layers, minibatch_size=None, num_samples=1, name='DGP', num_data=None):
        self.X = np.ascontiguousarray(X, np.float64)
        self.likelihood = likelihood
        self.layers = list(layers)
        self.gaussian = isinstance(likelihood, Gaussian)
        self.bernoulli = isinstance(likelihood, Bernoulli)
        self.softmax = isinstance(likelihood, Softmax)           # int32 labels like MultiClass; its node table is pushed at build time
        self.student_t = isinstance(likelihood, StudentT)       # robust regression: the trainable scale where the Gaussian variance lives
        self.poisson = isinstance(likelihood, Poisson)          # count targets
        self.float_targets = self.gaussian or self.bernoulli or self.student_t or self.poisson     # float64 N x D targets and the _f64y entry points
        self.Y = self._targets_host(Y) if self.float_targets else np.ascontiguousarray(np.reshape(Y, (-1,)), np.int32)
        self.num_samples = int(num_samples)
        self.minibatch_size = minibatch_size
        self.name = name
        self.num_data = int(num_data if num_data is not None else self.X.shape[0])
        self.global_batch = None      # multi-rank runs: the minibatch size summed over the ranks (see _default_scale)
        self.dedup_layer0 = False     # exact optimisation: layer 0 sees S identical copies of the batch
        self._ctx = None
        self._model = None
        self._batch_rng = np.random.RandomState(0)    # Minibatch(seed=0)
        self._dataset = None          # (rows, attached without arguments?) of the set attach_dataset put on the device
        self.augmentation = None      # the Augmentation set_augmentation put on the device model (None: off)
        if not self.layers or not isinstance(self.layers[-1], SVGP_Layer):
            raise ValueError("the last layer must be an SVGP_Layer")
        for l in self.layers[:-1]:
            if not isinstance(l, ConvLayer):
                raise ValueError("hidden layers must be ConvLayer instances")

    def _targets_host(self, Y, n=None):
        """Gaussian, Bernoulli, StudentT or Poisson likelihood: float64 targets N x D, D the head's num_outputs (Bernoulli: bool, int or
        float values in {0, 1}; Poisson: finite non-negative integer values)."""
        D = self.layers[-1].num_outputs
        kind = self._lik_name()
        Y = np.asarray(Y)
        if self.bernoulli and Y.size and not np.all((Y == 0) | (Y == 1)):
            raise ValueError("Bernoulli likelihood: targets must be 0 or 1")
        if self.poisson and Y.size:
            Yf = Y.astype(np.float64)
            if not np.all(np.isfinite(Yf)):
                raise ValueError("Poisson likelihood: targets must be finite")
            if not np.all(Yf >= 0):
                raise ValueError("Poisson likelihood: targets must be >= 0")
            if not np.all(Yf == np.floor(Yf)):
                raise ValueError("Poisson likelihood: targets must be integer-valued counts")
        Y = Y.astype(np.float64)
        if Y.ndim == 1 and D == 1:
            Y = Y[:, None]
        if Y.ndim != 2 or Y.shape[1] != D:
            raise ValueError("%s likelihood: targets must be N x %d (the head's num_outputs), got shape %r" % (kind, D, np.shape(Y)))
        if n is not None and Y.shape[0] != n:
            raise ValueError("%d targets for %d images" % (Y.shape[0], n))
        return np.ascontiguousarray(Y)

    def _lik_name(self):
        for flag, name in (("gaussian", "Gaussian"), ("bernoulli", "Bernoulli"), ("student_t", "StudentT"), ("poisson", "Poisson"),
                           ("softmax", "Softmax")):
            if getattr(self, flag):
                return name
        return "RobustMax"

    def _targets(self, Y, N):
        """(device targets, float64?) of an explicit minibatch: float64 N x D (Gaussian, Bernoulli) or int32 labels."""
        if self.float_targets:
            if isinstance(Y, dev.DeviceArray):
                if Y.dtype != np.float64 or int(np.prod(Y.shape)) != N * self.layers[-1].num_outputs:
                    raise ValueError("float-target likelihood: device targets must be float64 N x %d" % self.layers[-1].num_outputs)
                return Y, True
            return self._ctx.to_device(self._targets_host(Y, N)), True
        return self._ctx.as_device(np.reshape(Y, (-1,)) if not isinstance(Y, dev.DeviceArray) else Y, np.int32), False

    def _default_scale(self, n_local):
        """num_data / minibatch size.  With an RCCL communicator on the ctx the data term is summed over the ranks inside
        the device call, so the minibatch is the GLOBAL one: set ``global_batch`` (or pass ``scale``) -- the local shard
        size would make the ELBO too large by the rank count."""
        if getattr(self._ctx, "nranks", 1) > 1:
            if getattr(self, "global_batch", None) is None:
                raise ValueError("an RCCL communicator is attached: pass scale=num_data/global_batch or set model.global_batch")
            return float(self.num_data) / float(self.global_batch)
        return float(self.num_data) / float(n_local)

    # ---- device model -----------------------------------------------------------------------------
    def _ptr(self, a):
        return np.ascontiguousarray(a, np.float64).ctypes.data

    def _check_means(self):
        """Every model-level call: the mean functions the device model was built with must still be the ones on the layers (a
        Conv2dMean whose conv_filter was changed afterwards would run as the centre-pixel mean at the model level and through its
        generic __call__ at the layer level -- a silent disagreement)."""
        for li, l in enumerate(self.layers[:-1]):
            now = (bool(l.identity_mean), getattr(l, "generic_mean", None) is not None, getattr(l, "filter_mean", None) is not None)
            if now != self._built_means[li]:
                raise ValueError("layer %d: mean function changed after the device model was built (identity_mean %r -> %r, generic "
                                 "%r -> %r); build a new model" % (li, self._built_means[li][0], now[0], self._built_means[li][1], now[1]))

    def _build(self):
        if self._model is not None:
            self._check_means()
            return
        self._built_means = [(bool(l.identity_mean), getattr(l, "generic_mean", None) is not None, getattr(l, "filter_mean", None) is not None)
                             for l in self.layers[:-1]]
        ctx = self._ctx = dev.get_context()
        L = dev.lib()
        h = C.c_void_p()
        ctx._check(L.dcgp_model_create(ctx.handle, self.num_samples, JITTER, C.byref(h)))
        self._model = h.value
        for li, l in enumerate(self.layers[:-1]):
            v = l.view
            if getattr(l, "generic_mean", None) is not None:
                # the one-call ELBO adds Conv2dMean's centre pixel inside the layer launch (the only mean the reference builds,
                # conv_gp/models.py:95-99); an arbitrary callable exists at the layer level only
                raise ValueError("layer %d: the model path takes mean_function None / Zero() / Conv2dMean with its initial filter "
                                 "(or a LinearConv2dMean, whose filter lives on the device); got %r" % (li, l.mean_function))
            keep = [np.ascontiguousarray(a, np.float64) for a in (l.feature.Z, l.Z_prior, l.q_mu, l.q_sqrt)]
            Hp, Wp = getattr(v, "padded_size", v.input_size[:2])      # the device layer is a VALID layer on the padded image
            ctx._check(L.dcgp_model_add_conv_layer(
                self._model, Hp, Wp, l.feature_maps_in, v.filter_size, v.stride,
                l.num_inducing, l.gp_count, int(l.white), int(l.identity_mean), l.base_kernel.variance,
                1.0 if getattr(l.base_kernel, "ARD", False) else getattr(l.base_kernel, "lengthscales", 1.0), *[a.ctypes.data for a in keep]))
            if l.mixing is not None:           # G = gp_count latent GPs into R maps (csrc/mix.hip); ahead of the mean filter, which has R columns
                W = self._mixing_host(l)
                ctx._check(L.dcgp_model_set_mixing(self._model, li, W.ctypes.data, W.shape[0], W.shape[1]))
                if not getattr(l, "mixing_trainable", True):
                    ctx._check(L.dcgp_model_set_trainable(self._model, li, b"mixing", 0))
            if l.centre_mean:                  # a mixed layer's Conv2dMean: the frozen centre-pixel filter on the R maps
                W = np.ascontiguousarray(conv_mean_filter("centre0", v.filter_size, v.feature_maps, l.feature_maps_out), np.float64)
                ctx._check(L.dcgp_model_set_mean_filter(self._model, li, W.ctypes.data, 0))
            if l.filter_mean is not None:      # LinearConv2dMean: its filter [f, f, C, R] is the device's [L][R] as it stands (csrc/conv_mean.hip)
                W = self._mean_filter_host(l)
                ctx._check(L.dcgp_model_set_mean_filter(self._model, li, W.ctypes.data, int(bool(l.filter_mean.trainable))))
            desc = np.ascontiguousarray(l.base_kernel._describe(), np.float64)
            if desc[0] != 0.0:   # not the RBF the constructor call describes (ArcCosine, conv_gp/models.py:118-119)
                ctx._check(L.dcgp_model_set_param(self._model, li, b"base_kernel",
                                                  desc.ctypes.data, desc.size))
            if getattr(l.base_kernel, "ARD", False):     # RBF(f f C, ARD=True): one lengthscale per patch element (csrc/rbf.hip: the sweep's ARD instance)
                ls = np.ascontiguousarray(l.base_kernel.lengthscales, np.float64)
                ctx._check(L.dcgp_model_set_param(self._model, li, b"ard_lengthscales", ls.ctypes.data, ls.size))
        h_ = self.layers[-1]
        if hasattr(h_.kern, "base_kernel"):      # ConvKernel / AdditivePatchKernel head (--last-kernel conv | add)
            v = h_.kern.view
            Hp, Wp = getattr(v, "padded_size", v.input_size[:2])
            geom = (Hp, Wp, v.feature_maps, v.filter_size, v.stride)
            ktype, base, weights = int(h_.kern.kernel_type), h_.kern.base_kernel, h_.kern.patch_weights
        else:                                    # dense RBF head on the flattened features (--last-kernel rbf): one patch = the input
            geom = (1, 1, h_.kern.input_dim, 1, 1)
            ktype, base, weights = 0, h_.kern, np.ones(1)
        keep = [np.ascontiguousarray(a, np.float64) for a in (h_.feature.Z, weights, h_.q_mu, h_.q_sqrt)]
        ctx._check(L.dcgp_model_set_head(
            self._model, *geom, h_.num_inducing, h_.num_outputs, int(h_.white), ktype, base.variance,
            1.0 if getattr(base, "ARD", False) else base.lengthscales, *[a.ctypes.data for a in keep]))
        if getattr(base, "ARD", False):
            ls = np.ascontiguousarray(base.lengthscales, np.float64)
            ctx._check(L.dcgp_model_set_param(self._model, len(self.layers) - 1, b"ard_lengthscales", ls.ctypes.data, ls.size))
        for li, l in enumerate(self.layers[:-1]):  # dilation: the layer was added with its true size; the device runs it on the phase sub-images
            if getattr(l.view, "dilation", 1) > 1:
                ctx._check(L.dcgp_model_set_dilation(self._model, li, int(l.view.dilation)))
        for li, l in enumerate(self.layers):      # zero padding: the layer's input is its predecessor's output (X for layer 0) plus the border
            v = l.view if li < len(self.layers) - 1 else getattr(l.kern, "view", None)
            if getattr(v, "padding", 0):
                ctx._check(L.dcgp_model_set_input_padding(self._model, li, int(v.padding)))
        eps = np.array([float(getattr(self.likelihood, "epsilon", 1e-3))])
        ctx._check(L.dcgp_model_set_param(self._model, 0, b"likelihood_epsilon", eps.ctypes.data, 1))
        if self.gaussian:
            ctx._check(L.dcgp_model_set_likelihood(self._model, 1, float(self.likelihood.variance)))
        elif self.bernoulli:
            ctx._check(L.dcgp_model_set_likelihood(self._model, 2, 0.0))
        elif self.softmax:
            if self.likelihood.num_classes != h_.num_outputs:
                raise ValueError("Softmax(%d) on a head with %d outputs" % (self.likelihood.num_classes, h_.num_outputs))
            ctx._check(L.dcgp_model_set_likelihood(self._model, 3, 0.0))
            self.push_likelihood_nodes()
            self.likelihood._attach(self)
        elif self.student_t or self.poisson:
            par = np.ascontiguousarray(self.likelihood._params(), np.float64)
            ctx._check(L.dcgp_model_set_likelihood_params(self._model, self.likelihood.kind, par.ctypes.data, par.size))

    @staticmethod
    def _mean_filter_host(layer):
        """A layer's LinearConv2dMean filter as one contiguous float64 [f, f, C, R] array (ValueError for another shape)."""
        mf, v = layer.filter_mean, layer.view
        W = np.ascontiguousarray(mf.conv_filter, np.float64)
        shape = (v.filter_size, v.filter_size, v.feature_maps, layer.feature_maps_out)
        if W.shape != shape:
            raise ValueError("LinearConv2dMean.conv_filter must be %s, got %s" % (shape, W.shape))
        return W

    @staticmethod
    def _mixing_host(layer):
        """A mixed layer's W as one contiguous float64 [gp_count, feature_maps_out] array (ValueError for another shape)."""
        W = np.ascontiguousarray(layer.mixing, np.float64)
        if W.shape != (layer.gp_count, layer.feature_maps_out):
            raise ValueError("ConvLayer.mixing must be %s, got %s" % ((layer.gp_count, layer.feature_maps_out), W.shape))
        return W

    def push_likelihood_nodes(self):
        """Softmax likelihood: copy ``likelihood.nodes`` [Q, K] to the built device model (dcgp_model_set_likelihood_nodes).  The table is no
        parameter: factor reuse keeps its chain.  Not allowed while enqueued steps are outstanding."""
        if not self.softmax or self._model is None:
            return
        nodes = np.ascontiguousarray(self.likelihood.nodes, np.float64)
        self._ctx._check(dev.lib().dcgp_model_set_likelihood_nodes(self._model, nodes.ctypes.data, nodes.shape[0]))

    def sync_parameters(self):
        """Push the current Python-side parameter values to the device copy."""
        self._build()
        L, ctx = dev.lib(), self._ctx

        def push(li, which, val):
            a = np.ascontiguousarray(np.atleast_1d(val), np.float64)
            ctx._check(L.dcgp_model_set_param(self._model, li, which.encode(), a.ctypes.data, a.size))
        for li, l in enumerate(self.layers):
            head = li == len(self.layers) - 1
            kern = (l.kern.base_kernel if hasattr(l.kern, "base_kernel") else l.kern) if head else l.base_kernel
            push(li, "Z", l.feature.Z)
            push(li, "q_mu", l.q_mu)
            push(li, "q_sqrt", l.q_sqrt)
            push(li, "base_kernel", kern._describe())
            if getattr(kern, "ARD", False):
                push(li, "ard_lengthscales", kern.lengthscales)
            if head:
                if hasattr(l.kern, "patch_weights"):
                    push(li, "w", l.kern.patch_weights)
            else:
                push(li, "Z0", l.Z_prior)
                if l.filter_mean is not None:
                    push(li, "mean_filter", self._mean_filter_host(l))
                if l.mixing is not None:
                    push(li, "mixing", self._mixing_host(l))
        push(0, "likelihood_epsilon", float(getattr(self.likelihood, "epsilon", 1e-3)))
        if self.gaussian:
            push(0, "likelihood_variance", float(self.likelihood.variance))
        if self.student_t:
            push(0, "likelihood_scale", float(self.likelihood.scale))

    @property
    def parameters(self):
        """Objects with ``pathname`` + ``value`` in the reference's checkpoint naming
        (DGP/layers/<i>/..., notebooks/Inspect.ipynb cell 6)."""
        out = []
        if self.gaussian:                            # Gaussian variance under the BroadcastingLikelihood wrapper's doubled path
            out.append(Parameter("%s/likelihood/likelihood/variance" % self.name, lambda: np.array(self.likelihood.variance),
                                 lambda v: setattr(self.likelihood, "variance", float(v))))
        if self.student_t:                           # StudentT scale, beside the Gaussian's path (deg_free is no parameter)
            out.append(Parameter("%s/likelihood/likelihood/scale" % self.name, lambda: np.array(self.likelihood.scale),
                                 lambda v: setattr(self.likelihood, "scale", float(v))))
        if hasattr(self.likelihood, "epsilon"):     # RobustMax epsilon under the BroadcastingLikelihood wrapper's doubled path
            out.append(Parameter("%s/likelihood/likelihood/invlink/epsilon" % self.name, lambda: np.array(self.likelihood.epsilon),
                                 lambda v: setattr(self.likelihood, "epsilon", float(v))))
        for i, l in enumerate(self.layers):
            head = i == len(self.layers) - 1
            base = "%s/layers/%d" % (self.name, i)
            dense = head and not hasattr(l.kern, "base_kernel")
            kern = (l.kern if dense else l.kern.base_kernel) if head else l.base_kernel
            kpath = base + (("/kern" if dense else "/kern/base_kernel") if head else "/conv_kernel/base_kernel")
            out.append(Parameter(kpath + "/variance", lambda k=kern: np.array(k.variance), lambda v, k=kern: setattr(k, "variance", float(v))))
            for pname in (("lengthscales",) if hasattr(kern, "lengthscales") else ("weight_variances", "bias_variance")):
                out.append(Parameter(kpath + "/" + pname, lambda k=kern, n=pname: np.array(getattr(k, n)),
                                     lambda v, k=kern, n=pname: setattr(k, n, np.array(v, np.float64) if np.ndim(v) else float(v))))
            out.append(Parameter(base + "/feature/Z", lambda l=l: l.feature.Z, lambda v, l=l: setattr(l.feature, "Z", np.array(v, np.float64))))
            out.append(Parameter(base + "/q_mu", lambda l=l: l.q_mu, lambda v, l=l: setattr(l, "q_mu", np.array(v, np.float64))))
            out.append(Parameter(base + "/q_sqrt", lambda l=l: l.q_sqrt, lambda v, l=l: setattr(l, "q_sqrt", np.array(v, np.float64))))
            if not head and getattr(l, "filter_mean", None) is not None:      # LinearConv2dMean only (the reference freezes Conv2dMean's filter)
                out.append(Parameter(base + "/mean_function/conv_filter", lambda l=l: l.filter_mean.conv_filter,
                                     lambda v, l=l: setattr(l.filter_mean, "conv_filter",
                                                            np.array(v, np.float64).reshape(np.shape(l.filter_mean.conv_filter)))))
            if not head and getattr(l, "mixing", None) is not None:
                out.append(Parameter(base + "/mixing/W", lambda l=l: l.mixing,
                                     lambda v, l=l: setattr(l, "mixing", np.array(v, np.float64).reshape(np.shape(l.mixing)))))
            if head and not dense:
                out.append(Parameter(base + "/kern/patch_weights", lambda l=l: l.kern.patch_weights,
                                     lambda v, l=l: setattr(l.kern, "patch_weights", np.array(v, np.float64))))
        return out

    # ---- forward ----------------------------------------------------------------------------------
    def _z_table(self, zs, N, S):
        if zs is None:
            return None, []
        ctx, keep = self._ctx, []
        arr = (C.c_void_p * len(self.layers))()
        for i, z in enumerate(zs):
            if z is None:
                arr[i] = None
                continue
            D = self._out_dims()[i]
            if np.size(z) != S * N * D:
                raise ValueError("zs[%d] has %d values, layer %d draws S x N x D = %d x %d x %d = %d (a mixed layer: one per patch and latent GP)"
                                 % (i, np.size(z), i, S, N, D, S * N * D))
            dz = ctx.to_device(np.reshape(z, (S, N, D)))
            keep.append(dz)
            arr[i] = dz.ptr
        return arr, keep

    def compute_log_likelihood(self, X=None, Y=None, zs=None, seed=0, scale=None, return_parts=False):
        """ELBO of an explicit minibatch: sum_n E_q log p(y_n | f_n) * num_data / batch - sum_l KL_l
        (doubly_stochastic_dgp DGP_Base._build_likelihood; explicit feeds as at
        conv_gp/utils/tensorboard.py:32-35).  Without arguments a minibatch of ``minibatch_size`` is drawn."""
        self._build()
        if X is None:
            idx = self._batch_rng.choice(self.X.shape[0], size=min(self.minibatch_size or self.X.shape[0], self.X.shape[0]), replace=False)
            X, Y = self.X[idx], self.Y[idx]
        ctx, L = self._ctx, dev.lib()
        dX = ctx.as_device(np.reshape(X, (np.shape(X)[0], -1)) if not isinstance(X, dev.DeviceArray) else X)
        N = dX.shape[0]
        dY, f64y = self._targets(Y, N)
        if scale is None:
            scale = self._default_scale(N)
        arr, keep = self._z_table(zs, N, self.num_samples)
        out = (C.c_double * 3)()
        info = C.c_int(0)
        rc = (L.dcgp_elbo_forward_f64y if f64y else L.dcgp_elbo_forward)(self._model, dX.ptr, dY.ptr, N, float(scale), arr, int(seed), int(self.dedup_layer0), out, C.byref(info))
        ctx._check(rc, info)
        if return_parts:
            return out[0], out[1], out[2]
        return out[0]

    def enqueue_log_likelihood(self, X, Y, zs=None, seed=0, scale=None):
        """Throughput mode of ``compute_log_likelihood``: queue one ELBO step and return a ticket without waiting for
        the device (``dcgp_elbo_forward_enqueue``); ``collect_log_likelihood(ticket)`` returns its value.  At most 4
        tickets may be outstanding and they are collected in order.  The device buffers of the step are kept alive
        with the ticket."""
        self._build()
        ctx, L = self._ctx, dev.lib()
        dX = ctx.as_device(np.reshape(X, (np.shape(X)[0], -1)) if not isinstance(X, dev.DeviceArray) else X)
        N = dX.shape[0]
        dY, f64y = self._targets(Y, N)
        if scale is None:
            scale = self._default_scale(N)
        arr, keep = self._z_table(zs, N, self.num_samples)
        ticket = C.c_uint64(0)
        ctx._check((L.dcgp_elbo_forward_enqueue_f64y if f64y else L.dcgp_elbo_forward_enqueue)(self._model, dX.ptr, dY.ptr, N, float(scale), arr, int(seed), int(self.dedup_layer0),
                                               C.byref(ticket)))
        if not hasattr(self, "_inflight"):
            self._inflight = {}
        self._inflight[ticket.value] = (dX, dY, arr, keep)
        return ticket.value

    def collect_log_likelihood(self, ticket, return_parts=False):
        """Wait for an enqueued step and return its ELBO (same value and errors as ``compute_log_likelihood``)."""
        ctx, L = self._ctx, dev.lib()
        out = (C.c_double * 3)()
        info = C.c_int(0)
        rc = L.dcgp_elbo_forward_collect(self._model, int(ticket), out, C.byref(info))
        if rc != dev.ERR_ARG:
            getattr(self, "_inflight", {}).pop(int(ticket), None)
        ctx._check(rc, info)
        if return_parts:
            return out[0], out[1], out[2]
        return out[0]

    def compute_gradients(self, X, Y, zs=None, seed=0, scale=None, fetch=True, shards=None):
        """(ELBO, [per-layer dict]) -- the value and gradient TensorFlow hands the optimiser at
        conv_gp/experiment.py:84-108, from the hand-written reverse pass (csrc/grad.hip).  Keys: ``Z``,
        ``q_mu``, ``q_sqrt`` (lower triangle), ``variance``, ``lengthscales`` and, for the head,
        ``patch_weights``; a conv layer with a ``LinearConv2dMean`` adds ``mean_filter`` [f, f, C, R] (zero while the filter is frozen), a mixed
        conv layer ``mixing`` [G, R] (zero while frozen);
        all with respect to the constrained values."""
        self._build()
        ctx, L = self._ctx, dev.lib()
        dX = ctx.as_device(np.reshape(X, (np.shape(X)[0], -1)) if not isinstance(X, dev.DeviceArray) else X)
        N = dX.shape[0]
        dY, f64y = self._targets(Y, N)
        if scale is None:
            scale = self._default_scale(N)
        arr, keep = self._z_table(zs, N, self.num_samples)
        out = (C.c_double * 3)()
        info = C.c_int(0)
        # this call handles one of `shards` batch shards: the replicated KL term is weighted 1 / shards; None = the rank
        # count of the ctx's communicator (1 without one).  Always passed, so that it never sticks from an earlier call.
        ctx._check(L.dcgp_model_set_grad_shards(self._model, int(shards or 0)))
        ctx._check((L.dcgp_elbo_grad_f64y if f64y else L.dcgp_elbo_grad)(self._model, dX.ptr, dY.ptr, N, float(scale), arr, int(seed), int(self.dedup_layer0), out,
                                    C.byref(info)), info)
        if not fetch:            # the gradients stay on the device (dcgp_model_get_grad / the optimiser step read them there)
            return out[0], None
        grads = []
        for li, l in enumerate(self.layers):
            head = li == len(self.layers) - 1
            M, R = l.num_inducing, (l.num_outputs if head else l.gp_count)
            shapes = {"Z": (M, np.shape(l.feature.Z)[1]), "q_mu": (M, R), "q_sqrt": (R, M, M), "variance": (), "lengthscale": ()}
            if head and hasattr(l.kern, "patch_weights"):
                shapes["w"] = (np.size(l.kern.patch_weights),)
            ard = l.kern if head else l.base_kernel
            if getattr(ard, "ARD", False):       # dense RBF(ARD) head, ARD conv layer: one lengthscale per input dimension / patch element
                del shapes["lengthscale"]
                shapes["ard_lengthscales"] = (np.size(ard.lengthscales),)
            if not head and not hasattr(l.base_kernel, "lengthscales"):   # ArcCosine(order 0) base kernel
                del shapes["lengthscale"]
                shapes["weight_variances"], shapes["bias_variance"] = (), ()
            if not head and l.filter_mean is not None:
                shapes["mean_filter"] = np.shape(l.filter_mean.conv_filter)
            if not head and l.mixing is not None:
                shapes["mixing"] = np.shape(l.mixing)
            g = {}
            for which, shp in shapes.items():
                buf = np.empty(shp, np.float64)
                ctx._check(L.dcgp_model_get_grad(self._model, li, which.encode(), buf.ctypes.data, buf.size))
                g[{"lengthscale": "lengthscales", "ard_lengthscales": "lengthscales", "w": "patch_weights"}.get(which, which)] = buf
            grads.append(g)
        if self.gaussian:        # d ELBO / d likelihood variance, with the head's gradients
            buf = np.empty(1, np.float64)
            ctx._check(L.dcgp_model_get_grad(self._model, 0, b"likelihood_variance", buf.ctypes.data, 1))
            grads[-1]["likelihood_variance"] = buf.reshape(())
        if self.student_t:       # d ELBO / d likelihood scale, in the same slot
            buf = np.empty(1, np.float64)
            ctx._check(L.dcgp_model_get_grad(self._model, 0, b"likelihood_scale", buf.ctypes.data, 1))
            grads[-1]["likelihood_scale"] = buf.reshape(())
        return out[0], grads

    OBJECTIVES = {"density": 0, "elbo": 1}

    def _input_grad_args(self, S, objective):
        """Argument checks of ``input_gradient`` that need no device: (S, objective code)."""
        if objective not in self.OBJECTIVES:
            raise ValueError("objective must be 'density' or 'elbo', got %r" % (objective,))
        if objective == "density" and self.float_targets:
            raise NotImplementedError("input_gradient: the 'density' objective exists for the RobustMax and Softmax likelihoods only; a %s model takes "
                                      "objective='elbo'" % self._lik_name())
        S = self.num_samples if S is None else int(S)
        if S < 1:
            raise ValueError("S must be >= 1")
        return S, self.OBJECTIVES[objective]

    def input_gradient(self, X, Y, S=None, objective="density", zs=None, seed=0):
        """(J [N], dX [N, D_in]): a per-image objective and its gradient with respect to the input pixels, one device call
        (dcgp_model_input_grad).  ``objective="density"``: J_n = log 1/S sum_s p(y_n | f_sn), the value ``predict_density`` returns for
        the same (S, zs, seed) (RobustMax models); ``"elbo"``: J_n = 1/S sum_s E_q[log p(y_n | f_sn)], the image's unscaled share of the
        ELBO's data term (every likelihood).  ``S=None`` takes ``num_samples``; ``zs`` per layer [S, N, D].  X and Y may be host arrays
        or DeviceArrays.  Training state (parameters, gradients on the device, Adam moments, factor reuse) is left untouched."""
        S, code = self._input_grad_args(S, objective)
        N = np.shape(X)[0] if not isinstance(X, dev.DeviceArray) else X.shape[0]
        if N == 0:
            return np.zeros(0), np.zeros((0, self.X.shape[1]))
        if not isinstance(X, dev.DeviceArray):
            X = np.reshape(X, (N, -1))
            if X.shape[1] != self.X.shape[1]:
                raise ValueError("images of %d values, the model takes %d" % (X.shape[1], self.X.shape[1]))
        if not self.float_targets and not isinstance(Y, dev.DeviceArray):
            Yh = np.reshape(Y, (-1,))
            K = self.layers[-1].num_outputs
            if Yh.size != N:
                raise ValueError("%d labels for %d images" % (Yh.size, N))
            if Yh.size and (Yh.min() < 0 or Yh.max() >= K):
                raise ValueError("labels outside [0, %d)" % K)
        self._build()
        ctx, L = self._ctx, dev.lib()
        dX = ctx.as_device(X)
        dY, f64y = self._targets(Y, N)
        arr, keep = self._z_table(zs, N, S)
        J, g = ctx.empty((N,)), ctx.empty((N, self.X.shape[1]))
        info = C.c_int(0)
        code |= dev.INPUT_GRAD_DEDUP if self.dedup_layer0 else 0
        ctx._check((L.dcgp_model_input_grad_f64y if f64y else L.dcgp_model_input_grad)(self._model, dX.ptr, dY.ptr, N, S, arr, int(seed), code, J.ptr, g.ptr,
                                                                                     C.byref(info)), info)
        return J.numpy(), g.numpy()

    def saliency(self, X, Y=None, S=None, objective="density", zs=None, seed=0):
        """Saliency maps [N, H, W, C]: ``input_gradient``'s dX in the first layer's image shape.  ``Y=None`` takes the model's own
        prediction (``predict_proba(X, S, zs, seed).argmax(1)``, the same noise) as the label."""
        S = self.num_samples if S is None else int(S)
        if Y is None:
            if self.float_targets:
                raise ValueError("saliency: a Gaussian or Bernoulli model needs targets Y" if self.gaussian or self.bernoulli else
                                 "saliency: a %s model needs targets Y" % self._lik_name())
            Y = self.predict_proba(X, S, zs=zs, seed=seed).argmax(axis=1)
        _, g = self.input_gradient(X, Y, S=S, objective=objective, zs=zs, seed=seed)
        l0 = self.layers[0]
        v = l0.view if hasattr(l0, "view") else getattr(l0.kern, "view", None)
        if v is None:      # dense head on flat features: no image shape
            return g
        C_in = l0.feature_maps_in if hasattr(l0, "feature_maps_in") else v.feature_maps
        return g.reshape(g.shape[0], v.input_size[0], v.input_size[1], C_in)

    def adam_step(self, lr, t=None, beta1=0.9, beta2=0.999, epsilon=1e-8):
        """One Adam step (tf.train.AdamOptimizer defaults, gpflow.train.AdamOptimizer at
        conv_gp/experiment.py:104-107) on the gradients the last ``compute_gradients`` left on the device,
        in gpflow's unconstrained space.  ``t`` is the 1-based step count of the bias correction; None (default) = the
        device model's own count of steps since its moment buffers were created (independent of any global_step a
        checkpoint carried, like a freshly built tf optimiser).  The device copy of the parameters
        moves; ``pull_parameters`` refreshes the Python-side values."""
        self._ctx._check(dev.lib().dcgp_model_adam_step(self._model, float(lr), float(beta1), float(beta2), float(epsilon), int(t or 0)))

    def train_step(self, X, Y, lr, zs=None, seed=0, scale=None, t=None, beta1=0.9, beta2=0.999, epsilon=1e-8, shards=None):
        """One training step in one call -- ``compute_gradients`` and ``adam_step`` enqueued back to back with a single wait
        at the end (dcgp_model_train_step_adam): the optimiser's ``minimize`` step of conv_gp/experiment.py:84-108.  Returns the
        step's ELBO (evaluated before the update, as TensorFlow's fetch of the objective beside the train op would be).  A step whose
        K_uu is not positive definite raises and leaves every parameter as it was."""
        self._build()
        ctx, L = self._ctx, dev.lib()
        dX = ctx.as_device(np.reshape(X, (np.shape(X)[0], -1)) if not isinstance(X, dev.DeviceArray) else X)
        N = dX.shape[0]
        dY, f64y = self._targets(Y, N)
        if scale is None:
            scale = self._default_scale(N)
        arr, keep = self._z_table(zs, N, self.num_samples)
        out = (C.c_double * 3)()
        info = C.c_int(0)
        ctx._check(L.dcgp_model_set_grad_shards(self._model, int(shards or 0)))
        ctx._check((L.dcgp_model_train_step_adam_f64y if f64y else L.dcgp_model_train_step_adam)(self._model, dX.ptr, dY.ptr, N, float(scale), arr, int(seed), int(self.dedup_layer0),
                                                float(lr), float(beta1), float(beta2), float(epsilon), int(t or 0), out, C.byref(info)), info)
        return out[0]

    # ---- a training run on the device -------------------------------------------------------------
    def _row_length(self):
        """Values per image, H * W * C of the first layer's UNPADDED input (a padded first layer adds its border on the device)."""
        l = self.layers[0]
        if len(self.layers) > 1:
            return int(l.view.input_size[0] * l.view.input_size[1] * l.feature_maps_in)
        if hasattr(l.kern, "base_kernel"):
            v = l.kern.view
            return int(v.input_size[0] * v.input_size[1] * v.feature_maps)
        return int(l.kern.input_dim)

    def attach_dataset(self, X=None, Y=None):
        """Upload a training set once (dcgp_model_set_dataset); ``train_run`` then draws its batches from it on the device.  Defaults to the
        model's own ``X``, ``Y``.  Replaces an earlier set.  Targets are validated as for an explicit minibatch (``_targets_host``)."""
        self._build()
        default = X is None and Y is None
        X = self.X if X is None else X
        Y = self.Y if Y is None else Y
        X = np.ascontiguousarray(np.reshape(X, (np.shape(X)[0], -1)), np.float64)
        n = X.shape[0]
        if n < 1:
            raise ValueError("attach_dataset: the set is empty")
        if X.shape[1] != self._row_length():
            raise ValueError("attach_dataset: images of %d values, the model's first layer takes %d" % (X.shape[1], self._row_length()))
        if self.float_targets:
            Y = self._targets_host(Y, n)
        else:
            Y = np.ascontiguousarray(np.reshape(Y, (-1,)), np.int32)
            if Y.shape[0] != n:
                raise ValueError("%d targets for %d images" % (Y.shape[0], n))
        self._dataset = None
        self._ctx._check(dev.lib().dcgp_model_set_dataset(self._model, X.ctypes.data, Y.ctypes.data, n, int(self.float_targets)))
        self._dataset = (n, default)

    def detach_dataset(self):
        """Release the set ``attach_dataset`` uploaded."""
        if self._model is not None and self._dataset is not None:
            self._ctx._check(dev.lib().dcgp_model_set_dataset(self._model, None, None, 0, 0))
        self._dataset = None

    # ---- training-time augmentation ---------------------------------------------------------------
    def _image_geometry(self):
        """(H, W, C) of one image of the caller's X, from the first layer's view (unpadded); a dense head-only model has none."""
        l = self.layers[0]
        if len(self.layers) > 1:
            return int(l.view.input_size[0]), int(l.view.input_size[1]), int(l.feature_maps_in)
        if hasattr(l.kern, "base_kernel"):
            v = l.kern.view
            return int(v.input_size[0]), int(v.input_size[1]), int(v.feature_maps)
        raise ValueError("augmentation needs image geometry: this model is a dense head alone (--last-kernel rbf without conv layers), its "
                         "inputs are vectors of %d features, not H x W x C images" % int(l.kern.input_dim))

    def _checked_augmentation(self, aug):
        """(H, W, C, max_shift, hflip) of an Augmentation on this model's images; ValueError when it does not fit them."""
        H, W, Cc = self._image_geometry()
        t = int(aug.max_shift)
        if t < 0:
            raise ValueError("augmentation: max_shift must be >= 0, got %d" % t)
        if t >= min(H, W):
            raise ValueError("augmentation: max_shift %d must be < min(H, W) = %d of the model's %d x %d x %d images (--augment-shift)"
                             % (t, min(H, W), H, W, Cc))
        return H, W, Cc, t, int(bool(aug.hflip))

    def set_augmentation(self, aug):
        """Augment the batches of ``train_run`` on the device (dcgp_model_set_augmentation): ``aug`` an ``augment.Augmentation``; None, or one
        that does nothing, switches it off.  The geometry is the first layer's view's (unpadded); a dense head-only model raises ValueError.
        Only ``train_run`` consults it (and ``augment``): evaluation, prediction, ``input_gradient``, the loggers and the per-step calls see
        their images as they are (test-time augmentation is ``evaluate(views=...)``, a per-call argument).  No parameter: checkpoints do not hold it.  Not allowed while enqueued steps are outstanding."""
        args = self._checked_augmentation(aug) if aug else (0, 0, 0, 0, 0)
        if not aug and self._model is None:      # nothing built, nothing to switch off
            self.augmentation = None
            return
        self._build()
        try:
            self._ctx._check(dev.lib().dcgp_model_set_augmentation(self._model, *args))
        except dev.DcgpError as e:
            if e.code != dev.ERR_ARG:
                raise
            raise ValueError(str(e)) from None       # (enqueued steps still to be collected: the library's own check)
        self.augmentation = aug if aug else None

    def augment(self, X, seed):
        """The model's augmentation on an explicit batch, on the device (dcgp_augment_images): image b with the draw of (seed, b) --
        ``augment.apply(X, *augment.draw(seed, len(X), max_shift, hflip))`` to the bit.  X [N, H W C] or [N, H, W, C]; returns a new array
        of X's shape.  Without an augmentation set: a copy of X."""
        X = np.ascontiguousarray(X, np.float64)
        if not self.augmentation or X.shape[0] == 0:
            return X.copy()
        self._build()
        H, W, Cc, t, hflip = self._checked_augmentation(self.augmentation)
        if X.size != X.shape[0] * H * W * Cc:
            raise ValueError("augment: images of shape %r, the model's are %d x %d x %d" % (X.shape[1:], H, W, Cc))
        ctx = self._ctx
        dX, out = ctx.to_device(X), ctx.empty(X.shape)
        ctx._check(dev.lib().dcgp_augment_images(ctx.handle, dX.ptr, X.shape[0], H, W, Cc, t, hflip, int(seed) & 0xFFFFFFFFFFFFFFFF, out.ptr))
        return out.numpy()

    def train_run(self, idx, lr, seed=0, scale=None, beta1=0.9, beta2=0.999, epsilon=1e-8):
        """``steps`` training steps in one device call (dcgp_model_train_run_adam) -- ``Loop(self.loop, stop=test_every)`` of
        conv_gp/experiment.py:38-49.  ``idx`` [steps, batch]: the rows of the attached set each step trains on; ``lr``: a scalar or one rate
        per step; step i draws its noise from ``seed + i``; ``scale`` defaults to num_data / batch.  Returns the steps' ELBOs; they, the
        parameters and the optimiser state are those of ``steps`` calls ``train_step(X[idx[i]], Y[idx[i]], lr[i], seed=seed + i)`` bit for
        bit.  Raises what ``train_step`` raises, with the failing step in the message and in the exception's ``.step`` and the ELBOs of the
        completed steps in its ``.history``; bad arguments raise ``ValueError`` before anything is launched.
        With an augmentation set (``set_augmentation``) the gather also shifts and flips each image, with draws made on the device: step i is
        then ``train_step(augment.apply(X[idx[i]], *augment.draw(seed + i, batch, max_shift, hflip)), Y[idx[i]], lr[i], seed=seed + i)``, bit
        for bit (X[idx[i]] as [batch, H, W, C]).  Targets are untouched; with ``dedup_layer0`` an image is augmented once per step and its S
        replicas share the result (the batch is tiled afterwards)."""
        self._build()
        ctx, L = self._ctx, dev.lib()
        if self._dataset is None:
            raise ValueError("train_run: no dataset attached (attach_dataset)")
        if getattr(ctx, "nranks", 1) > 1:
            raise NotImplementedError("train_run drives one GPU; shard the minibatch per rank and call train_step yourself")
        n = self._dataset[0]
        idx = np.asarray(idx)
        if idx.ndim != 2 or idx.size == 0 or idx.dtype.kind not in "iu":
            raise ValueError("train_run: idx must be an integer array [steps, batch], got %s %r" % (idx.dtype, idx.shape))
        steps, batch = idx.shape
        if idx.min() < 0 or idx.max() >= n:
            raise ValueError("train_run: indices must lie in [0, %d), got [%d, %d]" % (n, idx.min(), idx.max()))
        idx = np.ascontiguousarray(idx, np.int32)
        lr = np.asarray(lr, np.float64)
        if lr.ndim == 0:
            lr = np.full(steps, float(lr))
        if lr.shape != (steps,):
            raise ValueError("train_run: %d steps but a learning-rate table of shape %r" % (steps, lr.shape))
        if not np.all(lr > 0):
            raise ValueError("train_run: every learning rate must be > 0")
        lr = np.ascontiguousarray(lr)
        if scale is None:
            scale = float(self.num_data) / float(batch)
        elbo = np.zeros(steps, np.float64)
        done, info = C.c_int(0), C.c_int(0)
        ctx._check(L.dcgp_model_set_grad_shards(self._model, 0))
        rc = L.dcgp_model_train_run_adam(self._model, idx.ctypes.data, steps, batch, float(scale), lr.ctypes.data, int(seed), int(self.dedup_layer0),
                                         float(beta1), float(beta2), float(epsilon), elbo.ctypes.data, C.byref(done), C.byref(info))
        if rc != dev.DCGP_OK:
            try:
                ctx._check(rc, info)
            except dev.DcgpError as e:
                e.args = ("%s (train_run: step %d of %d)" % (e.args[0] if e.args else "", done.value, steps),) + tuple(e.args[1:])
                e.step = done.value
                e.history = elbo[:done.value].copy()
                raise
        return elbo

    def set_grad_exchange(self, mode):
        """Multi-rank ``train_step``: 0 = all-reduce of the gradient blocks, every rank updates everything; 1 = reduce-scatter, Adam on this
        rank's shard of every layer's parameter block, all-gather of the parameters (dcgp_model_set_grad_exchange; dist.sharded_adam_step is
        the same three steps on host arrays)."""
        self._build()
        self._ctx._check(dev.lib().dcgp_model_set_grad_exchange(self._model, int(mode)))

    def set_factor_reuse(self, mode):
        """Parameter-only state across steps (dcgp_model_set_factor_reuse): 0 = every step runs the factorisation chain; 1 (default) = ``propagate`` /
        ``predict_y`` skip it while no parameter was pushed or stepped since the chain last ran (the reference's AccuracyLogger sweeps a test set at
        one parameter state, conv_gp/utils/log.py:55-68); 2 = ``compute_log_likelihood`` as well (LogLikelihoodLogger-style sweeps).  Bit-identical
        results; a training step never reuses it."""
        self._build()
        self._ctx._check(dev.lib().dcgp_model_set_factor_reuse(self._model, int(mode)))

    @property
    def chain_skips(self):
        """Steps of this model that reused the parameter-only chain of an earlier step (``set_factor_reuse``)."""
        self._build()
        out = C.c_uint64(0)
        self._ctx._check(dev.lib().dcgp_model_chain_skips(self._model, C.byref(out)))
        return int(out.value)

    def factor_groups(self):
        """[(Mp, matrices, riding)] of the factor groups the most recent step ran (dcgp_model_factor_groups): one batched factorisation chain per
        distinct padded size Mp, the matrices it factors and how many of them carried G / alpha on the chain.  Empty before the first step."""
        self._build()
        cap = 16
        n, Mp, mats, ride = C.c_int(0), (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
        self._ctx._check(dev.lib().dcgp_model_factor_groups(self._model, cap, C.byref(n), Mp, mats, ride))
        return [(Mp[q], mats[q], ride[q]) for q in range(min(n.value, cap))]

    def debug_sharded_adam(self, ranks, lr, t=None, beta1=0.9, beta2=0.999, epsilon=1e-8):
        """Debugging aid: ``adam_step`` taken the way ``ranks`` ranks take it in exchange mode 1, played on this one GPU (bit-identical).  Needs the
        complete gradient of a ``compute_gradients`` call."""
        self._build()
        self._ctx._check(dev.lib().dcgp_model_debug_sharded_adam(self._model, int(ranks), float(lr), float(beta1), float(beta2), float(epsilon), int(t or 0)))

    def sgd_step(self, lr):
        """Plain gradient ascent step in the unconstrained space (the "SGD" branch, conv_gp/experiment.py:100-103)."""
        self._ctx._check(dev.lib().dcgp_model_sgd_step(self._model, float(lr)))

    # ---- optimiser state and gradient clipping ----------------------------------------------------
    def _optimizer_groups(self):
        """[(key prefix, layer, group name, shape)] of every parameter group the device optimiser keeps Adam moments for
        (dcgp_model_get_adam_state's names), in the groups' own shapes."""
        out = []
        for li, l in enumerate(self.layers):
            head = li == len(self.layers) - 1
            base = "layers/%d/" % li
            out.append((base + "Z", li, "Z", np.shape(l.feature.Z)))
            out.append((base + "q_mu", li, "q_mu", np.shape(l.q_mu)))
            out.append((base + "q_sqrt", li, "q_sqrt", np.shape(l.q_sqrt)))
            if head:      # (a dense head keeps its single weight's slot)
                out.append((base + "w", li, "w", (int(np.size(l.kern.patch_weights)) if hasattr(l.kern, "patch_weights") else 1,)))
            out.append((base + "hyper", li, "hyper", (3,)))
            ard = l.kern if head else l.base_kernel
            if getattr(ard, "ARD", False):
                out.append((base + "ard_lengthscales", li, "ard_lengthscales", (int(np.size(ard.lengthscales)),)))
            if not head and l.filter_mean is not None:
                out.append((base + "mean_filter", li, "mean_filter", np.shape(l.filter_mean.conv_filter)))
            if not head and l.mixing is not None:
                out.append((base + "mixing", li, "mixing", np.shape(l.mixing)))
        if self.gaussian or self.student_t:
            out.append(("likelihood", 0, "likelihood", (1,)))
        return out

    def optimizer_state(self):
        """The device optimiser's own state: ``{"t": Adam's step count, "<group>/m": first moments, "<group>/v": second moments}`` for every
        group of ``_optimizer_groups`` -- ``layers/<i>/<Z | q_mu | q_sqrt | w | hyper | ard_lengthscales | mean_filter | mixing>`` and ``likelihood`` --
        in the unconstrained space the optimiser works in.  A model that has never stepped reports zeros and ``t = 0``.  With the parameters
        (``pull_parameters``) it is everything a later step depends on: see ``set_optimizer_state``."""
        self._build()
        ctx, L = self._ctx, dev.lib()
        t = C.c_int(0)
        ctx._check(L.dcgp_model_get_adam_t(self._model, C.byref(t)))
        state = {"t": int(t.value)}
        for key, li, which, shape in self._optimizer_groups():
            m, v = np.empty(shape, np.float64), np.empty(shape, np.float64)
            ctx._check(L.dcgp_model_get_adam_state(self._model, li, which.encode(), m.ctypes.data, v.ctypes.data, m.size))
            state[key + "/m"], state[key + "/v"] = m, v
        return state

    def set_optimizer_state(self, state):
        """Put an ``optimizer_state()`` back (of this model or of one with the same layers): the next step is then the step the other model
        would have taken at the same parameters.  A missing or extra key or a wrong shape raises ValueError naming the key; nothing is
        written in that case."""
        self._build()
        ctx, L = self._ctx, dev.lib()
        groups = self._optimizer_groups()
        want = {"t": ()}
        for key, _, _, shape in groups:
            want[key + "/m"] = want[key + "/v"] = tuple(shape)
        for key in want:
            if key not in state:
                raise ValueError("set_optimizer_state: key %r is missing" % key)
        for key in state:
            if key not in want:
                raise ValueError("set_optimizer_state: unexpected key %r" % key)
        arrays = {}
        for key, shape in want.items():
            a = np.asarray(state[key])
            if a.shape != shape:
                raise ValueError("set_optimizer_state: %r has shape %r, expected %r" % (key, a.shape, shape))
            arrays[key] = np.ascontiguousarray(a, np.float64)
        t = int(state["t"])
        if t < 0:
            raise ValueError("set_optimizer_state: 't' must be >= 0, got %d" % t)
        for key, li, which, _ in groups:
            m, v = arrays[key + "/m"], arrays[key + "/v"]
            ctx._check(L.dcgp_model_set_adam_state(self._model, li, which.encode(), m.ctypes.data, v.ctypes.data, m.size))
        ctx._check(L.dcgp_model_set_adam_t(self._model, t))

    def set_grad_clip(self, max_norm):
        """Clip every Adam / SGD step's gradient by its global norm on the device (dcgp_model_set_grad_clip; ``tf.clip_by_global_norm`` on the
        unconstrained variables the optimiser moves): the step uses ``g * max_norm / max(norm, max_norm)``.  0 switches it off (the default),
        ``inf`` measures the norm and scales nothing.  The natural-gradient update is not clipped.  Negative or NaN raises ValueError."""
        max_norm = float(max_norm)
        if not max_norm >= 0.0:
            raise ValueError("set_grad_clip: max_norm must be >= 0 (0: off, inf: measure only), got %r" % (max_norm,))
        self._build()
        self._ctx._check(dev.lib().dcgp_model_set_grad_clip(self._model, max_norm))
        self.grad_clip = max_norm

    @property
    def last_grad_norms(self):
        """Pre-clip global gradient norms of the steps of the most recent optimiser call (dcgp_model_grad_norms): one value after ``adam_step``,
        ``sgd_step`` or ``train_step``, one per completed step after ``train_run``; empty while clipping is off."""
        self._build()
        ctx, L = self._ctx, dev.lib()
        n = C.c_int(0)
        ctx._check(L.dcgp_model_grad_norms(self._model, None, 0, C.byref(n)))
        out = np.empty(n.value, np.float64)
        if n.value:
            ctx._check(L.dcgp_model_grad_norms(self._model, out.ctypes.data, n.value, C.byref(n)))
        return out

    def set_shard(self, first_image, global_batch):
        """Multi-GPU: this rank holds images [first_image, first_image + N) of a minibatch of ``global_batch`` images (dist.shard_range).
        Also sets ``global_batch`` for the default ELBO scale.  The device RNG then draws every element at its position in the un-sharded
        batch: a step's ELBO is the same whatever the number of ranks."""
        self._build()
        dev.get_context()._check(dev.lib().dcgp_model_set_shard(self._model, int(first_image), int(global_batch)))
        self.global_batch = int(global_batch) if global_batch else None

    def set_trainable(self, layer, which, on):
        """param.set_trainable(on) for the device optimiser steps: which in Z, q_mu, q_sqrt, w, hyper (every kernel parameter of the layer);
        weight_variances, bias_variance (that one parameter of an ArcCosine conv layer); ard_lengthscales (the per-dimension lengthscales of
        an ARD layer alone, its variance goes on moving); "likelihood_variance" (Gaussian likelihood,
        ``layer`` ignored); "likelihood_scale" (StudentT likelihood, ``layer`` ignored); "mean_filter" (the filter of a conv layer's
        ``LinearConv2dMean``: frozen, its gradient is not formed either); "mixing" (a mixed conv layer's W, likewise)."""
        self._build()
        if which == "mean_filter":
            mf = getattr(self.layers[int(layer)], "filter_mean", None) if 0 <= int(layer) < len(self.layers) - 1 else None
            if mf is None:
                raise ValueError("set_trainable: layer %d has no LinearConv2dMean" % int(layer))
            mf.trainable = bool(on)
        if which == "mixing":
            l = self.layers[int(layer)] if 0 <= int(layer) < len(self.layers) - 1 else None
            if getattr(l, "mixing", None) is None:
                raise ValueError("set_trainable: layer %d is not mixed" % int(layer))
            l.mixing_trainable = bool(on)
        self._ctx._check(dev.lib().dcgp_model_set_trainable(self._model, int(layer), which.encode(), int(bool(on))))

    def natgrad_step(self, gamma):
        """One natural-gradient step of size ``gamma`` on every layer's (q_mu, q_sqrt) -- gpflow.train.NatGradOptimizer
        on var_list=[(l.q_mu, l.q_sqrt)] as set up at conv_gp/experiment.py:90-99 -- from the gradients the last
        ``compute_gradients`` left on the device (dcgp_model_natgrad_step, csrc/natgrad.hip: batched Cholesky chains and
        GEMMs, nothing crosses the bus).  Raises ``numpy.linalg.LinAlgError`` and leaves the parameters untouched when
        the step leaves the positive-definite cone (the reference's loop then scales gamma back, experiment.py:36-49)."""
        info = C.c_int(0)
        rc = dev.lib().dcgp_model_natgrad_step(self._model, float(gamma), C.byref(info))
        if rc == dev.ERR_NOT_PD:
            raise np.linalg.LinAlgError("natural-gradient step not positive definite (column %d); reduce gamma" % info.value)
        self._ctx._check(rc, info)

    def pull_parameters(self):
        """Read the device copy of every trainable value back into the layer / kernel objects."""
        self._build()
        L, ctx = dev.lib(), self._ctx

        def pull(li, which, shape):
            buf = np.empty(shape, np.float64)
            ctx._check(L.dcgp_model_get_param(self._model, li, which.encode(), buf.ctypes.data, buf.size))
            return buf
        for li, l in enumerate(self.layers):
            head = li == len(self.layers) - 1
            kern = (l.kern.base_kernel if hasattr(l.kern, "base_kernel") else l.kern) if head else l.base_kernel
            l.feature.Z = pull(li, "Z", np.shape(l.feature.Z))
            l.q_mu = pull(li, "q_mu", np.shape(l.q_mu))
            l.q_sqrt = pull(li, "q_sqrt", np.shape(l.q_sqrt))
            kern.variance = float(pull(li, "variance", ()))
            if getattr(kern, "ARD", False):
                kern.lengthscales = pull(li, "ard_lengthscales", (np.size(kern.lengthscales),))
            elif hasattr(kern, "lengthscales"):
                kern.lengthscales = float(pull(li, "lengthscale", ()))
            else:                                             # ArcCosine(order 0)
                kern.weight_variances = float(pull(li, "weight_variances", ()))
                kern.bias_variance = float(pull(li, "bias_variance", ()))
            if head and hasattr(l.kern, "patch_weights"):
                l.kern.patch_weights = pull(li, "w", np.shape(l.kern.patch_weights))
            if not head and l.filter_mean is not None:
                l.filter_mean.conv_filter = pull(li, "mean_filter", np.shape(l.filter_mean.conv_filter))
            if not head and l.mixing is not None:
                l.mixing = pull(li, "mixing", np.shape(l.mixing))
        if self.gaussian:
            self.likelihood.variance = float(pull(0, "likelihood_variance", ()))
        if self.student_t:
            self.likelihood.scale = float(pull(0, "likelihood_scale", ()))

    # ---- re-selection of the inducing inputs during training -----------------------------------------
    @staticmethod
    def _reselect_rng(seed, stream):
        """The generator of one draw of ``reselect_inducing``: stream 0 the images, 1 + li layer li's candidates.  Never the global one."""
        return np.random.RandomState(np.array([int(seed) & 0xffffffff, int(stream)], np.uint32))

    def _reselect_kernel(self, li):
        """The kernel layer ``li`` selects under: a conv layer's base kernel, a patch head's scalar RBF, the dense head's ARD RBF."""
        l = self.layers[li]
        if li < len(self.layers) - 1:
            return l.base_kernel
        return l.kern.base_kernel if hasattr(l.kern, "base_kernel") else l.kern

    def _reselect_inputs(self, X_rows, Fs):
        """What every layer receives for the images ``X_rows``, from one propagation's samples ``Fs``: the image (layer 0) or the layer below's
        sample as that layer's output image -- a mixed layer's emitted maps --, with the layer's own zero border; the dense head: flat rows."""
        out = []
        for li, l in enumerate(self.layers):
            src = X_rows if li == 0 else Fs[li - 1][0]
            head = li == len(self.layers) - 1
            v = getattr(l.kern, "view", None) if head else l.view
            if v is None:
                out.append(np.ascontiguousarray(src.reshape(src.shape[0], -1), np.float64))
                continue
            img = np.asarray(src, np.float64).reshape(src.shape[0], v.input_size[0], v.input_size[1], v.feature_maps)
            out.append(np.ascontiguousarray(v.pad(img)))
        return out

    def reselect_candidates(self, li, layer_input, seed, candidates=100):
        """The candidates layer ``li`` selects from: ``candidates * M`` patches of its input drawn with the generator of (seed, li); the dense
        head: the flat rows themselves."""
        l = self.layers[li]
        if layer_input.ndim == 2:
            return layer_input
        head = li == len(self.layers) - 1
        v = l.kern.view if head else l.view
        from .models import draw_patches      # (a dilated layer: its candidates are dilated windows of what it receives)
        return np.ascontiguousarray(draw_patches(layer_input, int(candidates) * l.num_inducing, v.filter_size, self._reselect_rng(seed, 1 + li),
                                                 dilation=getattr(v, "dilation", 1)))

    def reselect_inducing(self, layers=None, images=1000, seed=0, candidates=100, min_variance=JITTER):
        """Choose the inducing inputs of ``layers`` (default: all) again, from what each layer receives NOW and under the kernel it has NOW,
        and carry q(u) over.  ``images`` training images (drawn with a generator of ``seed``) go through one ``propagate(S=1, seed=seed)``;
        per layer, ``candidates * M`` patches of its input (its flat rows for the dense head) are the candidates, ``kernels.greedy_variance``
        picks M of them, and ``kernels.transfer_inducing`` projects q(u) onto them (q'(u') = int p(u' | u) q(u) du; a transfer is a projection,
        also onto an unchanged Z).  All layers are computed from the one propagation, then written together: Z, q_mu, q_sqrt, on conv layers
        the KL prior's patches too; ``sync_parameters`` (a kept factor chain is no longer valid); the Adam moments of those three groups of
        those layers are zeroed, every other moment and the step count stay.  Fewer than M usable candidates: ValueError; a transfer that is
        not positive definite: ``NotPositiveDefinite``; the model is unchanged either way.  Not with a shard set (multi-rank models).

        Returns one dict per layer: ``layer``, ``rows`` (the candidates chosen), ``n_greedy``, ``trace_new`` (the candidates' Nystrom trace
        under the new Z, the selection's last), ``trace_old`` (the same trace under the old Z, with K_uu's jitter), ``kl_before``,
        ``kl_after`` (the layer's KL term)."""
        from scipy.linalg import solve_triangular
        from . import kernels as _k
        if self.global_batch is not None or getattr(self._ctx or dev.get_context(), "nranks", 1) > 1:
            raise NotImplementedError("reselect_inducing: not on a sharded (multi-rank) model")
        n_layers = len(self.layers)
        which = list(range(n_layers)) if layers is None else sorted(set(int(li) for li in layers))
        if any(li < 0 or li >= n_layers for li in which):
            raise ValueError("reselect_inducing: layers must be in 0 .. %d, got %r" % (n_layers - 1, layers))
        if int(images) < 1 or int(candidates) < 1:
            raise ValueError("reselect_inducing: images and candidates must be >= 1")
        self._build()
        self.pull_parameters()
        n = self.X.shape[0]
        idx = self._reselect_rng(seed, 0).choice(n, size=min(int(images), n), replace=False)
        X_rows = self.X[idx]
        Fs, _, _ = self.propagate(X_rows, S=1, seed=int(seed))
        inputs = self._reselect_inputs(X_rows, Fs)
        new, report = {}, []
        for li in which:
            l, kern = self.layers[li], self._reselect_kernel(li)
            M = l.num_inducing
            cand = self.reselect_candidates(li, inputs[li], seed, candidates)
            if cand.shape[0] < M:
                raise ValueError("reselect_inducing: layer %d has %d candidates for M = %d" % (li, cand.shape[0], M))
            Z_old = np.ascontiguousarray(l.feature.Z, np.float64)
            Z_new, info = _k.greedy_variance(cand, M, kern, min_variance=min_variance, return_info=True)
            q_mu, q_sqrt = _k.transfer_inducing(Z_old, Z_new, kern, l.q_mu, l.q_sqrt, white=l.white, jitter=JITTER)
            A = solve_triangular(np.linalg.cholesky(kern._gram(Z_old, JITTER)), _k.cross_gram(Z_old, cand, kern), lower=True)
            kdiag = kern._gram(cand[:1], 0.0)[0, 0]      # the Gram matrix's own diagonal: a constant of the kernel
            new[li] = (Z_new, q_mu, q_sqrt)
            report.append({"layer": li, "rows": info["rows"], "n_greedy": int(info["n_greedy"]), "trace_new": float(info["trace"][-1]),
                           "trace_old": float(cand.shape[0] * kdiag - np.sum(A * A)), "kl_before": float(l.KL())})
        # nothing has been written so far: every selection and transfer went through
        for li, (Z_new, q_mu, q_sqrt) in new.items():
            l = self.layers[li]
            l.feature.Z, l.q_mu, l.q_sqrt = Z_new, q_mu, q_sqrt
            if li < n_layers - 1:
                l.Z_prior = np.array(Z_new, np.float64)
                l._build_prior_cholesky()
        self.sync_parameters()
        L, ctx = dev.lib(), self._ctx
        for key, li, name, shape in self._optimizer_groups():
            if li in new and name in ("Z", "q_mu", "q_sqrt") and key.startswith("layers/"):
                zero = np.zeros(shape, np.float64)
                ctx._check(L.dcgp_model_set_adam_state(self._model, li, name.encode(), zero.ctypes.data, zero.ctypes.data, zero.size))
        for entry in report:
            entry["kl_after"] = float(self.layers[entry["layer"]].KL())
        return report

    def propagate(self, X, full_cov=False, S=1, zs=None, seed=0):
        """(Fs, Fmeans, Fvars): per layer S x N x D_l arrays (doubly_stochastic_dgp DGP_Base.propagate); full_cov=True: see
        ``_propagate_full_cov`` (Fvars S x N x N x D_l)."""
        if full_cov:
            return self._propagate_full_cov(X, S, zs, seed)
        self._build()
        ctx, L = self._ctx, dev.lib()
        X = np.ascontiguousarray(np.reshape(X, (np.shape(X)[0], -1)), np.float64)
        N = X.shape[0]
        dX = ctx.to_device(X)
        # the device model was created with num_samples; propagate takes S explicitly
        arr, keep = self._z_table(zs, N, S)
        ctx._check(L.dcgp_model_set_keep_outputs(self._model, 1))
        info = C.c_int(0)
        try:
            rc = L.dcgp_model_propagate(self._model, dX.ptr, N, int(S), arr, int(seed), None, None, C.byref(info))
            ctx._check(rc, info)
            Fs, Fm, Fv = [], [], []
            for i, l in enumerate(self.layers):
                D = l.num_outputs
                bufs = [ctx.empty((S, N, D)) for _ in range(3)]
                rows, width = C.c_int(0), C.c_int(0)
                ctx._check(L.dcgp_model_layer_output(self._model, i, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, C.byref(rows), C.byref(width)))
                assert rows.value == S * N and width.value == D, (rows.value, width.value, S, N, D)
                Fs.append(bufs[0].numpy()), Fm.append(bufs[1].numpy()), Fv.append(bufs[2].numpy())
        finally:
            L.dcgp_model_set_keep_outputs(self._model, 0)
        return Fs, Fm, Fv

    def _propagate_full_cov(self, X, S, zs, seed):
        """DGP_Base.propagate(full_cov=True): every layer's conditional with full N x N covariances over the inputs, sampled with
        mean + chol(var + jitter I) z.  The parameters are first pulled from the device model, so the result describes what it holds.
        Hidden conv layers run their full-cov conditional (layer 0 once, tiled over the S identical copies of X); the head runs
        the image-pair K and the batched conditional, one call each for all S samples; the samples come from one
        dcgp_reparam_full_cov launch per layer.  Noise: ``zs[l]`` [S, N, D_l] where given, else np.random.default_rng(seed) --
        these draws cannot match the on-device draws the mean-field path makes for the same seed.  Rank-local."""
        for li, l in enumerate(self.layers[:-1]):
            if getattr(l, "mixing", None) is not None:
                raise NotImplementedError("full-covariance predictions through a mixed layer are not provided (layer %d has a mixing W %r)"
                                          % (li, np.shape(l.mixing)))
            if getattr(l.view, "dilation", 1) > 1:
                raise NotImplementedError("full-covariance predictions through a dilated layer are not provided (layer %d has dilation %d)"
                                          % (li, l.view.dilation))
        self.pull_parameters()
        from .layers import reparameterize_full_cov
        X = np.asarray(X, np.float64)
        X = np.ascontiguousarray(X.reshape(X.shape[0], int(np.prod(X.shape[1:]))))
        N, S = X.shape[0], int(S)
        rng = np.random.default_rng(seed)
        Fs, Fmeans, Fvars = [], [], []
        F = np.tile(X[None], [S, 1, 1])
        nl = len(self.layers)
        for li, layer in enumerate(self.layers):
            D = layer.num_outputs
            if N == 0:
                F = np.zeros((S, 0, D))
                Fs.append(F), Fmeans.append(np.zeros((S, 0, D))), Fvars.append(np.zeros((S, 0, 0, D)))
                continue
            head = li == nl - 1
            if li == 0:   # S identical copies of X
                if head:
                    m, v = layer._conditional_full_cov(X[None])
                    m, v = m[0], v[0]
                else:
                    m, v = layer.conditional_ND(X, full_cov=True)
                mean, var = np.tile(m[None], [S, 1, 1]), np.tile(v[None], [S, 1, 1, 1])
            elif head:
                mean, var = layer._conditional_full_cov(F)
            else:
                mv = [layer.conditional_ND(F[s_], full_cov=True) for s_ in range(S)]
                mean, var = np.stack([m for m, _ in mv]), np.stack([v for _, v in mv])
            z = zs[li] if zs is not None and zs[li] is not None else None
            z = rng.standard_normal((S, N, D)) if z is None else np.reshape(np.asarray(z, np.float64), (S, N, D))
            F = reparameterize_full_cov(mean, var, z)
            Fs.append(F), Fmeans.append(mean), Fvars.append(var)
        return Fs, Fmeans, Fvars

    def predict_f_full_cov(self, X, S, zs=None, seed=0):
        """(Fmean S x N x num_classes, Fvar S x N x N x num_classes) of the last layer (doubly_stochastic_dgp
        DGP_Base.predict_f_full_cov); noise as in ``propagate(full_cov=True)``.  Rank-local."""
        _, Fmeans, Fvars = self._propagate_full_cov(X, S, zs, seed)
        return Fmeans[-1], Fvars[-1]

    def predict_all_layers_full_cov(self, X, S, zs=None, seed=0):
        """(Fs, Fmeans, Fvars) of every layer with full covariances (doubly_stochastic_dgp DGP_Base.predict_all_layers_full_cov):
        what ``propagate(full_cov=True)`` returns.  Rank-local."""
        return self._propagate_full_cov(X, S, zs, seed)

    def _predict(self, X, S, zs, seed, want_samples, want_mean):
        self._build()
        ctx, L = self._ctx, dev.lib()
        X = np.ascontiguousarray(np.reshape(X, (np.shape(X)[0], -1)), np.float64)
        N, K = X.shape[0], self.layers[-1].num_outputs
        dX = ctx.to_device(X)
        arr, keep = self._z_table(zs, N, S)
        p = ctx.empty((S * N, K)) if want_samples else None
        pm = ctx.empty((N, K)) if want_mean else None
        info = C.c_int(0)
        rc = L.dcgp_model_predict_y(self._model, dX.ptr, N, int(S), arr, int(seed), p.ptr if p else None,
                                    pm.ptr if pm else None, C.byref(info))
        ctx._check(rc, info)
        return (p.numpy().reshape(S, N, K) if p else None), (pm.numpy() if pm else None)

    def predict_y(self, X, S, zs=None, seed=0):
        """(mean, var) of p(y*) per sample: S x N x num_classes (used at conv_gp/utils/log.py:62-66).
        One device call: forward pass and RobustMax quadrature, only the probabilities come back.  Gaussian likelihood:
        (Fmean, Fvar + variance), each S x N x D (dcgp_model_predict_mean_var); Bernoulli: (p, p - p^2) with
        p = probit(Fmean / sqrt(1 + Fvar)), each S x N x D; StudentT, Poisson: (E_y, V_y) of the 20-node rule, each S x N x D
        (StudentT: Fmean and Fvar + scale^2 nu / (nu - 2))."""
        if np.shape(X)[0] == 0:
            K = self.layers[-1].num_outputs
            return np.zeros((S, 0, K)), np.zeros((S, 0, K))
        if self.float_targets:
            return self._predict_mean_var(X, S, zs, seed)
        ps, _ = self._predict(X, S, zs, seed, True, False)
        return ps, ps - np.square(ps)

    def _predict_mean_var(self, X, S, zs, seed):
        self._build()
        ctx, L = self._ctx, dev.lib()
        X = np.ascontiguousarray(np.reshape(X, (np.shape(X)[0], -1)), np.float64)
        N, D = X.shape[0], self.layers[-1].num_outputs
        dX = ctx.to_device(X)
        arr, keep = self._z_table(zs, N, S)
        m, v = ctx.empty((S * N, D)), ctx.empty((S * N, D))
        info = C.c_int(0)
        ctx._check(L.dcgp_model_predict_mean_var(self._model, dX.ptr, N, int(S), arr, int(seed), m.ptr, v.ptr, C.byref(info)), info)
        return m.numpy().reshape(S, N, D), v.numpy().reshape(S, N, D)

    def predict_proba(self, X, S, zs=None, seed=0):
        """Class probabilities averaged over the S samples, N x num_classes (the quantity AccuracyLogger
        arg-maxes, conv_gp/utils/log.py:62-67); the sample mean is taken on the device.  Bernoulli likelihood: the sample-mean
        p(y = 1), N x D (the mean over S of ``predict_y``'s p, summed in sample order as ``evaluate`` sums it)."""
        if self.gaussian or self.student_t or self.poisson:
            raise ValueError("predict_proba: class probabilities need a classification likelihood, this model is %s" % self._lik_name())
        if np.shape(X)[0] == 0:
            return np.zeros((0, self.layers[-1].num_outputs))
        if self.bernoulli:
            return self._predict_mean_var(X, S, zs, seed)[0].mean(0)
        return self._predict(X, S, zs, seed, False, True)[1]

    def predict_f(self, X, S, zs=None, seed=0):
        """(Fmean, Fvar) of the last layer, each S x N x num_classes (doubly_stochastic_dgp DGP_Base.predict_f)."""
        _, Fmeans, Fvars = self.propagate(X, S=S, zs=zs, seed=seed)
        return Fmeans[-1], Fvars[-1]

    def predict_patch_contributions(self, X, S, zs=None, seed=0):
        """(C [S, N, P, R], Fmean [S, N, R]): the head's posterior mean of ``predict_f(X, S, zs, seed)`` split over the P patches of
        the head's input, C[s, n, p, r] = (w_p / P) sum_m k(z_m, h_sn[p]) beta[m, r] with C.sum(2) == Fmean -- per class, where in
        the image the evidence comes from (``layers[-1].kern.view.as_maps(C)`` makes images of it).  One device call
        (dcgp_model_patch_evidence): same samples as ``propagate`` for the same (S, zs, seed), any likelihood.  Rank-local."""
        head = self.layers[-1]
        if not hasattr(head.kern, "patch_mean"):
            raise TypeError("predict_patch_contributions needs a patch head (ConvKernel / AdditivePatchKernel); a dense head has no patches")
        bk = head.kern.base_kernel
        if not hasattr(bk, "lengthscales") or getattr(bk, "ARD", False):
            raise NotImplementedError("predict_patch_contributions needs a scalar-lengthscale RBF base kernel")
        S = int(S)
        if S < 1:
            raise ValueError("S must be >= 1")
        N, P, R = np.shape(X)[0], head.kern.patch_count, head.num_outputs
        if N == 0:
            return np.zeros((S, 0, P, R)), np.zeros((S, 0, R))
        X = np.ascontiguousarray(np.reshape(X, (N, -1)), np.float64)
        self._build()
        ctx, L = self._ctx, dev.lib()
        dX = ctx.to_device(X)
        arr, keep = self._z_table(zs, N, S)
        c, fm = ctx.empty((S, N, P, R)), ctx.empty((S, N, R))
        info = C.c_int(0)
        rc = L.dcgp_model_patch_evidence(self._model, dX.ptr, N, S, arr, int(seed), c.ptr, fm.ptr, C.byref(info))
        ctx._check(rc, info)
        return c.numpy(), fm.numpy()

    def predict_all_layers(self, X, S, zs=None, seed=0):
        """(Fs, Fmeans, Fvars) of every layer (doubly_stochastic_dgp DGP_Base.predict_all_layers): what ``propagate`` returns."""
        return self.propagate(X, S=S, zs=zs, seed=seed)

    def _out_dims(self):
        """Noise values per row and layer: one per output, for a mixed conv layer one per (patch, latent GP)."""
        return [getattr(l, "num_latent_outputs", l.num_outputs) for l in self.layers]

    # ---- test-time augmentation --------------------------------------------------------------------
    @contextlib.contextmanager
    def _eval_views(self, views, S, who, extra_slots=0):
        """The views of ONE evaluation call: checked on the host (ValueError before anything is launched), set on the device model
        (dcgp_model_set_eval_views) for the body and cleared behind it, also when the body raises -- the model keeps no view state.  Yields V,
        or None without views."""
        if views is None:
            yield None
            return
        H, W, Cc = self._image_geometry()          # (a dense head alone: ValueError, it has no images)
        v = _augment.check_views(views, H, W)
        V, K = int(v.shape[0]), self.layers[-1].num_outputs
        if not self.float_targets and int(S) * V * K + K + extra_slots > EVAL_MAX_SLOTS:
            raise ValueError("%s: S = %d samples of V = %d views of %d classes exceed the tail's LDS: S * V * K + K%s = %d > %d"
                             % (who, int(S), V, K, " + %d" % extra_slots if extra_slots else "", int(S) * V * K + K + extra_slots,
                                EVAL_MAX_SLOTS))
        self._build()
        L = dev.lib()

        def call(*args):
            try:
                self._ctx._check(L.dcgp_model_set_eval_views(self._model, *args))
            except dev.DcgpError as e:
                if e.code != dev.ERR_ARG:
                    raise
                raise ValueError(str(e)) from None

        call(H, W, Cc, V, v.ctypes.data)
        try:
            yield V
        finally:
            call(0, 0, 0, 0, None)

    def _eval_call(self, X, Y, S, batch_size, seed, flat_zs, want_p_mean, density_only=False):
        self._build()
        ctx, L = self._ctx, dev.lib()
        X = np.ascontiguousarray(np.reshape(X, (np.shape(X)[0], -1)), np.float64)
        N, K = X.shape[0], self.layers[-1].num_outputs
        if X.shape[1] != self.X.shape[1]:
            raise ValueError("images of %d values, the model takes %d" % (X.shape[1], self.X.shape[1]))
        if self.float_targets:
            return self._eval_call_f64y(X, self._targets_host(Y, N), S, batch_size, seed, flat_zs, want_p_mean, density_only)
        Y = np.ascontiguousarray(np.reshape(Y, (-1,)), np.int32)
        if Y.size != N:
            raise ValueError("%d labels for %d images" % (Y.size, N))
        dX, dY = ctx.to_device(X), ctx.to_device(Y, np.int32)     # the whole set crosses the bus once
        arr, keep = None, []
        if flat_zs is not None:
            arr = (C.c_void_p * len(self.layers))()
            for i, z in enumerate(flat_zs):
                if z is not None:
                    keep.append(ctx.to_device(z))
                    arr[i] = keep[-1].ptr
        ld = ctx.empty((N,))
        pm = ctx.empty((N, K)) if want_p_mean else None
        info = C.c_int(0)
        if density_only:
            rc = L.dcgp_model_predict_density(self._model, dX.ptr, dY.ptr, N, int(S), arr, int(seed), ld.ptr, C.byref(info))
            ctx._check(rc, info)
            return ld.numpy(), None, None
        out = (C.c_double * 2)()
        rc = L.dcgp_model_evaluate(self._model, dX.ptr, dY.ptr, N, int(batch_size), int(S), arr, int(seed), ld.ptr,
                                   pm.ptr if pm else None, out, C.byref(info))
        ctx._check(rc, info)
        return ld.numpy(), (pm.numpy() if pm else None), (out[0], out[1])

    def _eval_call_f64y(self, X, Y, S, batch_size, seed, flat_zs, want_y_mean, density_only):
        ctx, L = self._ctx, dev.lib()
        N, D = X.shape[0], self.layers[-1].num_outputs
        dX, dY = ctx.to_device(X), ctx.to_device(Y)
        arr, keep = None, []
        if flat_zs is not None:
            arr = (C.c_void_p * len(self.layers))()
            for i, z in enumerate(flat_zs):
                if z is not None:
                    keep.append(ctx.to_device(z))
                    arr[i] = keep[-1].ptr
        info = C.c_int(0)
        if density_only:
            ld = ctx.empty((N, D))
            ctx._check(L.dcgp_model_predict_density_f64y(self._model, dX.ptr, dY.ptr, N, int(S), arr, int(seed), ld.ptr, C.byref(info)), info)
            return ld.numpy(), None, None
        ld = ctx.empty((N,))
        ym = ctx.empty((N, D)) if want_y_mean else None
        out = (C.c_double * 2)()
        ctx._check(L.dcgp_model_evaluate_f64y(self._model, dX.ptr, dY.ptr, N, int(batch_size), int(S), arr, int(seed), ld.ptr,
                                              ym.ptr if ym else None, out, C.byref(info)), info)
        return ld.numpy(), (ym.numpy() if ym else None), (out[0], out[1])

    def predict_density(self, X, Y, S, zs=None, seed=0, views=None):
        """Log predictive density of each label, N x 1: logsumexp_s log p(y | f_s) - log S (doubly_stochastic_dgp
        DGP_Base.predict_density with the RobustMax likelihood).  Gaussian likelihood: N x D, per output
        logsumexp_s log N(y; Fmean_s, Fvar_s + variance) - log S; Bernoulli: N x D, per output logsumexp_s log p(y | p_s) - log S with
        p_s = probit(Fmean_s / sqrt(1 + Fvar_s)); StudentT, Poisson: N x D, per output logsumexp_s ld_s - log S with ld_s the 20-node
        log density of sample s.  One device call; ``zs`` per layer [S, N, D].  ``views`` [V, 3] (``augment.views``): test-time
        augmentation as in ``evaluate`` -- the logsumexp runs over the S V (sample, view) members, minus log(S V); ``zs`` is then
        [S, V, N, D] per layer."""
        N = np.shape(X)[0]
        if N == 0:
            return np.zeros((0, self.layers[-1].num_outputs if self.float_targets else 1))
        with self._eval_views(views, S, "predict_density") as V:
            ld, _, _ = self._eval_call(X, Y, S, N, seed, batched_noise(zs, N, S, N, self._out_dims(), V), False, density_only=True)
        return ld if self.float_targets else ld.reshape(N, 1)

    def evaluate(self, X, Y, S=5, batch_size=32, seed=0, zs=None, per_image=False, views=None):
        """A whole test set in one device call (dcgp_model_evaluate): batches of ``batch_size`` images, batch i drawing its noise
        from ``seed + i`` as ``AccuracyLogger`` does, or from ``zs`` (per layer [S, N, D], indexed by image over the whole set).
        Returns {"accuracy", "mean_log_density", "n"}, with ``per_image`` also "log_density" [N] and "p_mean" [N, K] (the
        sample-mean class probabilities).  Gaussian likelihood: {"mean_log_density", "rmse", "n"} (the root mean squared error of the
        sample-mean prediction over all N x D targets), with ``per_image`` also "log_density" [N] (summed over the D outputs) and
        "y_mean" [N, D].  Bernoulli likelihood: {"accuracy", "mean_log_density", "n"}, the accuracy over all N x D entries (an entry is
        correct when its label is 1 exactly where the sample-mean p > 0.5), with ``per_image`` also "log_density" [N] (summed over the
        D outputs) and "p_mean" [N, D] (the sample-mean p).  StudentT, Poisson: what a Gaussian model returns, "y_mean" the sample-mean
        E_y.  Rank-local: nothing is reduced across ranks.

        ``views``: test-time augmentation, an int array [V, 3] of (dy, dx, flip) (``augment.views``; None: the images as they are).  Every
        batch is then evaluated on the V shifted / mirrored views of its images (``augment.apply_views``, formed on the device) in the same
        call, and the predictive distribution of an image is the uniform mixture over the S samples AND the V views,
        p(y | x) = 1 / (S V) sum_{s, v} p(y | f_s(view_v(x))): "p_mean" / "y_mean" average over the S V members, "log_density" is the log of
        the mixture density (logsumexp over the members - log(S V) -- not the mean of per-view log densities), accuracy / rmse are those of
        the averaged prediction.  Batch i still draws from ``seed + i``, for its V n_i view images; ``zs`` per layer is [S, V, N, D], the
        noise of view v of image i.  The views hold for this call only: the model keeps no view state.  views=[(0, 0, 0)] is views=None, bit
        for bit.  ValueError before anything is launched: a table that is not [V, 3] or is empty, |dy| or |dx| >= min(H, W), a flip outside
        {0, 1}, a dense head alone (no images), S V K + K above the multi-class tails' 8192 LDS slots, ``zs`` of another size."""
        N = np.shape(X)[0]
        if int(batch_size) <= 0:
            raise ValueError("batch_size must be positive, got %r" % (batch_size,))
        if self.gaussian or self.student_t or self.poisson:
            D = self.layers[-1].num_outputs
            if N == 0:
                out = {"mean_log_density": float("nan"), "rmse": float("nan"), "n": 0}
                if per_image:
                    out["log_density"], out["y_mean"] = np.zeros(0), np.zeros((0, D))
                return out
            with self._eval_views(views, S, "evaluate") as V:
                ld, ym, (sq, total) = self._eval_call(X, Y, S, batch_size, seed,
                                                     batched_noise(zs, N, S, int(batch_size), self._out_dims(), V), per_image)
            out = {"mean_log_density": total / N, "rmse": float(np.sqrt(sq / (N * D))), "n": N}
            if per_image:
                out["log_density"], out["y_mean"] = ld, ym
            return out
        if N == 0:
            out = {"accuracy": 0.0, "mean_log_density": float("nan"), "n": 0}
            if per_image:
                out["log_density"], out["p_mean"] = np.zeros(0), np.zeros((0, self.layers[-1].num_outputs))
            return out
        with self._eval_views(views, S, "evaluate") as V:
            ld, pm, (correct, total) = self._eval_call(X, Y, S, batch_size, seed,
                                                     batched_noise(zs, N, S, int(batch_size), self._out_dims(), V), per_image)
        entries = N * self.layers[-1].num_outputs if self.bernoulli else N
        out = {"accuracy": correct / entries, "mean_log_density": total / N, "n": N}
        if per_image:
            out["log_density"], out["p_mean"] = ld, pm
        return out

    def _uncertainty_call(self, X, Y, S, batch_size, seed, flat_zs, bins, want_p_mean):
        """One dcgp_model_evaluate_uncertainty(_f64y) call; Y may be None.  Returns (host arrays by name, the [bins, 3] table, the
        seven dataset scalars)."""
        self._build()
        ctx, L = self._ctx, dev.lib()
        X = np.ascontiguousarray(np.reshape(X, (np.shape(X)[0], -1)), np.float64)
        N, K = X.shape[0], self.layers[-1].num_outputs
        if X.shape[1] != self.X.shape[1]:
            raise ValueError("images of %d values, the model takes %d" % (X.shape[1], self.X.shape[1]))
        dY = None
        if Y is not None and self.bernoulli:
            dY = ctx.to_device(self._targets_host(Y, N))
        elif Y is not None:
            Y = np.ascontiguousarray(np.reshape(Y, (-1,)), np.int32)
            if Y.size != N:
                raise ValueError("%d labels for %d images" % (Y.size, N))
            dY = ctx.to_device(Y, np.int32)
        dX = ctx.to_device(X)                                       # the whole set crosses the bus once
        arr, keep = None, []
        if flat_zs is not None:
            arr = (C.c_void_p * len(self.layers))()
            for i, z in enumerate(flat_zs):
                if z is not None:
                    keep.append(ctx.to_device(z))
                    arr[i] = keep[-1].ptr
        per = (N, K) if self.bernoulli else (N,)
        bufs = {"log_density": ctx.empty((N,)) if dY is not None else None, "p_mean": ctx.empty((N, K)) if want_p_mean else None}
        for name in ("predictive_entropy", "expected_entropy", "mutual_information", "confidence"):
            bufs[name] = ctx.empty(per)
        bufs["prediction"] = ctx.empty(per, np.int32)
        table = ctx.empty((int(bins), 3))
        out, info = (C.c_double * 7)(), C.c_int(0)
        fn = L.dcgp_model_evaluate_uncertainty_f64y if self.bernoulli else L.dcgp_model_evaluate_uncertainty
        ptr = lambda a: a.ptr if a is not None else None            # noqa: E731
        rc = fn(self._model, dX.ptr, ptr(dY), N, int(batch_size), int(S), arr, int(seed), int(bins), ptr(bufs["log_density"]),
                ptr(bufs["p_mean"]), bufs["predictive_entropy"].ptr, bufs["expected_entropy"].ptr, bufs["mutual_information"].ptr,
                bufs["confidence"].ptr, bufs["prediction"].ptr, table.ptr, out, C.byref(info))
        ctx._check(rc, info)
        return {k: v.numpy() for k, v in bufs.items() if v is not None}, table.numpy(), list(out)

    _UNCERTAINTY_KEYS = ("predictive_entropy", "expected_entropy", "mutual_information", "confidence", "prediction")

    def _uncertainty_empty(self):
        per = (0, self.layers[-1].num_outputs) if self.bernoulli else (0,)
        out = {k: np.zeros(per) for k in self._UNCERTAINTY_KEYS[:4]}
        out["prediction"] = np.zeros(per, np.int32)
        return out

    def evaluate_uncertainty(self, X, Y, S=5, batch_size=32, seed=0, zs=None, bins=15, per_image=False, views=None):
        """``evaluate`` with the uncertainty of the predictions kept, still one device call (dcgp_model_evaluate_uncertainty): everything
        ``evaluate`` returns for the same arguments, bit for bit, plus -- in nats, from the S per-sample probabilities p_s and their mean
        pbar -- "mean_predictive_entropy" (the mean of H(pbar)), "mean_mutual_information" (BALD: H(pbar) - 1/S sum_s H(p_s), the part
        of the uncertainty that comes from the model), the calibration of the confidence max_k pbar[k] over ``bins`` equal-width bins
        ("ece", "mce", and "reliability": {"count", "confidence", "accuracy"} per bin, NaN where a bin is empty) and the "brier" score.
        With ``per_image`` also "predictive_entropy", "expected_entropy", "mutual_information", "confidence" and "prediction" per image.
        Bernoulli likelihood: every (image, output) entry counts, with the binary entropy, confidence max(pbar, 1 - pbar) and prediction
        pbar > 0.5; the per-image arrays are N x D.  A Gaussian model has no class probabilities: ValueError.  Rank-local.

        ``views`` (``augment.views``): test-time augmentation exactly as in ``evaluate`` -- the members p_s become the S V probabilities
        p_{s,v} of sample s on view v, pbar their mean.  The expected entropy averages H(p_{s,v}) over the S V members, so the mutual
        information (BALD) then counts disagreement BETWEEN VIEWS of an image as model uncertainty, together with the disagreement between
        samples: it is the uncertainty of the augmented predictor, not of the model on the image as it is.  ``zs`` per layer [S, V, N, D];
        the multi-class limit is S V K + K + 48 <= 8192."""
        if self.gaussian or self.student_t or self.poisson:
            raise ValueError("evaluate_uncertainty: class probabilities need a classification likelihood, this model is %s" % self._lik_name())
        N = np.shape(X)[0]
        if int(batch_size) <= 0:
            raise ValueError("batch_size must be positive, got %r" % (batch_size,))
        bins = int(bins)
        nan = float("nan")
        if N == 0:
            out = self.evaluate(X, Y, S=S, batch_size=batch_size, seed=seed, zs=zs, per_image=per_image)       # (no image, no view)
            out.update(ece=nan, mce=nan, brier=nan, mean_predictive_entropy=nan, mean_mutual_information=nan,
                       reliability={"count": np.zeros(max(bins, 0), np.int64), "confidence": np.full(max(bins, 0), nan),
                                    "accuracy": np.full(max(bins, 0), nan)})
            if per_image:
                out.update(self._uncertainty_empty())
            return out
        with self._eval_views(views, S, "evaluate_uncertainty", UNC_EXTRA_SLOTS) as V:
            arrs, table, h = self._uncertainty_call(X, Y, S, batch_size, seed,
                                                    batched_noise(zs, N, S, int(batch_size), self._out_dims(), V), bins, per_image)
        entries = N * self.layers[-1].num_outputs if self.bernoulli else N
        out = {"accuracy": h[0] / entries, "mean_log_density": h[1] / N, "n": N, "ece": h[2], "mce": h[3], "brier": h[4],
               "mean_predictive_entropy": h[5], "mean_mutual_information": h[6]}
        count = table[:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            out["reliability"] = {"count": count.astype(np.int64), "confidence": np.where(count > 0, table[:, 1] / count, nan),
                                  "accuracy": np.where(count > 0, table[:, 2] / count, nan)}
        if per_image:
            out.update(arrs)
        return out

    def predict_uncertainty(self, X, S, zs=None, seed=0, batch_size=None, views=None):
        """The per-image uncertainty of unlabelled images (acquisition functions, out-of-distribution scores), one device call:
        {"p_mean", "predictive_entropy", "expected_entropy", "mutual_information", "confidence", "prediction"} as
        ``evaluate_uncertainty(per_image=True)`` returns them.  ``batch_size`` None: one batch of all N images (``predict_proba``'s
        samples for the same ``seed`` / ``zs``); otherwise batch i draws from ``seed + i``.  Rank-local.  ``views``: test-time augmentation
        as in ``evaluate_uncertainty`` (S V members per image; the mutual information includes the disagreement between views)."""
        if self.gaussian or self.student_t or self.poisson:
            raise ValueError("predict_uncertainty: class probabilities need a classification likelihood, this model is %s" % self._lik_name())
        N = np.shape(X)[0]
        if N == 0:
            out = self._uncertainty_empty()
            out["p_mean"] = np.zeros((0, self.layers[-1].num_outputs))
            return out
        bs = N if batch_size is None else int(batch_size)
        if bs <= 0:
            raise ValueError("batch_size must be positive, got %r" % (batch_size,))
        with self._eval_views(views, S, "predict_uncertainty", UNC_EXTRA_SLOTS) as V:
            arrs, _, _ = self._uncertainty_call(X, None, S, bs, seed, batched_noise(zs, N, S, bs, self._out_dims(), V), 1, True)
        return arrs

    def KL(self):
        return float(sum(l.KL() for l in self.layers))

    def close(self):
        if self._model is not None:
            dev.lib().dcgp_model_destroy(self._model)
            self._model = None
            self._dataset = None      # (the resident training set went with the device model)
