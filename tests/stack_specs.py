"""Test helper: the one builder of live model specs for stacks with padding, stride and dilation (tests/padding_ref.py,
tests/dilation_ref.py, tests/conv_mean_ref.py, tests/mixing_ref.py, tests/compose_cases.py and their tests).

A conv entry is ``(f, s, R, pad, dil)``, the head ``(f, s, pad)``.  A spec entry carries ``pad`` and ``dil`` next to its UNPADDED ``H``, ``W`` --
the form ``ModelBuilder.spec()`` writes and ``build_layers_from_spec`` reads.  ``stack_spec`` draws live parameters by tests/live_specs.py's
recipe, per layer on the geometry the sliding window sees: the inducing patches of a layer are cut from images of its PHASE size (at
dilation 1 the padded size), whose ordinary patches are the dilated windows of the padded image.  Dilation above 1 takes stride 1.  Test
infrastructure only."""
import numpy as np

import live_specs as ls


def out_size(H, W, f, s, p, d=1):
    span = d * (f - 1) + 1
    return (H + 2 * p - span) // s + 1, (W + 2 * p - span) // s + 1


def phase_size(H, W, p, d):
    return -(-(H + 2 * p) // d), -(-(W + 2 * p) // d)


def chain(hwc, convs, head):
    """convs [(f, s, R, pad, dil)], head (f, s, pad) -> ([(H, W, C) entering each layer, unpadded, the head last], head patch count)."""
    H, W, C = hwc
    sizes = []
    for f, s, R, p, d in convs:
        assert d == 1 or s == 1, (s, d)
        sizes.append((H, W, C))
        H, W = out_size(H, W, f, s, p, d)
        C = R
    sizes.append((H, W, C))
    ho, wo = out_size(H, W, head[0], head[1], head[2])
    return sizes, ho * wo


def stack_spec(hwc, convs, head, Ms, S=2, seed=7, whites=None, c=1.0, a=0.1, num_data=60000, additive=False, conv2d_mean=()):
    """convs [(f, s, R, pad, dil)], head (f, s, pad); Ms one count per layer (or one int); conv2d_mean: indices of the conv layers with
    Conv2dMean."""
    nl = len(convs) + 1
    Ms = [Ms] * nl if np.ndim(Ms) == 0 else list(Ms)
    whites = [False] * nl if whites is None else list(whites)
    sizes, _ = chain(hwc, convs, head)
    spec = {"S": int(S), "num_data": int(num_data), "convs": []}
    for li, (f, s, R, p, d) in enumerate(convs):
        H, W, C = sizes[li]
        Hs, Ws = phase_size(H, W, p, d)
        one = ls.live_spec((Hs, Ws, C), [(f, s, R)], (1, 1), Ms[li], c, a, S=S, seed=seed + li, white=whites[li], num_data=num_data)
        layer = one["convs"][0]
        layer.update(H=H, W=W, pad=p, dil=d)
        if li in conv2d_mean:
            layer["mean_function"] = "conv2d"
        spec["convs"].append(layer)
    f, s, p = head
    H, W, C = sizes[-1]
    one = ls.live_spec((H + 2 * p, W + 2 * p, C), [], (f, s), Ms[-1], c, a, S=S, seed=seed + nl, white=whites[-1], num_data=num_data)
    h = one["head"]
    h.update(H=H, W=W, pad=p)
    if additive:
        h["kernel"] = "add"
    spec["head"] = h
    return spec


def output_dims(spec):
    """Per layer (noise values, outputs) a row: P * (the layer's GPs), P * (its feature maps); they differ on a mixed layer."""
    dims = []
    for c in spec["convs"]:
        ho, wo = out_size(c["H"], c["W"], c["f"], c["s"], c.get("pad", 0), c.get("dil", 1))
        Rout = c["R"] if c.get("mix_W") is None else np.shape(c["mix_W"])[1]
        dims.append((ho * wo * c["R"], ho * wo * Rout))
    return dims + [(spec["head"]["R"], spec["head"]["R"])]


def make_noise(spec, N, seed=7):
    """Per layer [S, N, P * (the layer's GPs)] in image order."""
    rng = np.random.default_rng(20_000 + seed)
    return [rng.standard_normal((spec["S"], N, d)) for d, _ in output_dims(spec)]
