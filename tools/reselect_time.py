#!/usr/bin/env python
"""usage (GPU box): python tools/reselect_time.py [--rounds 3] [--adam-steps 200] [--images 1000] [--out profiles/reselect_time.json]

What a re-selection of the inducing patches during training (``DGP_Base.reselect_inducing``: csrc/greedy.hip + csrc/transfer.hip) costs and what
it does, on cfg2's conv + head model (28 x 28 x 1 synthetic images of deepcgp_amd.synthetic, conv f5 s2 into head f5, M = 256, variance =
lengthscale = 5, 512 training images) started from the k-means initialisation and trained for ``--adam-steps`` Adam steps (lr 1e-3).

Cost: one ``reselect_inducing(images=--images)`` by the host clock, and its pieces timed one by one on the same model state -- the
propagation, the candidate draw (host gather), the selection (dcgp_greedy_variance, both layers) and the transfer (dcgp_inducing_transfer,
both layers); the rest is the diagnostics (the old Z's Nystrom trace: dcgp_cross_gram and a host solve), the parameter push and the KL terms.
Beside them one period's ``train_run`` of ``--adam-steps`` steps, measured in the same session.  Medians over ``--rounds`` rounds.

Effect, per layer: the candidates' Nystrom trace under the old and the new Z, cond(K_uu + jitter I) before and after, the layer's KL term before
and after.  And the ELBO of one fixed batch (fixed device draws) before the re-selection, right after it, and after ``--adam-steps`` more
steps, each with its data term -- in alternating rounds with and without the re-selection, both arms from the same parameters and optimiser state, on the same
minibatches and seeds (round r: its own re-selection seed and its own minibatches).

No figure is fixed in advance; the case where the re-selection does not help is reported as it comes out.  Prints one JSON line."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_TRAIN, BATCH, LR = 512, 32, 1e-3


def images(n):
    from deepcgp_amd import synthetic as syn
    return syn._blur_images(np.random.default_rng(1235), n, 28, 28, 1)


def start_spec():
    """cfg2 C + H with the k-means initialisation of both layers (the reference's recipe, as tools/inducing_init_time.py builds it)."""
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.kernels import JITTER, RBF, _cluster_patches
    spec, _, _ = syn.make_config("cfg2_mnist_CH_M256")
    c0, h0 = spec["convs"][0], spec["head"]
    imgs = images(N_TRAIN)
    feats = syn._identity_conv(imgs, c0["f"], c0["R"], c0["s"])
    for li, (src, lay, scale) in enumerate(((imgs, c0, 1e-5), (feats, h0, 1.0))):
        np.random.seed(100 + li)
        Z = _cluster_patches(src, lay["M"], lay["f"])
        lay["Z"] = Z
        if "Z0" in lay:
            lay["Z0"] = Z.copy()
        Lu = np.linalg.cholesky(RBF(Z.shape[1], lay["variance"], lay["ls"])._gram(Z, JITTER))
        lay["q_sqrt"] = np.tile(Lu[None], [lay["q_sqrt"].shape[0], 1, 1]) * scale
    spec["num_data"] = N_TRAIN
    return spec, imgs.reshape(N_TRAIN, -1), np.random.default_rng(7).integers(0, 10, size=N_TRAIN).astype(np.int32)


def snapshot(spec, model):
    """(spec holding the model's parameters and prior patches, its optimiser state): what an identical copy is built from."""
    model.pull_parameters()
    out = copy.deepcopy(spec)
    for c, l in zip(out["convs"] + [out["head"]], model.layers):
        head = c is out["head"]
        kern = l.kern.base_kernel if head else l.base_kernel
        c["Z"], c["q_mu"], c["q_sqrt"] = np.array(l.feature.Z), np.array(l.q_mu), np.array(l.q_sqrt)
        c["variance"], c["ls"] = float(kern.variance), float(kern.lengthscales)
        if head:
            c["w"] = np.array(l.kern.patch_weights)
        else:
            c["Z0"] = np.array(l.Z_prior)
    return out, model.optimizer_state()


def copy_of(snap, X, Y):
    from deepcgp_amd.models import build_from_spec
    model = build_from_spec(copy.deepcopy(snap[0]), X, Y)
    model.set_optimizer_state(snap[1])
    model.dedup_layer0 = True
    model.attach_dataset()
    return model


def steps(model, n, seed):
    idx = np.stack([np.random.default_rng(seed + t).choice(N_TRAIN, BATCH, replace=False) for t in range(n)])
    t0 = time.perf_counter()
    model.train_run(idx, LR, seed=seed)
    return 1e3 * (time.perf_counter() - t0)


def elbo(model, fixed, res, tag):
    """ELBO of the fixed batch under fixed device draws, with its data term (the KL is their difference)."""
    e, d, _ = model.compute_log_likelihood(*fixed, seed=1, return_parts=True)
    res["elbo_" + tag], res["data_term_" + tag] = float(e), float(d)


def conds(model):
    from deepcgp_amd.kernels import JITTER
    out = []
    for li, l in enumerate(model.layers):
        out.append(float(np.linalg.cond(model._reselect_kernel(li)._gram(l.feature.Z, JITTER))))
    return out


def pieces(model, n_images, seed):
    """The pieces of one re-selection, timed one by one on the model as it stands (nothing is written)."""
    from deepcgp_amd import kernels as k
    t = {}
    t0 = time.perf_counter()
    model.pull_parameters()
    idx = model._reselect_rng(seed, 0).choice(N_TRAIN, size=min(n_images, N_TRAIN), replace=False)
    Fs, _, _ = model.propagate(model.X[idx], S=1, seed=seed)
    t["propagate_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    inputs = model._reselect_inputs(model.X[idx], Fs)
    cands = [model.reselect_candidates(li, inputs[li], seed) for li in range(len(model.layers))]
    t["candidates_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    Zs = [k.greedy_variance(c, l.num_inducing, model._reselect_kernel(li)) for li, (c, l) in enumerate(zip(cands, model.layers))]
    t["selection_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    for li, (Z, l) in enumerate(zip(Zs, model.layers)):
        k.transfer_inducing(l.feature.Z, Z, model._reselect_kernel(li), l.q_mu, l.q_sqrt, white=l.white)
    t["transfer_ms"] = 1e3 * (time.perf_counter() - t0)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--adam-steps", type=int, default=200)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from deepcgp_amd.models import build_from_spec
    spec, X, Y = start_spec()
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = True
    model.attach_dataset()
    steps(model, a.adam_steps, 1000)
    snap = snapshot(spec, model)
    model.close()
    fixed = (X[:BATCH], Y[:BATCH])
    out = {"M": 256, "adam_steps": a.adam_steps, "lr": LR, "images": min(a.images, N_TRAIN), "train_images": N_TRAIN, "rounds": []}
    for r in range(a.rounds + 1):                # round 0: warm-up, not reported
        entry = {"seed": r}
        for arm in (("with", "without") if r % 2 else ("without", "with")):
            m = copy_of(snap, X, Y)
            res = {}
            elbo(m, fixed, res, "before")
            if arm == "with":
                res["cond_before"] = conds(m)
                res["pieces"] = pieces(m, a.images, 5000 + r)
                t0 = time.perf_counter()
                report = m.reselect_inducing(images=a.images, seed=5000 + r)
                res["reselect_ms"] = 1e3 * (time.perf_counter() - t0)
                res["cond_after"] = conds(m)
                res["layers"] = [{k: v for k, v in rep.items() if k != "rows"} for rep in report]
                elbo(m, fixed, res, "right_after")
            res["train_run_ms"] = steps(m, a.adam_steps, 2000 + 1000 * r)
            elbo(m, fixed, res, "after")
            m.close()
            entry[arm] = res
        if r:
            out["rounds"].append(entry)
    med = lambda xs: float(np.median(xs))
    w = [e["with"] for e in out["rounds"]]
    out["summary"] = {
        "reselect_ms": med([x["reselect_ms"] for x in w]),
        "pieces_ms": {k: med([x["pieces"][k] for x in w]) for k in w[0]["pieces"]},
        "train_run_ms": med([e[arm]["train_run_ms"] for e in out["rounds"] for arm in ("with", "without")]),
        "elbo_after_with_minus_without": [e["with"]["elbo_after"] - e["without"]["elbo_after"] for e in out["rounds"]],
        "elbo_right_after_minus_before": [e["with"]["elbo_right_after"] - e["with"]["elbo_before"] for e in out["rounds"]],
        "data_term_after_with_minus_without": [e["with"]["data_term_after"] - e["without"]["data_term_after"] for e in out["rounds"]],
        "data_term_right_after_minus_before": [e["with"]["data_term_right_after"] - e["with"]["data_term_before"] for e in out["rounds"]],
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
