"""Test helper: predictive uncertainty and calibration in plain NumPy, written from their definitions (nats, natural log).

    ps [S, N, K] per-sample class probabilities (Bernoulli: [S, N, D] per-sample p(y = 1)), pbar = (1/S) sum_s ps[s] in sample order
    predictive_entropy  = -sum_k pbar[k] log pbar[k]                      (Bernoulli: h(pbar), h(q) = -q log q - (1 - q) log(1 - q))
    expected_entropy    = (1/S) sum_s -sum_k ps[s][k] log ps[s][k]
    mutual_information  = predictive_entropy - expected_entropy           (BALD; the raw difference)
    confidence          = max_k pbar[k]                                   (Bernoulli: max(pbar, 1 - pbar))
    prediction          = first index of the maximum                      (Bernoulli: pbar > 0.5)
    bin b               = min(B - 1, floor(confidence * B));  per bin count, sum_confidence, sum_correct
    ece                 = sum_b (count_b / n) |sum_correct_b - sum_confidence_b| / count_b over non-empty bins, mce the largest gap
    brier               = (1/n) sum_i sum_k (pbar[i][k] - [y_i = k])^2    (Bernoulli: (pbar - y)^2 per entry)
No clamping: the probabilities the likelihoods produce are bounded away from 0 and 1."""
import numpy as np


def sample_mean(ps):
    ps = np.asarray(ps, np.float64)
    acc = np.zeros(ps.shape[1:])
    for s in range(ps.shape[0]):
        acc = acc + ps[s]
    return acc / ps.shape[0]


def multiclass(ps):
    ps = np.asarray(ps, np.float64)
    pbar = sample_mean(ps)
    h = -np.sum(pbar * np.log(pbar), axis=-1)
    e = np.mean(-np.sum(ps * np.log(ps), axis=-1), axis=0)
    return {"p_mean": pbar, "predictive_entropy": h, "expected_entropy": e, "mutual_information": h - e,
            "confidence": pbar.max(axis=-1), "prediction": pbar.argmax(axis=-1)}


def binary_entropy(q):
    return -q * np.log(q) - (1 - q) * np.log(1 - q)


def bernoulli(ps):
    ps = np.asarray(ps, np.float64)
    pbar = sample_mean(ps)
    h, e = binary_entropy(pbar), np.mean(binary_entropy(ps), axis=0)
    return {"p_mean": pbar, "predictive_entropy": h, "expected_entropy": e, "mutual_information": h - e,
            "confidence": np.maximum(pbar, 1 - pbar), "prediction": (pbar > 0.5).astype(np.int64)}


def bin_table(confidence, correct, bins):
    """[bins, 3] = {count, sum_confidence, sum_correct} over the flattened entries."""
    confidence, correct = np.ravel(confidence), np.ravel(correct).astype(np.float64)
    b = np.minimum(bins - 1, np.floor(confidence * bins).astype(np.int64))
    table = np.zeros((bins, 3))
    for j in range(bins):
        sel = b == j
        table[j] = sel.sum(), confidence[sel].sum(), correct[sel].sum()
    return table


def ece_mce(table):
    n = table[:, 0].sum()
    ece, mce = 0.0, 0.0
    for count, sum_conf, sum_correct in table:
        if count == 0:
            continue
        gap = abs(sum_correct - sum_conf) / count
        ece += (count / n) * gap
        mce = max(mce, gap)
    return ece, mce


def calibration(pbar, Y, bins, bernoulli_targets=False):
    """The dataset quantities from the sample-mean probabilities and the labels (MultiClass: Y [N] integers; Bernoulli: Y [N, D], 1 = positive)."""
    pbar = np.asarray(pbar, np.float64)
    if bernoulli_targets:
        pos = np.asarray(Y).reshape(pbar.shape) == 1
        conf, pred = np.maximum(pbar, 1 - pbar), pbar > 0.5
        correct = pred == pos
        brier = np.mean((pbar - pos.astype(np.float64)) ** 2)
    else:
        Y = np.reshape(Y, (-1,))
        conf, pred = pbar.max(axis=-1), pbar.argmax(axis=-1)
        correct = pred == Y
        onehot = np.zeros_like(pbar)
        onehot[np.arange(len(Y)), Y] = 1.0
        brier = np.sum((pbar - onehot) ** 2) / len(Y)
    table = bin_table(conf, correct, bins)
    ece, mce = ece_mce(table)
    return {"table": table, "ece": ece, "mce": mce, "brier": float(brier), "accuracy": float(np.mean(correct)),
            "confidence": conf, "prediction": pred.astype(np.int64), "correct": correct}


def near_a_decision(pbar, bins, tol=1e-9, bernoulli_targets=False):
    """Entries whose bin or prediction a perturbation of pbar below `tol` could change: the confidence within tol of a bin edge, or the
    two largest probabilities within tol of each other (Bernoulli: pbar within tol of 1/2)."""
    pbar = np.asarray(pbar, np.float64)
    if bernoulli_targets:
        conf, tie = np.maximum(pbar, 1 - pbar), np.abs(pbar - 0.5) <= tol
    else:
        top = np.sort(pbar, axis=-1)
        conf, tie = top[..., -1], top[..., -1] - top[..., -2] <= tol
    scaled = conf * bins
    return tie | (np.abs(scaled - np.round(scaled)) <= tol * bins)
