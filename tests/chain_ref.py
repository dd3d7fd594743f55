"""Reference of the factorisation chain (csrc/chol_fused.hip) in plain NumPy / SciPy float64: the factor, its inverse, the right-hand sides that ride the chain
and their sums of squares in the layout documented at ChainRhs in csrc/common.h."""
import numpy as np
import scipy.linalg


def n_panels(Mp):
    return (Mp + 31) // 32


def n_slots(Mp):
    return n_panels(Mp) * (n_panels(Mp) + 1) // 2


def block_sums(G, alpha, R, Mp, dtype=np.float64):
    """sums [R + 1][ns] and the mask of the slots that exist: row r < R, slot p (p + 1) / 2 + ct = the sum of squares of the 32 x 32 block (rows of panel p,
    column tile ct <= p) of G_r; row R, slot p = that of panel p's rows of alpha (np slots; the rest of the row is unused).  G / alpha None: that part is left
    out of the mask."""
    np_, ns = n_panels(Mp), n_slots(Mp)
    sums = np.full((R + 1, ns), np.nan)
    mask = np.zeros((R + 1, ns), bool)
    for p in range(np_):
        rows = slice(32 * p, min(32 * p + 32, Mp))
        if G is not None:
            for ct in range(p + 1):
                blk = G[:, rows, 32 * ct:32 * ct + 32].astype(dtype)
                sums[:R, p * (p + 1) // 2 + ct] = (blk * blk).sum(axis=(1, 2)).astype(np.float64)
                mask[:R, p * (p + 1) // 2 + ct] = True
        if alpha is not None:
            blk = alpha[rows].astype(dtype)
            sums[R, p] = float((blk * blk).sum())
            mask[R, p] = True
    return sums, mask


def reference(inp):
    """of the inputs of chain_cases.build(): L, Linv [batch][Mp][Mp]; per entry G [R][Mp][Mp], alpha [Mp][Rp], sums and their mask (None where nothing rides)"""
    Mp, nb = inp["Mp"], len(inp["ents"])
    eye = np.eye(Mp)
    L = np.stack([np.linalg.cholesky(inp["A"][b]) for b in range(nb)])
    Linv = np.stack([scipy.linalg.solve_triangular(L[b], eye, lower=True) for b in range(nb)])
    G, alpha, sums, mask = [], [], [], []
    for b, e in enumerate(inp["ents"]):
        g = np.stack([scipy.linalg.solve_triangular(L[b], inp["Lq"][b][r], lower=True) for r in range(e["R"])]) if e["Lq"] else None
        a = scipy.linalg.solve_triangular(L[b], inp["qmu"][b], lower=True) if e["qmu"] else None
        s, m = block_sums(g, a, e["R"], Mp) if (e["Lq"] or e["qmu"]) else (None, None)
        G.append(g); alpha.append(a); sums.append(s); mask.append(m)
    return dict(L=L, Linv=Linv, G=G, alpha=alpha, sums=sums, mask=mask)
