"""Re-selection of the inducing inputs without a GPU: the transfer's two guarantees on the NumPy mirror (tests/reselect_ref.py) -- every new
covariance stays away from singular, and the KL to the prior never rises --, the flags and their parser, the driver's schedule against a recorder
model, and the independence of the candidate draws from the global generator."""
import argparse
import os

import numpy as np
import pytest

import reselect_ref as rr
from deepcgp_amd import device as dev
from deepcgp_amd import utils
from deepcgp_amd.arguments import FLAGS, default_parser, parse_reselect, reselect_due
from deepcgp_amd.dgp import DGP_Base
from deepcgp_amd.experiment import Experiment, read_args

JITTER = 1e-3
KERNEL_ARGS = {
    "rbf": dict(kind="rbf", variance=5.0, p1=3.0, p2=0.0, ard=None),
    "rbf_ard": dict(kind="rbf", variance=5.0, p1=1.0, p2=0.0, ard=np.linspace(2.0, 4.5, 9)),
    "acos": dict(kind="acos", variance=5.0, p1=1.0, p2=1.0, ard=None),
    "matern32": dict(kind="matern32", variance=5.0, p1=3.0, p2=0.0, ard=None),
    "matern52": dict(kind="matern52", variance=5.0, p1=3.0, p2=0.0, ard=None),
}


def inputs(M, Mn, shared, seed):
    rng = np.random.default_rng(seed)
    Z, Zn = rng.standard_normal((M, 9)), rng.standard_normal((Mn, 9))
    Zn[:shared] = Z[:shared]
    return rng, Z, Zn


# ---- the mirror: S' stays positive definite --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", sorted(KERNEL_ARGS))
@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e-5])
@pytest.mark.parametrize("shared", [0, 4])
def test_new_covariance_keeps_half_the_jitter(kern, scale, shared):
    """u and u' carry independent jitter: Kn - B^T B is the conditional covariance of u' given u in a joint prior that is positive definite with
    smallest eigenvalue >= jitter, so every S'_r has its smallest eigenvalue >= jitter / 2 -- however small q_sqrt is, and also where Z' shares
    rows with Z."""
    rng, Z, Zn = inputs(24, 24, shared, 5)
    q_mu, q_sqrt = rr.random_q(rng, 24, 3, scale)
    for white in (False, True):
        _, S, _, _ = rr.new_covariances(Z, Zn, jitter=JITTER, q_mu=q_mu, q_sqrt=q_sqrt, white=white, **KERNEL_ARGS[kern])
        smallest = min(np.linalg.eigvalsh(S[r]).min() for r in range(3))
        print(kern, scale, shared, white, "smallest eigenvalue %.3e" % smallest)
        assert smallest >= JITTER / 2
        mu, Ls = rr.transfer(Z, Zn, jitter=JITTER, q_mu=q_mu, q_sqrt=q_sqrt, white=white, **KERNEL_ARGS[kern])
        assert np.all(np.isfinite(mu)) and np.all(np.isfinite(Ls)) and np.all(np.diagonal(Ls, axis1=1, axis2=2) > 0)


def test_same_z_is_a_projection_not_the_identity():
    rng, Z, _ = inputs(24, 24, 0, 6)
    q_mu, q_sqrt = rr.random_q(rng, 24, 2)
    mu, Ls = rr.transfer(Z, Z.copy(), jitter=JITTER, q_mu=q_mu, q_sqrt=q_sqrt, **KERNEL_ARGS["rbf"])
    assert np.abs(mu - q_mu).max() > 1e-6          # documented: the two sets carry independent jitter
    K = rr.gram(Z, jitter=JITTER, **KERNEL_ARGS["rbf"])
    assert rr.gauss_kl(mu, Ls, K) <= rr.gauss_kl(q_mu, q_sqrt, K)


# ---- the mirror: data processing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", sorted(KERNEL_ARGS))
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("M,Mn", [(24, 16), (24, 24), (16, 40)])
def test_kl_never_rises(kern, white, M, Mn):
    """KL[q' || N(0, Kn)] <= KL[q || N(0, K)]: q' and the new prior are q and the old prior pushed through the same conditional p(u' | u)."""
    rng, Z, Zn = inputs(M, Mn, 2, 7)
    q_mu, q_sqrt = rr.random_q(rng, M, 3)
    kw = KERNEL_ARGS[kern]
    mu, Ls = rr.transfer(Z, Zn, jitter=JITTER, q_mu=q_mu, q_sqrt=q_sqrt, white=white, **kw)
    if white:
        before, after = rr.gauss_kl(q_mu, q_sqrt), rr.gauss_kl(mu, Ls)
    else:
        before, after = rr.gauss_kl(q_mu, q_sqrt, rr.gram(Z, jitter=JITTER, **kw)), rr.gauss_kl(mu, Ls, rr.gram(Zn, jitter=JITTER, **kw))
    print(kern, white, M, Mn, "KL %.9g -> %.9g" % (before, after))
    assert after <= before * (1 + 1e-12)


def test_white_is_the_unwhitened_transfer_in_other_coordinates():
    rng, Z, Zn = inputs(24, 16, 2, 8)
    m_w, Lq_w = rr.random_q(rng, 24, 2)
    kw = KERNEL_ARGS["matern52"]
    L, Ln = np.linalg.cholesky(rr.gram(Z, jitter=JITTER, **kw)), np.linalg.cholesky(rr.gram(Zn, jitter=JITTER, **kw))
    mu_w, Ls_w = rr.transfer(Z, Zn, jitter=JITTER, q_mu=m_w, q_sqrt=Lq_w, white=True, **kw)
    mu_u, Ls_u = rr.transfer(Z, Zn, jitter=JITTER, q_mu=L @ m_w, q_sqrt=np.einsum("ij,rjk->rik", L, Lq_w), white=False, **kw)
    np.testing.assert_allclose(Ln @ mu_w, mu_u, rtol=0, atol=1e-10)
    np.testing.assert_allclose(np.einsum("ij,rjk->rik", Ln, Ls_w), Ls_u, rtol=0, atol=1e-10)


def test_nystrom_trace_of_the_candidates_own_rows_is_the_jitter_residue():
    rng, Z, _ = inputs(12, 12, 0, 9)
    kw = KERNEL_ARGS["rbf"]
    assert abs(rr.nystrom_trace(Z, Z, jitter=0.0, **kw)) < 1e-8
    cand = rng.standard_normal((50, 9))
    assert 0 < rr.nystrom_trace(Z, cand, jitter=JITTER, **kw) <= 50 * 5.0


# ---- flags -------------------------------------------------------------------------------------------------------------------------
def test_flags_and_parser(tmp_path):
    rows = {f[0]: f for f in FLAGS}
    assert rows["--reselect-every"][1:3] == (int, 0) and rows["--reselect-images"][1:3] == (int, 1000)
    fl = default_parser().parse_args(["--name", "x"])
    assert parse_reselect(fl) == (0, 1000)
    fl = default_parser().parse_args(["--name", "x", "--reselect-every", "3", "--reselect-images", "250"])
    assert parse_reselect(fl) == (3, 250)
    assert parse_reselect(argparse.Namespace()) == (0, 1000)                       # a namespace from before the flags
    assert parse_reselect(argparse.Namespace(reselect_every=None, reselect_images=None)) == (0, 1000)
    with pytest.raises(ValueError, match="--reselect-every"):
        parse_reselect(argparse.Namespace(reselect_every=-1))
    with pytest.raises(ValueError, match="--reselect-images"):
        parse_reselect(argparse.Namespace(reselect_every=1, reselect_images=0))
    log = utils.Log(str(tmp_path), "x", [utils.GlobalStepLogger()])
    log.write_flags(fl)
    log.close()
    lines = open(os.path.join(str(tmp_path), "x", "options.toml")).read().splitlines()
    assert "reselect_every = 3" in lines and "reselect_images = 250" in lines, lines


def test_header_declares_the_entry_points():
    declared = dev.declared_symbols()
    for name in ("dcgp_cross_gram", "dcgp_inducing_transfer"):
        assert name in declared and name in dev._SIGS, name


def test_schedule():
    assert [p for p in range(8) if reselect_due(2, p * 50, 50)] == [2, 4, 6]
    assert [p for p in range(5) if reselect_due(1, p * 50, 50)] == [1, 2, 3, 4]
    assert not any(reselect_due(0, p * 50, 50) for p in range(5))


# ---- the driver, against a recorder ---------------------------------------------------------------------------------------------------
class _Recorder:
    minibatch_size = 4
    parameters = []
    layers = []

    def __init__(self):
        self.X = np.zeros((10, 3))
        self.calls = []

    def train_run(self, idx, lr, seed=0):
        self.calls.append(("train_run", seed))
        return np.arange(len(idx), dtype=np.float64)

    def pull_parameters(self):
        pass

    def reselect_inducing(self, **kw):
        self.calls.append(("reselect", kw))
        return [dict(layer=0, rows=np.arange(4), n_greedy=4, trace_old=2.0, trace_new=1.0, kl_before=3.0, kl_after=2.5)]


class _RecorderExperiment(Experiment):
    def _load_data(self):
        self.X_train = self.Y_train = self.X_test = self.Y_test = None

    def _setup_model(self):
        self.model = _Recorder()
        self.global_step = 0

    def _setup_logger(self):
        self.log = utils.Log(self.flags.log_dir, self.flags.name, [utils.GlobalStepLogger()])
        self.log.write_flags(self.flags)


def test_driver_reselects_on_schedule(tmp_path, capsys):
    def run(name, *extra):
        flags = read_args(["--name", name, "--data", "none.npz", "--log-dir", str(tmp_path), "--test-every", "3", "--batch-size", "4"] + list(extra))
        flags.seed = 7
        exp = _RecorderExperiment(flags)
        for _ in range(5):
            exp.train_step()
        exp.conclude()
        return exp.model.calls
    off = run("off")
    assert [c[0] for c in off] == ["train_run"] * 5                                     # the flag at 0: no new call into the model
    on = run("on", "--reselect-every", "2", "--reselect-images", "123")
    assert [c[0] for c in on] == ["train_run", "train_run", "reselect", "train_run", "train_run", "reselect", "train_run"]
    picks = [c[1] for c in on if c[0] == "reselect"]
    assert picks == [dict(images=123, seed=7 + 6), dict(images=123, seed=7 + 12)]      # seed + global_step of the period's first step
    assert [c[1] for c in on if c[0] == "train_run"] == [7, 10, 13, 16, 19]             # the periods' own seeds are what they were
    out = capsys.readouterr().out
    assert out.count("re-selected") == 2 and "layer 0" in out
    for opt in ("SGD", "NatGrad"):                                                     # every optimiser: the hook sits in front of _optimize
        flags = read_args(["--name", opt, "--data", "none.npz", "--log-dir", str(tmp_path), "--test-every", "3", "--optimizer", opt, "--reselect-every", "1"])
        exp = _RecorderExperiment(flags)
        exp._optimize = lambda: setattr(exp, "global_step", exp.global_step + 3)
        exp.train_step()
        exp.train_step()
        exp.conclude()
        assert [c[0] for c in exp.model.calls] == ["reselect"]


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def test_draws_do_not_depend_on_the_global_generator():
    from deepcgp_amd.models import draw_patches
    imgs = np.random.default_rng(0).standard_normal((6, 8, 8, 2))
    np.random.seed(1)
    a = draw_patches(imgs, 40, 3, DGP_Base._reselect_rng(11, 2))
    ia = DGP_Base._reselect_rng(11, 0).choice(50, size=20, replace=False)
    np.random.seed(2)
    np.random.rand(17)
    state = np.random.get_state()[1].copy()
    b = draw_patches(imgs, 40, 3, DGP_Base._reselect_rng(11, 2))
    ib = DGP_Base._reselect_rng(11, 0).choice(50, size=20, replace=False)
    assert np.array_equal(np.random.get_state()[1], state)                             # untouched
    assert a.tobytes() == b.tobytes() and np.array_equal(ia, ib)
    assert not np.array_equal(a, draw_patches(imgs, 40, 3, DGP_Base._reselect_rng(11, 3)))      # another layer, another stream
    assert not np.array_equal(a, draw_patches(imgs, 40, 3, DGP_Base._reselect_rng(12, 2)))      # another seed
    assert DGP_Base._reselect_rng(2 ** 40 + 5, 1).randint(0, 1000) == DGP_Base._reselect_rng(5, 1).randint(0, 1000)    # seeds are taken mod 2^32
