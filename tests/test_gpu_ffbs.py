"""The marginal particle smoother (psvo_ffbs_smooth, --FFBS) on the GPU: the kernel directly on synthetic particle systems,
through the filter objectives, beside training, and through runner.main.

Accuracy is judged against the fp64 restatement (tests/ffbs_reference.py) with a MEASURED yardstick instead of a hand-set
tolerance: the same restatement run in fp32 on the CPU says what fp32 arithmetic costs at a shape (err_32), and the kernel may
be K times as far from fp64 plus 8 fp32 ulps of the largest value:
    err_hip <= K err_32 + 8 2^-24 max|q_64|            for q in exp(logWs), Xmean, ess.
K: twice the worst err_hip / err_32 measured on the MI355X over all cases of this file, rounded up, not below 2
(profiles/ffbs_smoother.md has the ratios).  Both errors are printed before the assertion (pytest -s shows them).
"""
import glob
import math
import pickle

import pytest
import torch

from oracle import psvo_oracle as O
from tests import ffbs_reference as R
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

K = {"p": 6, "Xmean": 4, "ess": 3}          # worst measured ratios: 2.62, 1.68, 1.42 (profiles/ffbs_smoother.md)
EDGE_TOL = 5e-6            # (tests/test_gpu_large.py: a flipped draw needs u within this of a CDF edge)
ULP = 2.0 ** -24

# (T, B, Dx, N, sigma, per-particle scales)
SHAPES = [
    (1, 1, 2, 8, 1.0, False),          # no recursion
    (2, 2, 2, 12, 1.0, False),         # one step, sub-wave N that is not a power of two
    (6, 2, 3, 100, 1.0, False),
    (7, 2, 2, 130, 0.3, True),         # N just past two waves
    (6, 1, 4, 256, 1.0, False),
    (6, 2, 4, 300, 0.1, True),         # the 512-thread configuration, partly filled
    (5, 1, 4, 512, 1.0, False),
    (40, 2, 2, 64, 0.05, False),       # sharp transitions: ESS collapses to 1, log-densities reach about -800
    (200, 1, 2, 64, 0.3, True),        # drift over a bench-length T
]
_ids = lambda s: "-".join(map(str, s))


def _system(T, B, Dx, N, sig, cov, seed=3):
    """particles scattered around a random walk, transition means near them; fp32 values (what the kernel is given)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    X = torch.cumsum(0.3 * rn(T, B, Dx, 1), 0) + 2 * sig * rn(T, B, Dx, N)
    Fm = X + 0.1 * torch.tanh(X) + 0.05 * rn(T, B, Dx, N)
    S = torch.full((T, B, Dx, N), sig, dtype=torch.float64)
    if cov:
        S = S * (0.5 + torch.rand(T, B, Dx, N, generator=g, dtype=torch.float64))
    logW = -3.0 + 1.5 * rn(T, B, N)
    u = torch.rand(T, B, N, generator=g, dtype=torch.float64)
    return tuple(v.float().contiguous() for v in (X, Fm, S, logW, u))


_CACHE = {}


def _case(shape):
    """inputs (fp32, CPU) and both references of a shape, computed once and shared by the tests below"""
    if shape not in _CACHE:
        X, Fm, S, logW, u = _system(*shape)
        q64 = R.quantities(X.double(), Fm.double(), S.double(), logW.double())
        q32 = R.quantities(X, Fm, S, logW)
        _CACHE[shape] = dict(X=X, Fm=Fm, S=S, logW=logW, u=u, q64=q64, q32=q32)
    return _CACHE[shape]


def _launch(shape, c, **kw):
    from psvo_amd import ops
    T, B, Dx, N, sig, cov = shape
    desc = ops.make_desc(B, T, N, 1, Dx, 1, 32)
    filt = {"X": c["X"].cuda(), "Fm": c["Fm"].cuda(), "logW": c["logW"].cuda(), "Fs": c["S"].cuda() if cov else None}
    sig_f = None if cov else c["S"][0, 0, :, 0].contiguous().cuda()
    out = ops.ffbs_smooth(desc, filt, sig_f=sig_f, **kw)
    torch.cuda.synchronize()
    return filt, out


def _yardstick(tag, hip, q64, q32):
    """hip: dict(p, Xmean, ess) of fp64 CPU tensors; asserts the rule of the module docstring, printing the figures first"""
    failed = []
    for name in ("p", "Xmean", "ess"):
        err_hip = float((hip[name] - q64[name]).abs().max())
        err_32 = float((q32[name] - q64[name]).abs().max())
        floor = 8 * ULP * float(q64[name].abs().max())
        print("ffbs-yardstick %s %s err_hip %.3e err_32 %.3e ratio %.3f floor %.3e"
              % (tag, name, err_hip, err_32, err_hip / err_32 if err_32 > 0 else float("inf"), floor))
        if not err_hip <= K[name] * err_32 + floor:
            failed.append((name, err_hip, err_32, floor))
    assert not failed, failed


def _check_draws(logWs, u, idx, X, Xs):
    """the draws against the kernel's OWN smoothed weights (isolates the prefix sum and the search), and the gather"""
    T, B, N = logWs.shape
    flat = lambda v: v.reshape(T * B, N).t()
    d = O.draw_distance(flat(logWs.double().cpu()), flat(u.double().cpu()), flat(idx.long().cpu()))
    ref = R.draw(logWs.double().cpu(), u.double().cpu())
    assert float(O.draw_distance(flat(logWs.double().cpu()), flat(u.double().cpu()), flat(ref)).max()) == 0.0
    worst, off = float(d.max()), int((d > 0).sum())
    print("ffbs-draws worst %.3e off %d of %d" % (worst, off, d.numel()))
    assert worst <= EDGE_TOL
    assert off <= max(3, int(20 * EDGE_TOL * d.numel()))
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    assert torch.equal(Xs, torch.gather(X, 3, idx.long().unsqueeze(2).expand(-1, -1, X.shape[2], -1)))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_kernel_against_fp64(built_lib, shape):
    T, B, Dx, N, sig, cov = shape
    c = _case(shape)
    filt, out = _launch(shape, c, u=c["u"].cuda())
    for k, v in out.items():
        assert torch.isfinite(v.float()).all(), k
    lw = out["logWs"].double().cpu()
    assert float((lw.exp().sum(-1) - 1).abs().max()) <= 64 * ULP
    last = c["logW"][T - 1].double()
    last = last - torch.logsumexp(last, -1, keepdim=True)
    ulp = 2.0 ** (math.floor(math.log2(float(last.abs().max()))) - 23)
    assert float((lw[T - 1] - last).abs().max()) <= 4 * ulp
    hip = {"p": lw.exp(), "Xmean": out["Xmean"].double().cpu(), "ess": out["ess"].double().cpu()}
    _yardstick(_ids(shape), hip, c["q64"], c["q32"])
    _check_draws(out["logWs"], c["u"], out["idx"], filt["X"], out["Xs"])


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[6]], ids=_ids)
def test_teacher_forced_draws_and_no_draws(built_lib, shape):
    T, B, Dx, N, sig, cov = shape
    c = _case(shape)
    filt, base = _launch(shape, c, u=c["u"].cuda())
    idx_in = torch.randint(0, N, (T, B, N), generator=torch.Generator().manual_seed(9), dtype=torch.int32).cuda()
    _, out = _launch(shape, c, idx_in=idx_in)
    assert torch.equal(out["idx"], idx_in)
    assert torch.equal(out["Xs"], torch.gather(filt["X"], 3, idx_in.long().unsqueeze(2).expand(-1, -1, Dx, -1)))
    _, none = _launch(shape, c, want_draws=False)
    assert none["Xs"] is None and none["idx"] is None
    for k in ("logWs", "Xmean", "ess"):
        assert torch.equal(out[k], base[k]) and torch.equal(none[k], base[k]), k
    from psvo_amd import ops
    with pytest.raises(ValueError):
        _launch(shape, c)                                            # draws wanted, nothing to draw with
    with pytest.raises(ValueError):
        ops.ffbs_smooth(ops.make_desc(B, T, N, 1, Dx, 1, 32), dict(filt, Fs=c["S"].cuda()),
                        sig_f=c["S"][0, 0, :, 0].contiguous().cuda(), want_draws=False)      # both scales
    with pytest.raises(ValueError):
        ops.ffbs_smooth(ops.make_desc(B, T, N, 1, Dx, 1, 32), dict(filt, Fs=None), want_draws=False)      # neither


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_two_launches_are_bit_identical(built_lib, shape):
    from psvo_amd import _lib
    c = _case(shape)
    u = c["u"].cuda()
    _, a = _launch(shape, c, u=u)
    _, b = _launch(shape, c, u=u)
    with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, 1):
        _, d1 = _launch(shape, c, u=u)
        _, d2 = _launch(shape, c, u=u)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(d1[k], d2[k]) and torch.equal(a[k], d1[k]), k


# ---- through the model ---------------------------------------------------------------------------------------------------
_COV = dict(output_cov=True, diag_cov=True)
MODEL_CASES = [
    # (objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q), extra flags
    (("AESMC", 2, 6, 16, 1, 2, 1, 32, True, True), {}),
    (("AESMC", 2, 6, 16, 1, 2, 1, 32, True, True), dict(q1_layers="32,32", g_layers="32,32")),
    (("IWAE", 2, 8, 96, 1, 3, 1, 16, False, True), {}),                 # weights carried, never resampled
    (("SVO", 2, 6, 24, 1, 2, 2, 32, False, False), {}),
    (("AESMC", 2, 7, 130, 1, 2, 1, 16, True, False), _COV),             # bootstrap: Fs comes from the shared head
    (("SVO", 2, 5, 40, 1, 3, 2, 16, False, True), dict(_COV, poisson_emission=True)),
]


def _setup(obj, B, T, N, M, Dx, Dy, H, bootstrap, two_q, seed=0, **extra):
    """a perturbed model, its objective, observations and the oracle's noise in the kernels' layout (as tests/test_gpu_parity.py)"""
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.IWAE import IWAE
    from psvo_amd.SMC.SVO import SVO
    cls = {"SVO": SVO, "AESMC": AESMC, "IWAE": IWAE}[obj]
    hs = str(H)
    kw = dict(Dx=Dx, Dy=Dy, n_particles=N, n_particles_for_BSim_proposal=M, batch_size=B, time=T,
              q0_layers=hs, q1_layers=hs, q2_layers=hs, f_layers=hs, g_layers=hs,
              y_smoother_Dhs="8", X0_smoother_Dhs="8", use_bootstrap=bootstrap, use_2_q=two_q)
    kw.update(extra)
    FLAGS = Hh.make_flags(obj, **kw)
    torch.manual_seed(seed)
    model = Hh.perturb_(SSM(FLAGS)).cuda()
    g = torch.Generator().manual_seed(100 + seed)
    obs = (torch.randn(B, T, Dy, generator=g, dtype=torch.float64) * 1.5).float().cuda()
    noise = Hh.noise_to_hip(O.make_noise(Hh.oracle_flags(FLAGS, obj), B, T, seed=1234 + seed), "cuda")
    noise["u_s"] = torch.rand(T, B, N, generator=g).cuda()
    return FLAGS, model, cls, obs, noise


@pytest.mark.parametrize("case,extra", MODEL_CASES, ids=lambda v: _ids(v) if isinstance(v, tuple) else ",".join(sorted(v)) or "plain")
def test_smoother_behind_the_filter_objectives(built_lib, case, extra):
    obj, B, T, N, M, Dx = case[:6]
    FLAGS, model, cls, obs, noise = _setup(*case, FFBS=True, **extra)
    smc = cls(model, FLAGS)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs, None, noise=noise)
        z0, log0 = cls(model, Hh.make_flags(obj, **{**FLAGS.as_dict(), "FFBS": False})).get_log_ZSMC(obs, None, noise=noise)
    torch.cuda.synchronize()
    filt = log["filter"]
    assert torch.equal(z, z0) and torch.equal(filt["logW"], log0["filter"]["logW"])       # the filter itself is untouched
    assert "Xs_filter" not in log0 and "ess_smooth" not in log0
    assert log["Xs"].shape == (B, T, N, Dx)
    assert torch.equal(log["Xs_filter"], filt["Xanc"].permute(1, 0, 3, 2)) and torch.equal(log0["Xs"], log["Xs_filter"])
    assert log["X_smooth_mean"].shape == (B, T, Dx) and log["ess_smooth"].shape == (B, T)
    assert log["logW_smooth"].shape == (T, B, N)

    # the restatement on the filter's own outputs
    X, Fm, logW = (filt[k].cpu() for k in ("X", "Fm", "logW"))
    if FLAGS.output_cov:
        S = filt["Fs"].cpu()
    else:
        dist = model.q1_dist if FLAGS.use_bootstrap else model.f_dist
        S = R.scales(dist.get_sigma().detach().float().cpu(), T, B, Dx, N, dtype=torch.float32)
    q64 = R.quantities(X.double(), Fm.double(), S.double(), logW.double())
    q32 = R.quantities(X, Fm, S, logW)
    hip = {"p": log["logW_smooth"].double().cpu().exp(), "Xmean": log["X_smooth_mean"].transpose(0, 1).double().cpu(),
           "ess": log["ess_smooth"].transpose(0, 1).double().cpu()}
    for v in hip.values():
        assert torch.isfinite(v).all()
    _yardstick(_ids(case) + ("+" + ",".join(sorted(extra)) if extra else ""), hip, q64, q32)
    sm = log["smoother"]
    _check_draws(log["logW_smooth"], noise["u_s"], sm["idx"], filt["X"], sm["Xs"])
    assert torch.equal(log["Xs"], sm["Xs"].permute(1, 0, 3, 2))

    # teacher-forced smoothed draws, and the objective's own generator when nothing is injected
    with torch.no_grad():
        _, log2 = smc.get_log_ZSMC(obs, None, noise=dict({k: v for k, v in noise.items() if k != "u_s"}, idx_s=sm["idx"]))
        smc.generator = torch.Generator(device="cuda").manual_seed(5)
        _, log3 = smc.get_log_ZSMC(obs, None)
        smc.generator.manual_seed(5)
        _, log4 = smc.get_log_ZSMC(obs, None)
    assert torch.equal(log2["Xs"], log["Xs"])
    assert torch.equal(log3["Xs"], log4["Xs"]) and torch.equal(log3["ess_smooth"], log4["ess_smooth"])


@pytest.mark.parametrize("case,extra", [MODEL_CASES[0], MODEL_CASES[3]], ids=["AESMC", "SVO"])
def test_training_is_unaffected(built_lib, monkeypatch, case, extra):
    """under autograd the smoother is not launched; ELBO and every parameter gradient are bit-identical with and without --FFBS"""
    from psvo_amd import ops
    obj = case[0]
    FLAGS, model, cls, obs, noise = _setup(*case, FFBS=True, **extra)

    def refuse(*a, **k):
        raise AssertionError("ops.ffbs_smooth was called under autograd")
    monkeypatch.setattr(ops, "ffbs_smooth", refuse)
    res = []
    for ffbs in (True, False):
        smc = cls(model, Hh.make_flags(obj, **{**FLAGS.as_dict(), "FFBS": ffbs}))
        assert smc.FFBS is ffbs
        model.zero_grad(set_to_none=True)
        z, log = smc.get_log_ZSMC(obs, None, noise=noise)
        z.backward()
        torch.cuda.synchronize()
        assert "Xs_filter" not in log and "ess_smooth" not in log
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 4
    for n, g in res[0][1].items():
        assert torch.equal(g, res[1][1][n]), n


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """runner.main with --AESMC --FFBS (and --noPSVO: PSVO is the registry's default objective): the four ffbs_ess_* keys are in
    metric_*.p, within [1, N]; the trajectories have their usual shape; the same run without --FFBS has no such keys"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    argv = ["--noPSVO", "--AESMC", "--generateTrainingData", "--time=20", "--n_train=4", "--n_test=4", "--batch_size=2",
            "--n_particles=16", "--epoch=1"]
    keys = ["ffbs_ess_%s_%s" % (s, split) for s in ("mean", "min") for split in ("train", "test")]
    for ffbs in (True, False):
        work = tmp_path / ("on" if ffbs else "off")
        work.mkdir()
        monkeypatch.chdir(work)
        runner.main(parse_flags(argv + (["--FFBS"] if ffbs else [])))
        torch.cuda.synchronize()
        metrics = glob.glob(str(work / "rslts" / "epoch_data" / "**" / "metric_*.p"), recursive=True)
        assert metrics
        for path in metrics:
            with open(path, "rb") as fh:
                m = pickle.load(fh)
            if ffbs:
                for split in ("train", "test"):
                    lo, mean = m["ffbs_ess_min_" + split], m["ffbs_ess_mean_" + split]
                    assert 1 <= lo <= mean <= 16, (split, lo, mean)
            else:
                assert not any(k in m for k in keys) and not any(k.startswith("ffbs") for k in m)
        traj = glob.glob(str(work / "rslts" / "epoch_data" / "**" / "trajectory_*.p"), recursive=True)
        assert traj
        with open(traj[0], "rb") as fh:
            assert pickle.load(fh)["Xs"].shape == (4, 20, 16, 2)
        assert glob.glob(str(work / "rslts" / "epoch_data" / "**" / "y_hat_*.p"), recursive=True)
