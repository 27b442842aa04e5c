"""The backward sampler (psvo_ffbs_sample, --FFBSi) on the GPU: the kernel directly on synthetic particle systems, through the
filter objectives, beside training, and through runner.main.

Direct launches use the smoother's shapes and systems (tests/test_gpu_ffbs.py: SHAPES, _system, seed 3) plus N = 1 and two
systems with particles of weight zero (tests/ffbsi_reference.cases).  Log-probabilities are judged against the fp64 restatement
(tests/ffbsi_reference.py) by the smoother's rule, with the yardstick err_32 = what the same restatement costs in fp32 on the CPU:
    err_hip <= K err_32 + 8 2^-24 max|logq_64|,   K = 8
(profiles/ffbs_smoother.md: no quantity of the same pair arithmetic exceeded this ratio).  Draws are judged in fp64 given the
kernel's own successor indices: an index is off only where u sits within EDGE_TOL of a CDF edge, and only a few may be.
Figures are printed before every assertion (pytest -s shows them); profiles/ffbsi_sampler.md records them.
"""
import glob
import pickle

import pytest
import torch

from tests import ffbsi_reference as R
from tests import helpers as Hh
from tests.test_gpu_ffbs import MODEL_CASES, _setup
from tests.test_gpu_large import EDGE_TOL

pytestmark = pytest.mark.gpu

K = 8
ULP = 2.0 ** -24
CASES = R.cases()
_params = pytest.mark.parametrize("shape,masked", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
_ids = lambda s: "-".join(map(str, s))
KEYS = ("Xs", "idx", "logq", "distinct")


def _launch(shape, c, **kw):
    from psvo_amd import ops
    T, B, Dx, N, sig, cov = shape
    desc = ops.make_desc(B, T, N, 1, Dx, 1, 32)
    filt = {"X": c["X"].cuda(), "Fm": c["Fm"].cuda(), "logW": c["logW"].cuda(), "Fs": c["S"].cuda() if cov else None}
    sig_f = None if cov else c["S"][0, 0, :, 0].contiguous().cuda()
    out = ops.ffbs_sample(desc, filt, sig_f=sig_f, **kw)
    torch.cuda.synchronize()
    assert set(out) == set(KEYS)
    assert out["Xs"].shape == (T, B, Dx, N) and out["idx"].shape == (T, B, N) and out["idx"].dtype == torch.int32
    assert out["logq"].shape == (T, B, N) and out["distinct"].shape == (T, B) and out["distinct"].dtype == torch.int32
    return filt, out


@_params
def test_teacher_forced_values(built_lib, shape, masked):
    T, B, Dx, N = shape[:4]
    c = R.case(shape, masked)
    idx_in = c["idx_in"].cuda()
    filt, out = _launch(shape, c, idx_in=idx_in)
    assert torch.equal(out["idx"], idx_in)
    assert torch.equal(out["Xs"], R.gather(filt["X"], idx_in))
    assert torch.equal(out["distinct"].cpu().long(), c["forced64"]["distinct"])
    ref = c["forced64"]["logq"]
    err_hip, biggest = R.forced_error(out["logq"].cpu(), ref)
    err_32, _ = R.forced_error(c["forced32"]["logq"], ref)
    floor = 8 * ULP * biggest
    print("ffbsi-yardstick %s%s logq err_hip %.3e err_32 %.3e ratio %.3f floor %.3e"
          % (_ids(shape), "-masked" if masked else "", err_hip, err_32, err_hip / err_32 if err_32 > 0 else float("inf"), floor))
    assert err_hip <= K * err_32 + floor
    # uniforms beside forced indices change nothing: the forced indices win
    _, both = _launch(shape, c, idx_in=idx_in, u=c["u"].cuda())
    for k in KEYS:
        assert torch.equal(both[k], out[k]), k


@_params
def test_free_running_draws(built_lib, shape, masked):
    T, B, Dx, N = shape[:4]
    c = R.case(shape, masked)
    filt, out = _launch(shape, c, u=c["u"].cuda())
    idx = out["idx"].cpu().long()
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    d = R.draw_distances(c["X"], c["Fm"], c["S"], c["logW"], c["u"], idx)
    d32 = R.draw_distances(c["X"], c["Fm"], c["S"], c["logW"], c["u"], c["free32"]["idx"])
    worst, off, dead = float(d.max()), int((d > 0).sum()), int((~torch.isfinite(torch.gather(c["logW"], 2, idx))).sum())
    same = int((idx == c["free32"]["idx"]).sum())
    print("ffbsi-draws %s%s worst %.3e off %d of %d weight-zero %d (fp32 restatement: worst %.3e off %d); %d indices as the "
          "restatement's; distinct mean %.1f min %d"
          % (_ids(shape), "-masked" if masked else "", worst, off, d.numel(), dead, float(d32.max()), int((d32 > 0).sum()), same,
             float(out["distinct"].float().mean()), int(out["distinct"].min())))
    assert float(d32.max()) == 0.0
    assert dead == 0
    assert worst <= EDGE_TOL
    assert off <= max(3, int(20 * EDGE_TOL * d.numel()))
    assert torch.equal(out["Xs"], R.gather(filt["X"], out["idx"]))
    assert torch.equal(out["distinct"].cpu().long(), R.distinct(idx))
    assert torch.isfinite(out["logq"]).all() and float(out["logq"].max()) <= 1e-5
    # the log-probabilities of the drawn indices are those of the same indices teacher-forced
    _, forced = _launch(shape, c, idx_in=out["idx"])
    for k in KEYS:
        assert torch.equal(forced[k], out[k]), k


@_params
def test_two_launches_are_bit_identical(built_lib, shape, masked):
    from psvo_amd import _lib
    c = R.case(shape, masked)
    u = c["u"].cuda()
    _, a = _launch(shape, c, u=u)
    _, b = _launch(shape, c, u=u)
    with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, 1):
        _, d1 = _launch(shape, c, u=u)
        _, d2 = _launch(shape, c, u=u)
    for k in KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(d1[k], d2[k]) and torch.equal(a[k], d1[k]), k


def test_op_refuses_bad_arguments(built_lib):
    """the shape checks and the error style of ops.ffbs_smooth"""
    from psvo_amd import ops
    T, B, Dx, N = 3, 2, 2, 8
    desc = ops.make_desc(B, T, N, 1, Dx, 1, 32)
    z = lambda *s: torch.zeros(*s, device="cuda")
    filt = {"X": z(T, B, Dx, N), "Fm": z(T, B, Dx, N), "logW": z(T, B, N), "Fs": None}
    sig, u = torch.ones(Dx, device="cuda"), z(T, B, N)
    with pytest.raises(ValueError, match="exactly one transition scale"):
        ops.ffbs_sample(desc, filt, u=u)
    with pytest.raises(ValueError, match="exactly one transition scale"):
        ops.ffbs_sample(desc, dict(filt, Fs=z(T, B, Dx, N)), sig_f=sig, u=u)
    with pytest.raises(ValueError, match="uniforms"):
        ops.ffbs_sample(desc, filt, sig_f=sig)
    with pytest.raises(ValueError, match="needs the filter's"):
        ops.ffbs_sample(desc, dict(filt, Fm=None), sig_f=sig, u=u)
    with pytest.raises(ValueError, match="logW must have shape"):
        ops.ffbs_sample(desc, dict(filt, logW=z(T, B, N + 1)), sig_f=sig, u=u)
    with pytest.raises(ValueError, match="idx_in must be"):
        ops.ffbs_sample(desc, filt, sig_f=sig, idx_in=torch.zeros(T, B, N, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="unsupported"):
        ops.ffbs_sample(ops.make_desc(B, T, 600, 1, Dx, 1, 32), {"X": z(T, B, Dx, 600), "Fm": z(T, B, Dx, 600),
                                                                 "logW": z(T, B, 600)}, sig_f=sig, u=z(T, B, 600))


# ---- through the model ---------------------------------------------------------------------------------------------------
WOBS_CASE = (("AESMC", 2, 7, 100, 1, 3, 10, 32, False, True), {})          # Dy = 10: the wide-observation filter feeds the sampler


def _flags_with(FLAGS, obj, **kw):
    return Hh.make_flags(obj, **{**FLAGS.as_dict(), **kw})


@pytest.mark.parametrize("case,extra", MODEL_CASES + [WOBS_CASE],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else ",".join(sorted(v)) or "plain")
def test_sampler_behind_the_filter_objectives(built_lib, case, extra):
    obj, B, T, N, M, Dx = case[:6]
    FLAGS, model, cls, obs, noise = _setup(*case, FFBSi=True, **extra)
    noise["u_p"] = torch.rand(T, B, N, generator=torch.Generator().manual_seed(77)).cuda()
    smc = cls(model, FLAGS)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs, None, noise=noise)
        z0, log0 = cls(model, _flags_with(FLAGS, obj, FFBSi=False)).get_log_ZSMC(obs, None, noise=noise)
    torch.cuda.synchronize()
    filt = log["filter"]
    assert torch.equal(z, z0)                                               # the filter itself is untouched
    for k in ("X", "Xanc", "Fm", "logW", "lse"):
        assert torch.equal(filt[k], log0["filter"][k]), k
    for k in ("Xs_filter", "path_logq", "path_distinct", "paths", "Xs_marginal"):
        assert k not in log0, k
    assert "Xs_marginal" not in log and "ess_smooth" not in log
    paths = log["paths"]
    assert set(paths) == set(KEYS)
    assert log["Xs"].shape == (B, T, N, Dx) and log["path_logq"].shape == (T, B, N) and log["path_distinct"].shape == (B, T)
    assert torch.equal(log["Xs"], R.gather(filt["X"], paths["idx"]).permute(1, 0, 3, 2))
    assert torch.equal(log["Xs"], paths["Xs"].permute(1, 0, 3, 2))
    assert torch.equal(log["Xs_filter"], filt["Xanc"].permute(1, 0, 3, 2)) and torch.equal(log0["Xs"], log["Xs_filter"])
    assert torch.equal(log["path_logq"], paths["logq"]) and torch.equal(log["path_distinct"], paths["distinct"].t())
    assert torch.equal(paths["distinct"].cpu().long(), R.distinct(paths["idx"].cpu()))
    assert torch.isfinite(paths["logq"]).all() and float(paths["logq"].max()) <= 1e-5
    assert int(paths["idx"].min()) >= 0 and int(paths["idx"].max()) < N

    # teacher-forced paths, and the objective's own generator when nothing is injected
    with torch.no_grad():
        _, log2 = smc.get_log_ZSMC(obs, None, noise=dict({k: v for k, v in noise.items() if k != "u_p"}, idx_p=paths["idx"]))
        smc.generator = torch.Generator(device="cuda").manual_seed(5)
        _, log3 = smc.get_log_ZSMC(obs, None)
        smc.generator.manual_seed(5)
        _, log4 = smc.get_log_ZSMC(obs, None)
    assert torch.equal(log2["Xs"], log["Xs"]) and torch.equal(log2["path_logq"], log["path_logq"])
    assert torch.equal(log3["Xs"], log4["Xs"]) and torch.equal(log3["path_distinct"], log4["path_distinct"])

    # with --FFBS as well both kernels run: the smoother's outputs are those of an --FFBS-only run
    with torch.no_grad():
        _, both = cls(model, _flags_with(FLAGS, obj, FFBS=True)).get_log_ZSMC(obs, None, noise=noise)
        _, only = cls(model, _flags_with(FLAGS, obj, FFBS=True, FFBSi=False)).get_log_ZSMC(obs, None, noise=noise)
    torch.cuda.synchronize()
    for k in ("X_smooth_mean", "ess_smooth", "logW_smooth", "Xs_filter"):
        assert torch.equal(both[k], only[k]), k
    for k in only["smoother"]:
        assert torch.equal(both["smoother"][k], only["smoother"][k]), k
    assert torch.equal(both["Xs_marginal"], only["Xs"]) and "Xs_marginal" not in only
    assert torch.equal(both["Xs"], log["Xs"]) and torch.equal(both["path_logq"], log["path_logq"])


@pytest.mark.parametrize("case,extra", [MODEL_CASES[0], MODEL_CASES[3]], ids=["AESMC", "SVO"])
def test_training_is_unaffected(built_lib, monkeypatch, case, extra):
    """under autograd the sampler is not launched; ELBO and every parameter gradient are bit-identical with and without
    --FFBSi"""
    from psvo_amd import ops
    obj = case[0]
    FLAGS, model, cls, obs, noise = _setup(*case, FFBSi=True, **extra)

    def refuse(*a, **k):
        raise AssertionError("ops.ffbs_sample was called under autograd")
    monkeypatch.setattr(ops, "ffbs_sample", refuse)
    res = []
    for on in (True, False):
        smc = cls(model, _flags_with(FLAGS, obj, FFBSi=on))
        assert smc.FFBSi is on
        model.zero_grad(set_to_none=True)
        z, log = smc.get_log_ZSMC(obs, None, noise=noise)
        z.backward()
        torch.cuda.synchronize()
        assert "Xs_filter" not in log and "paths" not in log
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 4
    for n, g in res[0][1].items():
        assert torch.equal(g, res[1][1][n]), n


@pytest.mark.parametrize("case,extra", [MODEL_CASES[0], MODEL_CASES[3]], ids=["AESMC", "SVO"])
def test_step_replays_from_hipgraph(built_lib, monkeypatch, case, extra):
    """a local training step under --FFBSi, eager and captured into a GraphedStep: the replay equals the eager step bit for
    bit; the sampler is never launched.  (Deterministic mode: the filter's reverse pass
    otherwise adds with LDS float atomics, whose order a replay need not keep.  The step is built as in tests/test_gpu_wobs.py:
    a fresh model, the flat gradient buffer before the first backward pass, and nothing of an earlier evaluation's autograd
    graph alive at the capture -- SVO._release says what such a leftover does to a capture.)"""
    from psvo_amd import _lib, ops
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    FLAGS, model, cls, obs, noise = _setup(*case, FFBSi=True, **extra)

    def refuse(*a, **k):
        raise AssertionError("ops.ffbs_sample was called under autograd")
    monkeypatch.setattr(ops, "ffbs_sample", refuse)
    smc = cls(model, FLAGS)
    assert smc.FFBSi is True
    flat = FlatParams(model)

    def local():
        flat.zero_grad()
        z, _ = smc.get_log_ZSMC(obs, None, noise=noise)
        z.backward()
        return z.detach()
    with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, 1):
        z_e = local().clone()
        g_e = flat.grad.clone()
        torch.cuda.synchronize()
        assert torch.isfinite(z_e) and torch.isfinite(g_e).all() and float(g_e.abs().max()) > 0
        step = GraphedStep(local)
        for _ in range(2):
            flat.grad.fill_(float("nan"))
            z_g = step()
            torch.cuda.synchronize()
            assert torch.equal(z_g, z_e)
            assert torch.equal(flat.grad, g_e)


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """runner.main with --AESMC --FFBSi (and --noPSVO: PSVO is the registry's default objective): the four ffbsi_distinct_* keys
    are in metric_*.p, within [1, N]; the saved trajectories have the (saving_num, T, N, Dx) protocol"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    argv = ["--noPSVO", "--AESMC", "--FFBSi", "--generateTrainingData", "--time=12", "--n_train=4", "--n_test=4",
            "--batch_size=2", "--n_particles=16", "--epoch=2"]
    monkeypatch.chdir(tmp_path)
    FLAGS = parse_flags(argv)
    runner.main(FLAGS)
    torch.cuda.synchronize()
    metrics = glob.glob(str(tmp_path / "rslts" / "epoch_data" / "**" / "metric_*.p"), recursive=True)
    assert metrics
    for path in metrics:
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        for split in ("train", "test"):
            lo, mean = m["ffbsi_distinct_min_" + split], m["ffbsi_distinct_mean_" + split]
            assert 1 <= lo <= mean <= 16, (split, lo, mean)
        assert not any(k.startswith("ffbs_ess") for k in m)
    traj = glob.glob(str(tmp_path / "rslts" / "epoch_data" / "**" / "trajectory_*.p"), recursive=True)
    assert traj
    with open(traj[0], "rb") as fh:
        assert pickle.load(fh)["Xs"].shape == (min(FLAGS.saving_num, 4), 12, 16, 2)
