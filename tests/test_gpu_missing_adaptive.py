"""Adaptive resampling on missing observations (FLAGS.missing_obs with FLAGS.resample_ess and FLAGS.resample_ess_missing_obs;
psvo_filter_forward_wobs_missing_adaptive / psvo_filter_backward_wobs_missing_adaptive, the fourth compilation of
psvo_amd/csrc/filter_wobs_impl.h) on the GPU against the fp64 reference of tests/missing_adaptive_reference.py.

Cases (MA.CASES) are the smallest shapes that reach each form of the kernels; the mask is MR.mask with the case's seed.  Value
tolerances are tests/test_gpu_missing.py::_assert_values's (X / Xanc / Xs 2e-4, logW / lse 5e-4, the ELBO 1e-4 relative), the
gradient tolerance is the suite's 2e-3 of a tensor's largest entry + 1e-6, and the effective sample size is held to
MARGIN = 4 x ESS_GAP32_MISSING of N: ESS_GAP32_MISSING is the largest |ESS_fp32 - ESS_fp64| / N the fp32 CPU reference shows on
these cases (tests/test_missing_adaptive_host.py measures it and holds it to that figure) and 4 allows for the kernel's v_exp_f32
against libm.  Every case keeps its ESS / N at least 100 x MARGIN away from its threshold (same host test), so the decisions of a
free run are the reference's."""
import functools
import glob
import pickle

import numpy as np
import pytest
import torch

from oracle import psvo_oracle as O
from tests import adaptive_reference as AR
from tests import count_reference as CR
from tests import helpers as Hh
from tests import missing_adaptive_reference as MA
from tests.test_gpu_large import EDGE_TOL
from tests.test_gpu_missing import _assert_values, _lorenz_with_gaps
from tests.test_gpu_parity import _pairs
from tests.test_gpu_wobs import _run_main
from tests.test_gpu_wobs_adaptive import _grads, _hip, _run

pytestmark = pytest.mark.gpu

MARGIN = 4 * MA.ESS_GAP32_MISSING
CASES = list(range(len(MA.CASES)))
COUNT_CASES = [i for i in CASES if MA.is_count(MA.CASES[i])]
_id = lambda i: MA.case_id(MA.CASES[i])


@functools.lru_cache(maxsize=None)
def _reference(i):
    """case i's set-up on the GPU and the fp64 reference free running on it (computed once, shared, never modified)"""
    case = MA.CASES[i]
    FLAGS, model, smc, obs, noise, m = MA.setup(case, "cuda")
    assert smc.missing_obs and smc.resample_ess == case[11] and not smc.wide_obs
    z_ref, ref = MA.run_oracle(model, FLAGS, case, obs, noise)
    teacher = {"idx_f": ref["idx_f"], "rs_f": ref["rs_f"].long()}
    return dict(FLAGS=FLAGS, model=model, smc=smc, obs=obs, noise=noise, mask=m, z_ref=z_ref, ref=ref, teacher=teacher)


def _check_ess(i, filt, ref):
    N = MA.CASES[i][3]
    gap = float(((filt["ess"].double().cpu() - ref["ess"]).abs() / N).max())
    print("%s: |ESS - ESS_ref| / N max %.3e (margin %.3e)" % (_id(i), gap, MARGIN))
    assert gap <= MARGIN, "ESS off by %.3e N (margin %.3e N)" % (gap, MARGIN)


@pytest.mark.parametrize("i", CASES, ids=_id)
def test_teacher_forced_values_and_decisions(built_lib, i):
    """the reference's indices and decisions teacher-forced: values against fp64, rs_out is what was forced, which is the rule
    applied to the reference's ESS on these weights, and ESS is within the margin"""
    r = _reference(i)
    case, ref = MA.CASES[i], r["ref"]
    T, B, N, tau = case[2], case[1], case[3], case[11]
    with torch.no_grad():
        z, log = r["smc"].get_log_ZSMC(r["obs"].float().cuda(), None, noise=_hip(r["noise"], r["teacher"]))
    torch.cuda.synchronize()
    filt = log["filter"]
    assert set(filt) == {"lse", "Fm", "logW", "X", "Xanc", "idx", "eps", "u", "rs", "ess"}
    assert r["smc"]._desc().emission == (2 if MA.is_count(case) else int(bool(case[9].get("poisson_emission"))))
    assert torch.equal(log["missing"].cpu(), torch.isnan(r["obs"])) and torch.equal(log["missing"].cpu(), r["mask"][0])
    assert torch.isfinite(filt["logW"]).all() and torch.isfinite(filt["lse"]).all() and torch.isfinite(filt["ess"]).all()
    _assert_values(z, log, r["z_ref"], ref)
    rs_hip = filt["rs"].cpu() != 0
    assert filt["rs"].dtype == torch.int32 and filt["rs"].shape == (T, B) and bool(((filt["rs"] == 0) | (filt["rs"] == 1)).all())
    assert torch.equal(rs_hip, ref["rs_f"]) and torch.equal(rs_hip, AR.decide(ref["ess"], tau, N))
    assert torch.equal(log["ess"], filt["ess"].t()) and torch.equal(log["resampled"], (filt["rs"] != 0).t())
    assert 0 < int(rs_hip.sum()) < T * B
    _check_ess(i, filt, ref)


@pytest.mark.parametrize("i", CASES, ids=_id)
def test_free_running(built_lib, i):
    """in-kernel draws and decisions: the decisions are the reference's free-running ones; the reference replayed with the HIP
    run's indices and decisions gives the values, and every HIP draw lies on its CDF edge on the replayed weights"""
    r = _reference(i)
    case = MA.CASES[i]
    N, tau = case[3], case[11]
    with torch.no_grad():
        z, log = r["smc"].get_log_ZSMC(r["obs"].float().cuda(), None, noise=_hip(r["noise"]))
    torch.cuda.synchronize()
    filt = log["filter"]
    o = MA.objective(r["model"].export_reference_layout(torch.float64), r["FLAGS"], case)
    o.draw_log = []
    with torch.no_grad():
        z_rep, rep = o.get_log_ZSMC(r["obs"].double().cpu(), {**r["noise"], **MA.hip_teacher(log)})
    draws = off = 0
    worst = 0.0
    for log_W, u, idx in o.draw_log:
        d = O.draw_distance(log_W, u, idx)
        draws += d.numel()
        off += int((d > 0).sum())
        worst = max(worst, float(d.max()))
    differ = int((filt["idx"].permute(0, 2, 1).cpu().long() != r["ref"]["idx_f"]).sum())
    print("%s: draws %d, off their interval %d (worst edge distance %.3e), differing from the free reference %d"
          % (_id(i), draws, off, worst, differ))
    assert draws > 0 and worst <= EDGE_TOL, "a draw that is not on a CDF edge"
    rs_hip = filt["rs"].cpu() != 0
    assert torch.equal(rs_hip, r["ref"]["rs_f"]), "decisions differ from the reference's free-running ones"
    assert torch.equal(rs_hip, AR.decide(rep["ess"], tau, N))
    _assert_values(z, log, z_rep, rep)
    _check_ess(i, filt, rep)


@pytest.mark.parametrize("i", CASES, ids=_id)
def test_every_gradient(built_lib, i):
    """d log_ZSMC / d(every parameter), indices and decisions teacher-forced, against fp64 autograd of the reference; the
    never-observed output's column of the output layer, its bias and its scale are exactly 0.0"""
    r = _reference(i)
    case, model = MA.CASES[i], r["model"]
    e_never = r["mask"][2]
    z_ref, P = MA.oracle_grads(model, r["FLAGS"], case, r["obs"], r["noise"], r["teacher"])
    z, log = _run(model, r["smc"], r["obs"], _hip(r["noise"], r["teacher"]))
    assert torch.equal(log["filter"]["rs"].cpu() != 0, r["ref"]["rs_f"])
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    rows = []
    for name, p, ref in _pairs(model, P):
        g = torch.zeros_like(ref) if p.grad is None else p.grad.detach().double().cpu()
        want = torch.zeros_like(ref) if ref.grad is None else ref.grad
        assert torch.isfinite(g).all(), name
        rows.append((name, float((g - want).abs().max()), max(float(want.abs().max()), 1e-6)))
        if e_never is not None and name in ("g.Wmu", "g.bmu", "g.sigma"):
            assert p.grad is not None, name
            col = p.grad[e_never] if p.grad.dim() == 1 else p.grad[:, e_never]
            assert bool((col == 0.0).all()), (name, col)
            others = [e for e in range(case[5]) if e != e_never]
            if name != "g.sigma":
                live = p.grad[others] if p.grad.dim() == 1 else p.grad[:, others].abs().amax(0)
                assert bool((live.abs() > 0).all()), name
    names = {n for n, _, _ in rows}
    has_scale = not MA.is_count(case) and not case[9].get("poisson_emission")      # (the other two emissions have no scale vector)
    assert len(rows) > 8 and {"g.W0", "g.b0", "g.Wmu", "g.bmu"} <= names and ("g.sigma" in names) == has_scale
    worst = max(rows, key=lambda v: v[1] / v[2])
    print("%s: worst gradient error / largest entry: %s %.3e" % (_id(i), worst[0], worst[1] / worst[2]))
    bad = [v for v in rows if v[1] > 2e-3 * v[2] + 1e-6]
    assert not bad, "gradient mismatch (name, max abs err, largest entry): %s" % bad
    if case[0] == "SVO":
        assert any(n.startswith("y_smoother") and s > 1e-6 for n, _, s in rows)


# ---- semantics of the gap ----------------------------------------------------------------------------------------------------
def test_a_step_with_nothing_observed_is_kept(built_lib):
    """MA.GAP_CASE (bootstrap, no q2): the step with nothing observed follows a resampled step in both sequences; its ESS / N is
    1 within the margin and the sequence is kept"""
    i = MA.GAP_CASE
    r = _reference(i)
    t_all = r["mask"][1]
    with torch.no_grad():
        _, log = r["smc"].get_log_ZSMC(r["obs"].float().cuda(), None, noise=_hip(r["noise"]))
    torch.cuda.synchronize()
    rs, ess = log["filter"]["rs"].cpu(), log["filter"]["ess"].cpu()
    N = MA.CASES[i][3]
    assert bool(torch.isnan(r["obs"][:, t_all]).all())
    assert bool((rs[t_all - 1] == 1).all())
    print("gap step: ESS / N %s" % (ess[t_all] / N).tolist())
    assert float((ess[t_all].double() / N - 1.0).abs().max()) <= MARGIN
    assert bool((rs[t_all] == 0).all())


@pytest.mark.parametrize("i", CASES, ids=_id)
def test_all_ones_is_the_missing_kernel(built_lib, i):
    """decisions forced to all ones: psvo_filter_forward_wobs_missing on the same inputs -- bit for bit for the count cases; the
    Gaussian cases agree in their draws and in logW within one ulp"""
    case = MA.CASES[i]
    T, B = case[2], case[1]
    r = _reference(i)
    _, model_m, smc_m, obs_m, noise_m, _ = MA.setup(case, "cuda", resample_ess=0.0)
    assert smc_m.missing_obs and smc_m.resample_ess == 0.0
    assert torch.equal(torch.nan_to_num(obs_m, nan=-7.0), torch.nan_to_num(r["obs"], nan=-7.0))
    ones = torch.ones(T, B, dtype=torch.int32)
    with torch.no_grad():
        _, log_a = r["smc"].get_log_ZSMC(r["obs"].float().cuda(), None, noise=_hip(r["noise"], {"rs_f": ones}))
        _, log_m = smc_m.get_log_ZSMC(obs_m.float().cuda(), None, noise=_hip(noise_m))
    torch.cuda.synchronize()
    fa, fm = log_a["filter"], log_m["filter"]
    assert bool((fa["rs"] == 1).all())
    assert torch.equal(fa["idx"], fm["idx"])
    if MA.is_count(case):
        for k in ("X", "Xanc", "Fm", "logW", "lse"):
            assert torch.equal(fa[k], fm[k]), k
    else:
        ulp = 2.0 ** -23 * torch.maximum(fa["logW"].abs(), fm["logW"].abs())
        d = (fa["logW"] - fm["logW"]).abs()
        print("%s: logW differs in %d of %d entries, worst %.3e" % (_id(i), int((d > 0).sum()), d.numel(), float(d.max())))
        assert bool((d <= ulp).all())


@pytest.mark.parametrize("i", [i for i in COUNT_CASES if MA.CASES[i][5] >= 3], ids=_id)
def test_nothing_missing_count_is_the_wide_adaptive_kernel(built_lib, i):
    """no NaN in obs: the count form equals psvo_filter_forward_wobs_adaptive bit for bit (Dy >= 3)"""
    case = MA.CASES[i]
    FLAGS, model, smc, obs, noise, _ = MA.setup(case, "cuda", knock=False)
    assert smc.missing_obs and not bool(torch.isnan(obs).any())
    _, model_w, smc_w, _, noise_w = AR.setup(case[:11], "cuda", resample_ess=case[11], resample_ess_wide_obs=True)
    assert smc_w.wide_obs and not smc_w.missing_obs and smc_w.resample_ess == case[11]
    assert torch.equal(obs, CR.counts(case[1], case[2], case[5], 100 + case[10]).double())
    with torch.no_grad():
        _, log_a = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise))
        _, log_w = smc_w.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise_w))
    torch.cuda.synchronize()
    for k in ("X", "Xanc", "Fm", "logW", "lse", "idx", "rs", "ess"):
        assert torch.equal(log_a["filter"][k], log_w["filter"][k]), k
    assert 0 < int(log_a["filter"]["rs"].sum()) < case[1] * case[2]


# ---- reproducibility and integration -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 5, 6], ids=_id)
def test_two_passes_are_bit_identical(built_lib, i):
    """forward + reverse twice in one process: the ELBO, the decisions, ESS and every .grad bit for bit"""
    case = MA.CASES[i]
    FLAGS, model, smc, obs, noise, _ = MA.setup(case, "cuda")
    nz = _hip(noise)
    res = []
    for _ in range(2):
        z, log = _run(model, smc, obs, nz)
        res.append((z, log["filter"]["rs"].clone(), log["filter"]["ess"].clone(), _grads(model)))
    a, b = res
    assert torch.isfinite(a[0]) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[3].keys() == b[3].keys() and len(a[3]) > 4
    for n, g in a[3].items():
        assert torch.isfinite(g).all() and torch.equal(g, b[3][n]), n


def test_step_replays_from_hipgraph(built_lib):
    """one local training step of case 3, eager and captured into a GraphedStep: the decision is made on the device, so the
    capture holds the whole step and a replay equals the eager step bit for bit; the obs buffer carries the NaNs"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    FLAGS, model, smc, obs, noise, _ = MA.setup(MA.CASES[3], "cuda")
    nz = _hip(noise)
    flat = FlatParams(model)
    obs_c = obs.float().cuda()
    assert bool(torch.isnan(obs_c).any())
    seen = {}

    def local():
        flat.zero_grad()
        z, log = smc.get_log_ZSMC(obs_c, None, noise=nz)
        z.backward()
        seen["rs"] = log["filter"]["rs"]
        return z.detach()
    z_e = local().clone()
    g_e, rs_e = flat.grad.clone(), seen["rs"].clone()
    torch.cuda.synchronize()
    assert torch.isfinite(z_e) and torch.isfinite(g_e).all() and float(g_e.abs().max()) > 0
    assert 0 < int(rs_e.sum()) < rs_e.numel()
    step = GraphedStep(local)
    for _ in range(2):
        flat.grad.fill_(float("nan"))
        z_g = step()
        torch.cuda.synchronize()
        assert torch.equal(z_g, z_e)
        assert torch.equal(flat.grad, g_e)


@pytest.mark.parametrize("i", [1, 6], ids=_id)
def test_ffbs_and_ffbsi_behind_it(built_lib, i):
    """--FFBS --FFBSi under no_grad behind the adaptive missing-observation filter: they read X, Fm and logW only, so the filter
    is untouched, everything they return is finite and log["Xs"] holds no NaN"""
    case = MA.CASES[i]
    FLAGS, model, smc, obs, noise, _ = MA.setup(case, "cuda", FFBS=True, FFBSi=True)
    assert smc.FFBS and smc.FFBSi and smc.missing_obs and smc.resample_ess == case[11]
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise))
        _, plain = _reference(i)["smc"].get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise))
    torch.cuda.synchronize()
    assert torch.isfinite(z) and torch.equal(log["filter"]["logW"], plain["filter"]["logW"])
    assert torch.equal(log["filter"]["rs"], plain["filter"]["rs"]) and 0 < int(log["filter"]["rs"].sum()) < case[1] * case[2]
    for key in ("Xs", "Xs_filter", "Xs_marginal", "X_smooth_mean", "ess_smooth", "logW_smooth", "path_logq"):
        assert torch.isfinite(log[key]).all(), key
    B, T, N, Dx = case[1], case[2], case[3], case[4]
    assert log["Xs"].shape == (B, T, N, Dx) and int(log["path_distinct"].min()) >= 1


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """two epochs on the Lorenz slice with gaps through psvo_amd.runner with --missing_obs --resample_ess=0.5
    --resample_ess_missing_obs: finite history and R^2 (asserted by _run_main), the adaptive_* and missing_share_* keys in every
    metric_<iter>.p"""
    data = _lorenz_with_gaps()
    FLAGS, hist, work = _run_main(tmp_path, monkeypatch, "gaps_adaptive", data,
                                  ["--AESMC", "--missing_obs", "--resample_ess=0.5", "--resample_ess_missing_obs",
                                   "--n_particles=32", "--batch_size=4"], 3, 10)
    assert FLAGS.missing_obs and FLAGS.resample_ess == 0.5 and (FLAGS.n_train, FLAGS.n_test, FLAGS.time) == (8, 4, 100)
    metrics = glob.glob(str(work / "rslts" / "**" / "metric_*.p"), recursive=True)
    assert len(metrics) >= 2
    for path in metrics:
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        for split, key in (("train", "Ytrain"), ("test", "Yvalid")):
            assert m["missing_share_" + split] == pytest.approx(float(np.isnan(data[key]).mean()), abs=1e-12)
            assert 0.0 <= m["adaptive_rate_" + split] <= 1.0
            assert 1.0 / 32 - 1e-6 <= m["adaptive_ess_min_" + split] <= m["adaptive_ess_mean_" + split] <= 1.0 + 1e-5
    rates = [pickle.load(open(p, "rb"))["adaptive_rate_train"] for p in metrics]
    assert 0.0 < float(np.mean(rates)) < 1.0, rates          # some steps resampled and some kept
