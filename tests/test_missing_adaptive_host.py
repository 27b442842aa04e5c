"""Host side of adaptive resampling and the particle forecast on missing observations (FLAGS.resample_ess_missing_obs,
FLAGS.particle_forecast_missing_obs): flags, routing, refusals, the trainer's forecast metrics on gappy targets, and the fp64
reference of tests/missing_adaptive_reference.py on the cases of tests/test_gpu_missing_adaptive.py.  No GPU."""
import math

import numpy as np
import pytest
import torch

from tests import adaptive_reference as AR
from tests import helpers as Hh
from tests import missing_adaptive_reference as MA
from tests import missing_reference as MR

BOTH = dict(missing_obs=True, resample_ess=0.5, resample_ess_missing_obs=True)


def _objective(obj, **kw):
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.IWAE import IWAE
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.SMC.PSVOwR import PSVOwR
    from psvo_amd.SMC.SVO import SVO
    FLAGS = Hh.make_flags(obj, **kw)
    model = SSM(FLAGS)
    return FLAGS, model, {"AESMC": AESMC, "IWAE": IWAE, "PSVO": PSVO, "PSVOwR": PSVOwR, "SVO": SVO}[obj](model, FLAGS)


def test_flag_parsing_and_default():
    from psvo_amd.flags import Flags, parse_flags
    for name in ("resample_ess_missing_obs", "particle_forecast_missing_obs"):
        assert getattr(Flags(), name) is False and getattr(parse_flags([]), name) is False
        assert getattr(parse_flags(["--" + name]), name) is True and getattr(parse_flags(["--no" + name]), name) is False
        assert name in Flags().as_dict()
    F = parse_flags(["--noPSVO", "--AESMC", "--missing_obs", "--resample_ess=0.5", "--resample_ess_missing_obs",
                     "--particle_forecast", "--particle_forecast_missing_obs"])
    assert F.missing_obs and F.resample_ess == 0.5 and F.resample_ess_missing_obs and F.particle_forecast_missing_obs


def test_routing():
    from psvo_amd import _lib, autograd, ops
    assert hasattr(autograd, "FilterWobsMissingAdaptiveFunction")
    assert hasattr(ops, "filter_forward_wobs_missing_adaptive") and hasattr(ops, "filter_backward_wobs_missing_adaptive")
    assert ops._ADAPTIVE_ENTRY["psvo_filter_forward_wobs_missing_adaptive"] == "psvo_filter_forward_wobs_missing_adaptive"
    assert "psvo_filter_forward_wobs_missing" not in ops._ADAPTIVE_ENTRY and "psvo_filter_forward_wobs" not in ops._ADAPTIVE_ENTRY
    for name in ("psvo_filter_forward_wobs_missing_adaptive", "psvo_filter_backward_wobs_missing_adaptive",
                 "psvo_particle_forecast_missing"):
        assert name in _lib.SIGNATURES
    for obj in ("AESMC", "SVO"):
        for Dy in (1, 2, 3, 10, 32):                                  # every width, without --resample_ess_wide_obs
            smc = _objective(obj, Dy=Dy, Dx=3, **BOTH)[2]
            assert smc.missing_obs and smc.resample_ess == 0.5 and not smc.wide_obs and smc.resample_particles is True
        smc = _objective(obj, Dy=10, Dx=3, resample_ess_wide_obs=True, **BOTH)[2]       # ... which has no effect there
        assert smc.missing_obs and smc.resample_ess == 0.5 and not smc.wide_obs
        # the flag has no effect without --missing_obs or with the threshold off
        smc = _objective(obj, Dy=1, resample_ess=0.5, resample_ess_missing_obs=True)[2]
        assert not smc.missing_obs and smc.resample_ess == 0.5
        smc = _objective(obj, Dy=10, Dx=3, missing_obs=True, resample_ess_missing_obs=True)[2]
        assert smc.missing_obs and smc.resample_ess == 0.0
    for kw in (dict(poisson_emission=True), dict(count_emission=True)):               # every emission form
        for Dy in (1, 2, 5):
            smc = _objective("AESMC", Dy=Dy, **kw, **BOTH)[2]
            assert smc.missing_obs and smc.resample_ess == 0.5
    smc = _objective("AESMC", Dy=2, FFBS=True, FFBSi=True, **BOTH)[2]                 # the smoothers stay available behind it
    assert smc.FFBS and smc.FFBSi and smc.resample_ess == 0.5
    # the forecast
    for obj in ("AESMC", "SVO", "IWAE"):
        smc = _objective(obj, Dy=10, Dx=3, missing_obs=True, particle_forecast=True, particle_forecast_missing_obs=True)[2]
        assert smc.missing_obs and smc.forecast and smc.forecast_missing
        smc = _objective(obj, Dy=10, Dx=3, particle_forecast=True, particle_forecast_missing_obs=True)[2]
        assert smc.forecast and not smc.forecast_missing and not smc.missing_obs
    smc = _objective("AESMC", Dy=3, particle_forecast=True, particle_forecast_missing_obs=True, **BOTH)[2]
    assert smc.forecast_missing and smc.resample_ess == 0.5


@pytest.mark.parametrize("obj,kw,word", [
    # the pinned refusals, unchanged without the new flags
    ("AESMC", dict(Dy=1, resample_ess=0.5), r"--missing_obs with --resample_ess"),
    ("SVO", dict(Dy=10, Dx=3, resample_ess=0.5, resample_ess_wide_obs=True), r"--missing_obs with --resample_ess"),
    ("AESMC", dict(Dy=3, particle_forecast=True), r"--missing_obs with --particle_forecast.*lpd.*whole observation rows"),
    # one flag does not switch the other combination on
    ("AESMC", dict(Dy=1, resample_ess=0.5, particle_forecast_missing_obs=True), r"--missing_obs with --resample_ess"),
    ("AESMC", dict(Dy=3, particle_forecast=True, resample_ess_missing_obs=True), r"--missing_obs with --particle_forecast"),
    # still refused with the flags, by name
    ("IWAE", dict(Dy=3, resample_ess=0.5, resample_ess_missing_obs=True), r"--resample_ess with --IWAE.*never resamples"),
    ("PSVO", dict(Dy=1, resample_ess=0.5, resample_ess_missing_obs=True), r"--missing_obs with --PSVO / --PSVOwR"),
    ("PSVOwR", dict(Dy=1, resample_ess=0.5, resample_ess_missing_obs=True), r"--missing_obs with --PSVO / --PSVOwR"),
    ("PSVO", dict(Dy=1, particle_forecast=True, particle_forecast_missing_obs=True), r"--missing_obs with --PSVO / --PSVOwR"),
    ("AESMC", dict(Dy=1, output_cov=True, diag_cov=True, resample_ess=0.5, resample_ess_missing_obs=True),
     r"--missing_obs with output_cov"),
    ("AESMC", dict(Dy=1, q1_layers="32,32", g_layers="32,32", resample_ess=0.5, resample_ess_missing_obs=True),
     r"--missing_obs with per-particle MLP layers.*one hidden layer"),
    ("SVO", dict(Dy=10, Dx=3, g_layers="16,16", particle_forecast=True, particle_forecast_missing_obs=True),
     r"--missing_obs with per-particle MLP layers.*one hidden layer"),
    ("AESMC", dict(Dy=33, Dx=3, resample_ess=0.5, resample_ess_missing_obs=True), r"--missing_obs with Dy = 33.*1 <= Dy <= 32"),
    ("AESMC", dict(Dy=1, resample_ess=1.5, resample_ess_missing_obs=True), r"--resample_ess = 1\.5.*0 < tau <= 1"),
], ids=["ess-pinned", "ess-wide-pinned", "forecast-pinned", "ess-other-flag", "forecast-other-flag", "IWAE", "PSVO", "PSVOwR",
        "PSVO-forecast", "output_cov", "two-layers", "two-layers-forecast", "Dy33", "above-1"])
def test_refusals(obj, kw, word):
    with pytest.raises(ValueError, match=word):
        _objective(obj, missing_obs=True, **kw)


def test_the_checks_name_every_limit():
    """the checks runner.main makes on the flags alone; the new keyword parameters default to off"""
    from psvo_amd.SMC.SVO import check_missing_obs, check_resample_ess
    ok = dict(Dy=10, layers=["32", "32"])
    with pytest.raises(ValueError, match="--missing_obs with --resample_ess"):
        check_missing_obs(True, resample_ess=0.5, **ok)
    with pytest.raises(ValueError, match="--missing_obs with --particle_forecast"):
        check_missing_obs(True, particle_forecast=True, **ok)
    assert check_missing_obs(True, resample_ess=0.5, resample_ess_missing_obs=True, **ok) is True
    assert check_missing_obs(True, particle_forecast=True, particle_forecast_missing_obs=True, **ok) is True
    assert check_missing_obs(False, resample_ess=0.5, resample_ess_missing_obs=True, **ok) is False
    for kw, word in ((dict(ok, backward_simulation=True), "--PSVO / --PSVOwR"), (dict(ok, output_cov=True), "output_cov"),
                     (dict(ok, layers=["32", "32,32"]), "one hidden layer"), (dict(ok, Dy=33), r"1 <= Dy <= 32")):
        with pytest.raises(ValueError, match=word):
            check_missing_obs(True, resample_ess=0.5, particle_forecast=True, resample_ess_missing_obs=True,
                              particle_forecast_missing_obs=True, **kw)
    assert check_resample_ess(0.5, Dy=10, missing_obs=True) == 0.5 and check_resample_ess(0.5, Dy=1, missing_obs=True) == 0.5
    with pytest.raises(ValueError, match="--resample_ess_wide_obs"):
        check_resample_ess(0.5, Dy=10)
    for kw, word in ((dict(never_resamples=True), "--IWAE"), (dict(backward_simulation=True), "--PSVO / --PSVOwR"),
                     (dict(output_cov=True), "output_cov")):
        with pytest.raises(ValueError, match=word):
            check_resample_ess(0.5, Dy=10, missing_obs=True, **kw)


def test_runner_checks_before_it_touches_a_device(monkeypatch):
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags

    def unreachable(*a, **k):
        raise AssertionError("runner.main went on after a refusal")
    monkeypatch.setattr(runner, "_device", unreachable)
    monkeypatch.setattr(runner, "_dataset", unreachable)
    gaps = ["--noPSVO", "--AESMC", "--missing_obs"]
    ess = ["--resample_ess=0.5", "--resample_ess_missing_obs"]
    fc = ["--particle_forecast", "--particle_forecast_missing_obs"]
    for argv, word in ((gaps + ["--resample_ess=0.5"], "--missing_obs with --resample_ess"),
                       (gaps + ["--particle_forecast"], "--missing_obs with --particle_forecast"),
                       (gaps + ["--resample_ess=0.5", "--particle_forecast_missing_obs"], "--missing_obs with --resample_ess"),
                       (["--noPSVO", "--IWAE", "--missing_obs"] + ess, "--IWAE"),
                       (["--missing_obs"] + ess, "--PSVO / --PSVOwR"),
                       (["--noPSVO", "--PSVOwR", "--missing_obs"] + fc, "--PSVO / --PSVOwR"),
                       (gaps + ess + ["--output_cov", "--diag_cov"], "output_cov"),
                       (gaps + ess + ["--g_layers=32,32"], "one hidden layer"),
                       (gaps + fc + ["--q1_layers=32,32"], "one hidden layer"),
                       (gaps + ess + ["--Dx=3", "--Dy=33"], "1 <= Dy <= 32")):
        with pytest.raises(ValueError, match=word):
            runner.main(parse_flags(argv))

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(runner, "_device", reached)
    for argv in (gaps + ess, gaps + ess + ["--Dx=3", "--Dy=10"], gaps + ess + ["--Dx=3", "--Dy=32", "--FFBS", "--FFBSi"],
                 ["--noPSVO", "--SVO", "--missing_obs", "--Dy=2"] + ess + fc, gaps + fc + ["--Dx=3", "--Dy=10"],
                 gaps + ess + ["--generateTrainingData", "--count_emission", "--Dy=2", "--missing_rate=0.3"]):
        with pytest.raises(Reached):
            runner.main(parse_flags(argv))


# ---- the trainer's forecast metrics ------------------------------------------------------------------------------------------

def test_forecast_metrics_by_hand():
    """a (3 sequences, 4 steps, K = 5, 2 outputs) forecast against sums written out entry by entry: one fully missing target row,
    one never-observed output, horizons with no observed target (NaN)"""
    from psvo_amd.trainer import _forecast_metrics, _r_square
    rng = np.random.RandomState(5)
    n, T, K1, Dy = 3, 4, 6, 2
    obs = rng.randn(n, T, Dy)
    y_mean = rng.randn(n, T, K1, Dy)
    y_var = 0.5 + rng.rand(n, T, K1, Dy)
    lpd = rng.randn(n, T, K1)
    full = _forecast_metrics(y_mean, y_var, lpd, obs)
    assert len(full) == 3 and all(a.shape == (K1,) for a in full)
    assert np.isnan(full[0][4:]).all() and np.isfinite(full[0][:4]).all()             # K >= T: no pair
    for k in range(4):
        assert full[0][k] == pytest.approx(np.mean(lpd[:, :T - k, k]), rel=1e-12)
        assert full[2][k] == pytest.approx(np.mean(np.square(obs[:, k:] - y_mean[:, :T - k, k]) / y_var[:, :T - k, k]), rel=1e-12)
    # nothing missing: the masked form gives the same three numbers and lpd per entry = mean lpd / Dy
    same = _forecast_metrics(y_mean, y_var, lpd, obs, missing_obs=True)
    assert len(same) == 4
    for a, b in zip(full, same[:3]):
        assert np.allclose(a[:4], b[:4], rtol=1e-12, atol=0) and np.isnan(b[4:]).all()
    assert np.allclose(same[3][:4], full[0][:4] / Dy, rtol=1e-12, atol=0)
    gaps = obs.copy()
    gaps[:, :, 1] = np.nan              # a never-observed output
    gaps[1, 2, :] = np.nan              # a fully missing target row
    gaps[:, 3, :] = np.nan              # the last step observed by nobody: horizon 3 has no observed target
    lp, rsq, cal, per = _forecast_metrics(y_mean, y_var, lpd, gaps, missing_obs=True)
    assert math.isnan(lp[3]) and math.isnan(rsq[3]) and math.isnan(cal[3]) and math.isnan(per[3]) and np.isnan(lp[4:]).all()
    for k in range(3):
        s = c = ent = 0.0
        pairs = entries = 0
        for i in range(n):
            for t in range(T - k):
                seen = [e for e in range(Dy) if not math.isnan(gaps[i, t + k, e])]
                if not seen:
                    continue
                pairs += 1
                s += lpd[i, t, k]
                for e in seen:
                    entries += 1
                    c += (gaps[i, t + k, e] - y_mean[i, t, k, e]) ** 2 / y_var[i, t, k, e]
        assert pairs > 0 and entries == pairs          # (one observed output)
        assert lp[k] == pytest.approx(s / pairs, rel=1e-12)
        assert per[k] == pytest.approx(s / entries, rel=1e-12)
        assert cal[k] == pytest.approx(c / entries, rel=1e-12)
        assert rsq[k] == pytest.approx(_r_square(y_mean[:, :T - k, k], gaps[:, k:], True), rel=1e-12) and math.isfinite(rsq[k])
    # rows of different completeness: the score per entry is not the mean over pairs divided by anything fixed
    ragged = obs.copy()
    ragged[0, :, 1] = np.nan
    lp, _, _, per = _forecast_metrics(y_mean, y_var, lpd, ragged, missing_obs=True)
    assert lp[0] == pytest.approx(np.mean(lpd[:, :, 0]), rel=1e-12)
    assert per[0] == pytest.approx(np.sum(lpd[:, :, 0]) / (n * T * Dy - T), rel=1e-12)
    # without the argument a NaN target is a NaN, as before
    assert math.isnan(_forecast_metrics(y_mean, y_var, lpd, gaps)[2][0])


# ---- the reference against its parts, fp64 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("i", [0, 6], ids=lambda i: MA.case_id(MA.CASES[i]))
def test_reference_reduces_to_its_parts(i):
    """nothing missing: adaptive_reference's objective (with the count emission for the count case); decisions forced to all
    ones: missing_reference's resampling objective; all zeros: that objective without resampling"""
    from oracle import psvo_oracle as O
    from tests import count_reference as CR
    case = MA.CASES[i]
    obj, B, T = case[0], case[1], case[2]
    FLAGS, model, smc, obs, noise, _ = MA.setup(case)
    P = model.export_reference_layout(torch.float64)
    ones, zeros = torch.ones(T, B, dtype=torch.long), torch.zeros(T, B, dtype=torch.long)
    with torch.no_grad():
        # (1) nothing missing
        dense = MA.setup(case, knock=False)[3]
        z_a, log_a = MA.objective(P, FLAGS, case).get_log_ZSMC(dense, noise)
        plain = AR.objective(P, FLAGS, obj)
        if MA.is_count(case):
            plain.g = CR.CountEmission(P["g"])
        z_p, log_p = plain.get_log_ZSMC(dense, noise)
        assert torch.equal(log_a["rs_f"], log_p["rs_f"]) and torch.equal(log_a["idx_f"], log_p["idx_f"])
        assert float((log_a["log_Ws"] - log_p["log_Ws"]).abs().max()) <= 1e-10 and abs(float(z_a) - float(z_p)) <= 1e-10
        assert float((log_a["ess"] - log_p["ess"]).abs().max()) <= 1e-9
        # (2) all ones / all zeros on the gappy data
        z1, log1 = MA.objective(P, FLAGS, case).get_log_ZSMC(obs, {**noise, "rs_f": ones})
        z_m, log_m = MR.objective(P, FLAGS, obj).get_log_ZSMC(obs, noise)
        z0, log0 = MA.objective(P, FLAGS, case).get_log_ZSMC(obs, {**noise, "rs_f": zeros})
        never = O.OracleIWAE(P, Hh.oracle_flags(FLAGS, obj)) if obj == "AESMC" else O.OracleSVO(P, Hh.oracle_flags(FLAGS, obj),
                                                                                                resample_particles=False)
        never.g = MR.MissingEmission(CR.CountEmission(P["g"]) if MA.is_count(case) else never.g)
        pre = never.preprocess_obs
        never.preprocess_obs = lambda o: pre(MR.zero_filled(o))
        z_n, log_n = never.get_log_ZSMC(obs, noise)
    assert torch.equal(z1, z_m)
    for k in ("Xs", "X_prevs", "X_ancestors", "log_Ws", "idx_f"):
        assert torch.equal(log1[k], log_m[k]), k
    assert torch.equal(z0, z_n) and torch.equal(log0["log_Ws"], log_n["log_Ws"]) and torch.equal(log0["X_prevs"], log_n["X_prevs"])
    assert not torch.equal(z1, z0) and torch.isfinite(z1) and torch.isfinite(z0)


def test_the_gpu_cases_meet_their_conditions():
    """the cases of tests/test_gpu_missing_adaptive.py on the fp64 reference alone, free running: the resampling rate of each
    lies in [0.1, 0.9], no ESS / N comes closer to the threshold than 100 x the GPU's ESS tolerance, |ELBO| >= 1, the mask is the
    pattern tests/test_gpu_missing.py::_missing asserts, and the fp32 reference's ESS (same draws and decisions) stays within
    ESS_GAP32_MISSING of N -- the figure the GPU tolerance is 4 x of"""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    worst = 0.0
    for case in MA.CASES:
        FLAGS, model, smc, obs, noise, (miss, t_all, e_never) = MA.setup(case)
        B, T, N, Dy, tau = case[1], case[2], case[3], case[5], case[11]
        assert smc.resample_ess == tau and smc.missing_obs and not smc.wide_obs and FLAGS.resample_ess_missing_obs
        # the mask pattern
        assert torch.equal(torch.isnan(obs), miss) and torch.equal(miss, MR.mask(B, T, Dy, case[10])[0])
        assert bool(miss[:, t_all].all()) and (e_never is None) == (Dy == 1)
        rest = [e for e in range(Dy) if e != e_never]
        assert e_never is None or bool(miss[:, :, e_never].all())
        assert not bool(miss[0, 0, rest].any())
        if B == 2:
            assert bool(miss[1, T - 2:].all())
        assert 1.0 - float(miss.float().mean()) >= (0.5 if B == 1 else 0.2)
        if MA.is_count(case):
            seen = obs[~miss]
            assert float(seen.min()) >= 0.0 and torch.equal(seen, seen.floor())
        z, ref = MA.run_oracle(model, FLAGS, case, obs, noise)
        rate = float(ref["rs_f"].double().mean())
        closest = float((ref["ess"] / N - tau).abs().min())
        teacher = {"idx_f": ref["idx_f"], "rs_f": ref["rs_f"].long()}
        _, r32 = MA.run_oracle(model, FLAGS, case, obs, noise, teacher=teacher, dtype=torch.float32)
        gap = float((r32["ess"].double() - ref["ess"]).abs().max()) / N
        print("%s: tau %.2f rate %.3f, ESS / N in [%.3f, %.3f], closest to tau %.2e, |ESS32 - ESS64| / N %.3e, ELBO %.3f"
              % (MA.case_id(case), tau, rate, float(ref["ess"].min()) / N, float(ref["ess"].max()) / N, closest, gap, float(z)))
        assert 0.1 <= rate <= 0.9, (MA.case_id(case), rate)
        assert closest >= 100 * 4 * MA.ESS_GAP32_MISSING, (MA.case_id(case), closest)
        assert abs(float(z)) >= 1.0, (MA.case_id(case), float(z))
        assert torch.equal(AR.decide(ref["ess"], tau, N), ref["rs_f"])
        worst = max(worst, gap)
    # the recorded figure is this measurement, rounded up (slack for another host's fp32 summation order; the GPU tolerance is
    # 4 x the RECORDED figure whatever is measured here)
    assert 0.25 * MA.ESS_GAP32_MISSING <= worst <= 1.5 * MA.ESS_GAP32_MISSING, worst


def test_the_gap_step_of_a_bootstrap_filter_is_kept():
    """MA.GAP_CASE (bootstrap, no q2): the step with nothing observed follows a resampled step in both sequences; its weights are
    then f / q = 1 for every particle, ESS / N = 1 and the sequence is kept"""
    case = MA.CASES[MA.GAP_CASE]
    FLAGS, model, smc, obs, noise, (miss, t_all, _) = MA.setup(case)
    assert case[7] and not case[8] and bool(miss[:, t_all].all())
    _, ref = MA.run_oracle(model, FLAGS, case, obs, noise)
    assert bool(ref["rs_f"][t_all - 1].all())
    assert float((ref["ess"][t_all] / case[3] - 1.0).abs().max()) <= 1e-12
    assert not bool(ref["rs_f"][t_all].any())
