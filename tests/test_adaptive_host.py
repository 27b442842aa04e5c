"""Host side of adaptive resampling (FLAGS.resample_ess): flag, routing, refusals, and the fp64 reference of
tests/adaptive_reference.py against the unmodified oracle at its two ends and on the cases of tests/test_gpu_adaptive.py.  No GPU."""
import pytest
import torch

from oracle import psvo_oracle as O
from tests import adaptive_reference as AR
from tests import helpers as Hh


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
    assert Flags().resample_ess == 0.0 and isinstance(Flags().resample_ess, float)
    assert parse_flags([]).resample_ess == 0.0
    F = parse_flags(["--AESMC", "--resample_ess=0.5"])
    assert F.resample_ess == 0.5 and F.AESMC
    assert parse_flags(["--resample_ess", "0.25"]).resample_ess == 0.25
    assert "resample_ess" in Flags().as_dict()
    with pytest.raises(ValueError):
        parse_flags(["--resample_ess=half"])


def test_routing():
    from psvo_amd import autograd, ops
    assert hasattr(autograd, "FilterAdaptiveFunction")
    for obj in ("AESMC", "SVO"):
        assert _objective(obj)[2].resample_ess == 0.0                      # off by default: today's path
        for tau in (0.5, 1.0, 1e-3):
            smc = _objective(obj, resample_ess=tau)[2]
            assert smc.resample_ess == tau and smc.resample_particles is True
    # the other objectives are untouched with the flag off
    for obj in ("IWAE", "PSVO", "PSVOwR"):
        assert _objective(obj)[2].resample_ess == 0.0
    assert _objective("AESMC", resample_ess=0.5, FFBS=True, FFBSi=True)[2].FFBS          # the smoothers stay available behind it
    # the descriptor is the static one: the threshold travels as an argument of the adaptive entry points
    smc = _objective("AESMC", resample_ess=0.5)[2]
    smc.batch_size, smc.time = 2, 5
    assert smc._make_desc(1, 32).resample == 1
    import inspect
    assert {"ess_frac", "rs_in"} <= set(inspect.signature(ops.filter_forward).parameters)
    assert "adaptive" in inspect.signature(ops.filter_backward).parameters


@pytest.mark.parametrize("obj,kw,word", [
    ("AESMC", dict(resample_ess=1.5), r"--resample_ess = 1\.5.*0 < tau <= 1"),
    ("AESMC", dict(resample_ess=-0.1), r"--resample_ess = -0\.1.*0 < tau <= 1"),
    ("SVO", dict(resample_ess=float("nan")), r"0 < tau <= 1"),
    ("IWAE", dict(resample_ess=0.5), r"--resample_ess with --IWAE.*never resamples"),
    ("PSVO", dict(resample_ess=0.5), r"--resample_ess with --PSVO / --PSVOwR.*filter objectives"),
    ("PSVOwR", dict(resample_ess=0.5), r"--resample_ess with --PSVO / --PSVOwR"),
    ("AESMC", dict(resample_ess=0.5, output_cov=True, diag_cov=True), r"--resample_ess with output_cov.*no adaptive form"),
    ("AESMC", dict(resample_ess=0.5, Dy=3), r"--resample_ess with Dy = 3.*Dy <= 2"),
    ("SVO", dict(resample_ess=0.5, Dy=10, Dx=3), r"--resample_ess with Dy = 10.*Dy <= 2"),
], ids=["above-1", "negative", "nan", "IWAE", "PSVO", "PSVOwR", "output_cov", "Dy3", "Dy10"])
def test_refusals(obj, kw, word):
    with pytest.raises(ValueError, match=word):
        _objective(obj, **kw)


def test_runner_refuses_before_it_touches_a_device(monkeypatch):
    """runner.main checks the flags first: no device, no data set, no model is reached"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags

    def unreachable(*a, **k):
        raise AssertionError("runner.main went on after a refusal")
    monkeypatch.setattr(runner, "_device", unreachable)
    monkeypatch.setattr(runner, "_dataset", unreachable)
    for argv, word in ((["--noPSVO", "--AESMC", "--resample_ess=2"], "0 < tau <= 1"),
                       (["--noPSVO", "--IWAE", "--resample_ess=0.5"], "--IWAE"),
                       (["--resample_ess=0.5"], "--PSVO / --PSVOwR"),                          # (PSVO is the default objective)
                       (["--noPSVO", "--PSVOwR", "--resample_ess=0.5"], "--PSVO / --PSVOwR"),
                       (["--noPSVO", "--SVO", "--resample_ess=0.5", "--output_cov", "--diag_cov"], "output_cov"),
                       (["--noPSVO", "--AESMC", "--resample_ess=0.5", "--Dy=5"], "Dy = 5")):
        with pytest.raises(ValueError, match=word):
            runner.main(parse_flags(argv))


def _ends_case(obj):
    FLAGS, model, smc = _objective(obj, Dx=2, Dy=1, n_particles=12, batch_size=3, time=7, q0_layers="16", q1_layers="16",
                                   q2_layers="16", f_layers="16", g_layers="16", y_smoother_Dhs="8", X0_smoother_Dhs="8",
                                   resample_ess=0.5)
    torch.manual_seed(2)
    Hh.perturb_(model)
    g = torch.Generator().manual_seed(5)
    obs = torch.randn(3, 7, 1, generator=g, dtype=torch.float64)
    noise = O.make_noise(Hh.oracle_flags(FLAGS, obj), 3, 7, seed=9)
    return FLAGS, model, obs, noise


@pytest.mark.parametrize("obj", ["AESMC", "SVO"])
def test_reference_ends_are_the_oracle(obj):
    """forced all-ones decisions: the unmodified oracle objective, bit for bit; forced all-zeros: OracleIWAE's weights (for SVO:
    the oracle's own SMC with resampling switched off -- IWAE is AESMC's wiring without resampling)"""
    FLAGS, model, obs, noise = _ends_case(obj)
    P = model.export_reference_layout(torch.float64)
    fl = Hh.oracle_flags(FLAGS, obj)
    ones, zeros = torch.ones(7, 3, dtype=torch.long), torch.zeros(7, 3, dtype=torch.long)
    with torch.no_grad():
        z1, log1 = AR.objective(P, FLAGS, obj).get_log_ZSMC(obs, {**noise, "rs_f": ones})
        z_o, log_o = O.OBJECTIVES[obj](P, fl).get_log_ZSMC(obs, noise)
        z0, log0 = AR.objective(P, FLAGS, obj).get_log_ZSMC(obs, {**noise, "rs_f": zeros})
        never = O.OracleIWAE(P, fl) if obj == "AESMC" else O.OracleSVO(P, fl, resample_particles=False)
        z_n, log_n = never.get_log_ZSMC(obs, noise)
    assert torch.equal(z1, z_o)
    for k in ("Xs", "X_prevs", "X_ancestors", "log_Ws", "idx_f"):
        assert torch.equal(log1[k], log_o[k]), k
    assert bool(log1["rs_f"].all()) and not bool(log0["rs_f"].any())
    assert torch.equal(z0, z_n)
    assert torch.equal(log0["log_Ws"], log_n["log_Ws"]) and torch.equal(log0["X_prevs"], log_n["X_prevs"])
    # ... while the draw is still made and returned at every step
    assert log0["idx_f"].shape == (7, 12, 3)
    for t in range(7):
        assert torch.equal(log0["X_ancestors"][t], O.gather_particles(log0["X_prevs"][t], log0["idx_f"][t]))
    assert not torch.equal(z1, z0)
    # the thresholds that force the same: above 1 always resamples, a tiny one never does
    with torch.no_grad():
        za, loga = AR.objective(P, FLAGS, obj, ess_frac=2.0).get_log_ZSMC(obs, noise)
        zn, logn = AR.objective(P, FLAGS, obj, ess_frac=1e-9).get_log_ZSMC(obs, noise)
    assert torch.equal(za, z1) and bool(loga["rs_f"].all()) and torch.equal(zn, z0) and not bool(logn["rs_f"].any())


def test_reference_definitions():
    lw = torch.log(torch.tensor([[0.5, 1.0], [0.5, 0.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64))
    ess = AR.ess_of(lw)
    assert torch.allclose(ess, torch.tensor([2.0, 1.0], dtype=torch.float64), rtol=1e-14)
    assert AR.decide(ess, 0.4, 4).tolist() == [False, True]               # 2 >= 1.6 keeps; 1 < 1.6 resamples
    assert AR.decide(torch.tensor([2.0, 2.0 - 1e-9], dtype=torch.float64), 0.5, 4).tolist() == [False, True]   # ESS = tau N keeps
    assert AR.decide(torch.tensor([float("nan")]), 0.5, 4).tolist() == [True]          # a NaN ESS resamples
    shifted = AR.ess_of(lw + 123.0)
    assert torch.allclose(shifted, ess, rtol=1e-12)                                      # (scale-free)
    # decisions and indices are constants of the reverse pass: the mixed objective is differentiable
    FLAGS, model, obs, noise = _ends_case("AESMC")
    _, log = AR.run_oracle(model, FLAGS, "AESMC", obs, noise)
    assert 0 < int(log["rs_f"].sum()) < log["rs_f"].numel()
    z, P = AR.oracle_grads(model, FLAGS, "AESMC", obs, noise, {"idx_f": log["idx_f"], "rs_f": log["rs_f"].long()})
    assert torch.isfinite(z) and float(P["q1"]["layers"][0][0].grad.abs().max()) > 0


def test_the_gpu_cases_meet_their_conditions():
    """the cases of tests/test_gpu_adaptive.py on the fp64 reference alone: the resampling rate of each lies in [0.1, 0.9], and the
    fp32 reference's ESS (same draws and decisions) stays within ESS_GAP32 of N -- the figure the GPU tolerance is 4 x of"""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    worst = 0.0
    for case in AR.CASES:
        FLAGS, model, smc, obs, noise = AR.setup(case)
        assert smc.resample_ess == AR.TAU
        N = case[3]
        _, ref = AR.run_oracle(model, FLAGS, case[0], obs, noise)
        rate = float(ref["rs_f"].double().mean())
        teacher = {"idx_f": ref["idx_f"], "rs_f": ref["rs_f"].long()}
        _, r32 = AR.run_oracle(model, FLAGS, case[0], obs, noise, teacher=teacher, dtype=torch.float32)
        gap = float((r32["ess"].double() - ref["ess"]).abs().max()) / N
        print("%s: rate %.3f, ESS / N in [%.3f, %.3f], |ESS32 - ESS64| / N %.3e"
              % (AR.case_id(case), rate, float(ref["ess"].min()) / N, float(ref["ess"].max()) / N, gap))
        assert 0.1 <= rate <= 0.9, (AR.case_id(case), rate)
        assert torch.equal(AR.decide(ref["ess"], AR.TAU, N), ref["rs_f"])
        worst = max(worst, gap)
    # the recorded figure is this measurement, rounded up (slack for another host's fp32 summation order: the fp32 matrix products
    # of the MLPs are not summed in one order everywhere; the GPU tolerance is 4 x the RECORDED figure whatever is measured here)
    assert 0.25 * AR.ESS_GAP32 <= worst <= 1.5 * AR.ESS_GAP32, worst
