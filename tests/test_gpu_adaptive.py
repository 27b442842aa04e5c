"""Adaptive resampling (FLAGS.resample_ess; psvo_filter_forward_adaptive / psvo_filter_backward_adaptive) on the GPU against the
fp64 reference of tests/adaptive_reference.py.

Cases (adaptive_reference.CASES) are the smallest shapes that reach each kernel form: four lanes per particle in the four
wirings, one lane per particle at <= 256 threads with padded lanes (also under --poisson_emission), the 512-thread kernels, two
hidden layers in both forms, and SVO's encoder once.  Tolerances are the suite's own -- values as
tests/test_gpu_parity.py::test_teacher_forced_parity, the ELBO 1e-4 relative, gradients 2e-3 of a tensor's largest entry + 1e-6
 -- and, for the effective sample size, MARGIN = 4 x ESS_GAP32 of N, where ESS_GAP32 is the largest
|ESS_fp32 - ESS_fp64| / N the fp32 CPU reference shows over these cases (tests/test_adaptive_host.py measures it and holds it to
this figure; profiles/adaptive_resampling.md records it) and 4 allows for the kernel's v_exp_f32 against libm."""
import functools
import glob
import pickle

import numpy as np
import pytest
import torch

from tests import adaptive_reference as AR
from tests import ffbs_reference as FR
from tests import ffbsi_reference as FIR
from tests import helpers as Hh
from tests.test_gpu_parity import _pairs

pytestmark = pytest.mark.gpu

ESS_GAP32 = AR.ESS_GAP32
MARGIN = 4 * ESS_GAP32
CASES = list(range(len(AR.CASES)))
_id = lambda i: AR.case_id(AR.CASES[i])
LPP, WIDE, BIG, L2_LPP, L2_WIDE = 0, 4, 6, 7, 8          # one case per kernel form


def _hip(noise, teacher=None):
    """the reference's noise (+ teacher-forced idx_f / rs_f in its layouts) in the kernels' layout"""
    nz = Hh.noise_to_hip({**noise, **{k: v for k, v in (teacher or {}).items() if k == "idx_f"}}, "cuda")
    if "idx_f" in nz:
        nz.pop("u_f", None)
    if teacher and teacher.get("rs_f") is not None:
        nz["rs_f"] = teacher["rs_f"].to(torch.int32).contiguous().cuda()
    return nz


@functools.lru_cache(maxsize=None)
def _free_run(i):
    """case i on the GPU, free running at TAU, forward and reverse once: everything the value, decision and gradient tests share
    (computed once, never modified)"""
    case = AR.CASES[i]
    FLAGS, model, smc, obs, noise = AR.setup(case, "cuda")
    model.zero_grad(set_to_none=True)
    z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise))
    z.backward()
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    z_ref, ref = AR.replay_with_hip(model, FLAGS, case[0], obs, noise, log)
    return dict(FLAGS=FLAGS, model=model, smc=smc, obs=obs, noise=noise, z=z.detach(), log=log, grads=grads, z_ref=z_ref, ref=ref)


def _static(case, resample, seed=None):
    """the same model under the static filter: resampling at every step, or never (the IWAE path of psvo_filter_forward)"""
    FLAGS, model, smc, obs, noise = AR.setup(case, "cuda", seed=seed, resample_ess=0.0)
    assert smc.resample_ess == 0.0
    smc.resample_particles = bool(resample)
    return FLAGS, model, smc, obs, noise


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


# ---- 1. the two ends -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", CASES, ids=_id)
@pytest.mark.parametrize("end", ["always", "never"])
def test_ends_bit_for_bit(built_lib, i, end):
    """ess_frac = 2 (always) against psvo_filter_forward with resample = 1: X, Fm, logW, lse, idx, Xanc bit for bit; ess_frac =
    1e-9 (never) against resample = 0: X, Fm, logW, lse bit for bit.  Gradients against the existing persistent reverse pass
    (PSVO_TUNE_FILTER_BWD = 0) within the suite's gradient tolerance."""
    from psvo_amd import _lib
    case = AR.CASES[i]
    N = case[3]
    _, model_s, smc_s, obs, noise = _static(case, end == "always")
    _, model_a, smc_a, _, _ = AR.setup(case, "cuda")
    smc_a.resample_ess = 2.0 if end == "always" else 1e-9          # (outside the flag's range on purpose: the kernel's ends)
    nz = _hip(noise)
    res = []
    with Hh.tuning(_lib.PSVO_TUNE_FILTER_BWD, 0):
        for model, smc in ((model_s, smc_s), (model_a, smc_a)):
            model.zero_grad(set_to_none=True)
            z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
            z.backward()
            torch.cuda.synchronize()
            res.append((z.detach(), log["filter"], _grads(model)))
    (z_s, f_s, g_s), (z_a, f_a, g_a) = res
    rs, ess = f_a["rs"], f_a["ess"]
    assert rs.shape == ess.shape == (case[2], case[1]) and rs.dtype == torch.int32
    assert bool((rs == (1 if end == "always" else 0)).all())
    assert torch.isfinite(ess).all() and float(ess.min()) >= 1.0 - 1e-3 and float(ess.max()) <= N * (1 + 1e-5)
    for k in ("X", "Fm", "logW", "lse") + (("idx", "Xanc") if end == "always" else ()):
        assert torch.equal(f_a[k], f_s[k]), k
    assert torch.equal(z_a, z_s)
    assert g_a.keys() == g_s.keys() and len(g_a) > 4
    worst = ("", 0.0)
    for n in g_s:
        scale = max(float(g_s[n].abs().max()), 1e-6)
        err = float((g_a[n] - g_s[n]).abs().max())
        worst = max(worst, (n, err / scale), key=lambda v: v[1])
        assert err <= 2e-3 * scale + 1e-6, (n, err, scale)
    print("%s %s: worst gradient difference / largest entry: %s %.3e" % (_id(i), end, worst[0], worst[1]))


# ---- 2. values and decisions, free running ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", CASES, ids=_id)
def test_values_and_decisions(built_lib, i):
    """free running at TAU; the fp64 reference replayed with the HIP indices and decisions"""
    r = _free_run(i)
    case, log, ref = AR.CASES[i], r["log"], r["ref"]
    T, B, N = case[2], case[1], case[3]
    filt = log["filter"]
    err = lambda a, b: float((a - b).abs().max())
    lse_ref = torch.logsumexp(ref["log_Ws"], 1)
    ess_hip, ess_ref = filt["ess"].double().cpu(), ref["ess"]
    rs_hip = filt["rs"].cpu() != 0
    gap = (ess_hip - ess_ref).abs() / N
    print("%s: max abs err X %.3e logW %.3e lse %.3e; ELBO rel %.3e; |ESS - ESS_ref| / N max %.3e (margin %.3e); resampled %d of %d"
          % (_id(i), err(Hh.part_to_ref(filt["X"]), ref["X_prevs"]), err(Hh.w_to_ref(filt["logW"]), ref["log_Ws"]),
             err(filt["lse"].double().cpu(), lse_ref), abs(float(r["z"]) - float(r["z_ref"])) / abs(float(r["z_ref"])),
             float(gap.max()), MARGIN, int(rs_hip.sum()), T * B))
    assert abs(float(r["z"]) - float(r["z_ref"])) <= 1e-4 * abs(float(r["z_ref"]))
    assert torch.allclose(Hh.part_to_ref(filt["X"]), ref["X_prevs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.part_to_ref(filt["Xanc"]), ref["X_ancestors"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(filt["lse"].double().cpu(), lse_ref, atol=5e-4, rtol=1e-5)
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)
    # log["ess"] / log["resampled"] are the kernel's outputs in (B, T)
    assert torch.equal(log["ess"], filt["ess"].t()) and torch.equal(log["resampled"], (filt["rs"] != 0).t())
    assert bool(((filt["rs"] == 0) | (filt["rs"] == 1)).all())
    # the effective sample size against fp64
    assert float(gap.max()) <= MARGIN, "ESS off by %.3e N (margin %.3e N)" % (float(gap.max()), MARGIN)
    # every decision is the rule's on the replayed weights, unless ESS_ref / N is within the margin of the threshold
    rule = AR.decide(ess_ref, AR.TAU, N)
    differ = rule != rs_hip
    excusable = (ess_ref / N - AR.TAU).abs() <= MARGIN
    assert not bool((differ & ~excusable).any()), "decisions off the rule: %s" % (differ & ~excusable).nonzero().tolist()
    assert int((differ & excusable).sum()) <= 0.05 * T * B
    # the reference on its own (free running) resamples at some steps and keeps at others
    _, own = AR.run_oracle(r["model"], r["FLAGS"], case[0], r["obs"], r["noise"])
    rate = float(own["rs_f"].double().mean())
    assert 0.1 <= rate <= 0.9, rate
    assert 0 < int(rs_hip.sum()) < T * B


@pytest.mark.parametrize("i,words", [(LPP, ("filter_fwd_lpp_ad_kernel", "filter_bwd_lpp_ad_kernel")),
                                     (WIDE, ("filter_fwd_ad_kernel", "filter_bwd_ad_kernel", "256")),
                                     (BIG, ("filter_fwd_ad_kernel", "filter_bwd_ad_kernel", "512")),
                                     (L2_LPP, ("l2::filter_fwd_lpp_ad_kernel", "l2::filter_bwd_lpp_ad_kernel")),
                                     (L2_WIDE, ("l2::filter_fwd_ad_kernel", "l2::filter_bwd_ad_kernel"))],
                         ids=["lpp", "256-threads", "512-threads", "two-layers-lpp", "two-layers-256-threads"])
def test_kernel_forms(built_lib, i, words):
    """each case reaches the kernels it is there for, and no static filter kernel or affine-scan kernel runs"""
    case = AR.CASES[i]
    FLAGS, model, smc, obs, noise = AR.setup(case, "cuda")
    nz = _hip(noise)

    def run():
        z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        z.backward()
    _, names = Hh.kernel_names(run)
    for w in words[:2]:
        hit = [n for n in names if w in n]
        assert hit, (w, sorted(names))
        assert len(words) < 3 or all(", %s" % words[2] in n for n in hit), hit
    assert not any(("filter_fwd_kernel" in n or "filter_fwd_lpp_kernel" in n or "filter_bwd_kernel" in n
                    or "filter_bwd_lpp_kernel" in n or "fbs_" in n) for n in names), sorted(names)


# ---- 3. gradients -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", CASES, ids=_id)
def test_every_gradient(built_lib, i):
    """d log_ZSMC / d(every parameter) against fp64 autograd of the reference with the HIP forward's indices and decisions"""
    r = _free_run(i)
    case, model = AR.CASES[i], r["model"]
    z_ref, P = AR.oracle_grads(model, r["FLAGS"], case[0], r["obs"], r["noise"], AR.hip_teacher(r["log"]))
    assert abs(float(r["z"]) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    by_param = {id(p): n for n, p in model.named_parameters()}
    rows = []
    for name, p, ref in _pairs(model, P):
        g = r["grads"][by_param[id(p)]]
        g = torch.zeros_like(ref) if g is None else g.double().cpu()
        want = torch.zeros_like(ref) if ref.grad is None else ref.grad
        rows.append((name, float((g - want).abs().max()), max(float(want.abs().max()), 1e-6)))
    assert len(rows) > 8 and any(s > 1e-3 for _, _, s in rows)
    worst = max(rows, key=lambda v: v[1] / v[2])
    print("%s: worst gradient error / largest entry: %s %.3e" % (_id(i), worst[0], worst[1] / worst[2]))
    bad = [v for v in rows if v[1] > 2e-3 * v[2] + 1e-6]
    assert not bad, "gradient mismatch (name, max abs err, largest entry): %s" % bad


# ---- 4. reproducibility ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [LPP, WIDE, BIG, L2_WIDE], ids=_id)
def test_deterministic_mode_is_bit_identical(built_lib, i):
    """PSVO_TUNE_DETERMINISTIC = 1: forward + reverse twice, the ELBO, the decisions and every .grad bit for bit (the 512-thread
    case takes filter_bwd_ad_kernel<.., true>)"""
    from psvo_amd import _lib
    case = AR.CASES[i]
    FLAGS, model, smc, obs, noise = AR.setup(case, "cuda")
    nz = _hip(noise)
    res = []
    with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, 1):
        def run():
            model.zero_grad(set_to_none=True)
            z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
            z.backward()
            torch.cuda.synchronize()
            res.append((z.detach().clone(), log["filter"]["rs"].clone(), log["filter"]["ess"].clone(), _grads(model)))
        if i == BIG:
            _, names = Hh.kernel_names(run)
            det = [n for n in names if "filter_bwd_ad_kernel" in n]
            assert det and all("true" in n for n in det), sorted(names)
        else:
            run()
        run()
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[3].keys() == b[3].keys() and len(a[3]) > 4
    for n, g in a[3].items():
        assert torch.isfinite(g).all() and torch.equal(g, b[3][n]), n


def test_step_replays_from_hipgraph(built_lib):
    """one local training step, eager and captured into a GraphedStep: the decision is made on the device, so the capture holds
    the whole step and a replay equals the eager step bit for bit"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    FLAGS, model, smc, obs, noise = AR.setup(AR.CASES[WIDE], "cuda")
    nz = _hip(noise)
    flat = FlatParams(model)
    obs_c = obs.float().cuda()
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


@pytest.mark.parametrize("i", [LPP, BIG, L2_WIDE], ids=_id)
def test_forced_decisions_are_honoured(built_lib, i):
    """noise["rs_f"]: rs_out == rs_in exactly, whatever the effective sample size says; ess_out is still the step's ESS; all
    ones reproduce the static filter bit for bit"""
    case = AR.CASES[i]
    T, B = case[2], case[1]
    FLAGS, model, smc, obs, noise = AR.setup(case, "cuda")
    g = torch.Generator().manual_seed(11)
    forced = (torch.rand(T, B, generator=g) < 0.5).to(torch.int32)
    forced[0, 0], forced[1, 0] = 1, 0
    with torch.no_grad():
        _, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise, {"rs_f": forced}))
        _, free = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise))
    torch.cuda.synchronize()
    assert torch.equal(log["filter"]["rs"].cpu(), forced)
    assert not torch.equal(free["filter"]["rs"].cpu(), forced)
    assert torch.equal(log["filter"]["ess"][0], free["filter"]["ess"][0])          # (step 0 is the same in both runs)
    _, ref = AR.run_oracle(model, FLAGS, case[0], obs, noise,
                           teacher={"idx_f": log["filter"]["idx"].permute(0, 2, 1).cpu().long(), "rs_f": forced.long()})
    assert torch.allclose(Hh.w_to_ref(log["filter"]["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert float(((log["filter"]["ess"].double().cpu() - ref["ess"]).abs() / case[3]).max()) <= MARGIN
    _, _, smc_s, _, _ = _static(case, True)
    with torch.no_grad():
        _, ones = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise, {"rs_f": torch.ones(T, B, dtype=torch.int32)}))
        _, stat = smc_s.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise))
    for k in ("X", "Xanc", "Fm", "logW", "lse", "idx"):
        assert torch.equal(ones["filter"][k], stat["filter"][k]), k


# ---- 5. downstream ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [LPP, WIDE], ids=_id)
def test_smoother_and_sampler_behind_an_adaptive_filter(built_lib, i):
    """--FFBS and --FFBSi read X, Fm, logW of whatever filter ran: behind an adaptive filter they agree with their references
    fed that filter's outputs, at the tolerances of tests/test_gpu_ffbs.py / tests/test_gpu_ffbsi.py"""
    from tests.test_gpu_ffbs import EDGE_TOL, _check_draws, _yardstick
    from tests.test_gpu_ffbsi import K as K_PATH, ULP
    case = AR.CASES[i]
    T, B, N, Dx = case[2], case[1], case[3], case[4]
    FLAGS, model, smc, obs, noise = AR.setup(case, "cuda", FFBS=True, FFBSi=True)
    nz = _hip(noise)
    g = torch.Generator().manual_seed(100)
    nz["u_s"], nz["u_p"] = torch.rand(T, B, N, generator=g).cuda(), torch.rand(T, B, N, generator=g).cuda()
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    torch.cuda.synchronize()
    filt = log["filter"]
    assert 0 < int(filt["rs"].sum()) < T * B          # a filter that kept its particles at some steps
    assert torch.equal(filt["logW"], _free_run(i)["log"]["filter"]["logW"])          # the filter itself is untouched
    X, Fm, logW = (filt[k].cpu() for k in ("X", "Fm", "logW"))
    S = FR.scales(model.q1_dist.get_sigma().detach().float().cpu(), T, B, Dx, N, dtype=torch.float32)
    # the marginal smoother
    q64 = FR.quantities(X.double(), Fm.double(), S.double(), logW.double())
    q32 = FR.quantities(X, Fm, S, logW)
    hip = {"p": log["logW_smooth"].double().cpu().exp(), "Xmean": log["X_smooth_mean"].transpose(0, 1).double().cpu(),
           "ess": log["ess_smooth"].transpose(0, 1).double().cpu()}
    _yardstick(_id(i) + "+adaptive", hip, q64, q32)
    sm = log["smoother"]
    _check_draws(log["logW_smooth"], nz["u_s"], sm["idx"], filt["X"], sm["Xs"])
    assert torch.equal(log["Xs_marginal"], sm["Xs"].permute(1, 0, 3, 2))
    # the backward-sampled paths: the kernel's picks teacher-forced into the fp64 reference
    paths = log["paths"]
    assert torch.equal(log["Xs"], FIR.gather(filt["X"], paths["idx"]).permute(1, 0, 3, 2))
    assert torch.equal(paths["distinct"].cpu().long(), FIR.distinct(paths["idx"].cpu()))
    picks = paths["idx"].cpu()
    ref64 = FIR.sample(X.double(), Fm.double(), S.double(), logW.double(), idx_in=picks)["logq"]
    ref32 = FIR.sample(X, Fm, S, logW, idx_in=picks)["logq"]
    e_hip, biggest = FIR.forced_error(paths["logq"].cpu(), ref64)
    e_32, _ = FIR.forced_error(ref32, ref64)
    print("%s: path logq err_hip %.3e err_32 %.3e floor %.3e" % (_id(i), e_hip, e_32, 8 * ULP * biggest))
    assert e_hip <= K_PATH * e_32 + 8 * ULP * biggest
    d = FIR.draw_distances(X, Fm, S, logW, nz["u_p"].cpu(), picks.long())
    assert float(d.max()) <= EDGE_TOL and int((d > 0).sum()) <= max(3, int(20 * EDGE_TOL * d.numel()))


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """runner.main with --AESMC --resample_ess=0.5: the ELBO improves, the adaptive_* keys are in every metric_*.p and make
    sense; the same run without the flag has no such keys"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    argv = ["--noPSVO", "--AESMC", "--generateTrainingData", "--time=25", "--n_train=8", "--n_test=4", "--batch_size=4",
            "--n_particles=32", "--epoch=4", "--lr=0.01", "--seed=1"]
    keys = ["adaptive_%s_%s" % (s, split) for s in ("rate", "ess_mean", "ess_min") for split in ("train", "test")]
    for on in (True, False):
        work = tmp_path / ("on" if on else "off")
        work.mkdir()
        monkeypatch.chdir(work)
        hist = runner.main(parse_flags(argv + (["--resample_ess=0.5"] if on else [])))
        torch.cuda.synchronize()
        elbo = np.asarray(hist["log_ZSMC_trains"], dtype=np.float64)
        assert len(elbo) >= 2 and np.isfinite(elbo).all()
        metrics = glob.glob(str(work / "rslts" / "epoch_data" / "**" / "metric_*.p"), recursive=True)
        assert metrics
        for path in metrics:
            with open(path, "rb") as fh:
                m = pickle.load(fh)
            if on:
                assert set(keys) <= set(m), sorted(m)
                for split in ("train", "test"):
                    assert 0.0 <= m["adaptive_rate_" + split] <= 1.0
                    assert 1.0 / 32 - 1e-6 <= m["adaptive_ess_min_" + split] <= m["adaptive_ess_mean_" + split] <= 1.0 + 1e-5
            else:
                assert not any(k.startswith("adaptive") for k in m), sorted(m)
        if on:
            print("adaptive run: train ELBO %s" % np.array2string(elbo, precision=3))
            assert elbo[-1] > elbo[0], elbo
