"""Adaptive resampling on the wide-observation kernels (FLAGS.resample_ess with FLAGS.resample_ess_wide_obs;
psvo_filter_forward_wobs_adaptive / psvo_filter_backward_wobs_adaptive) on the GPU against the fp64 reference of
tests/adaptive_reference.py (count cases: with tests/count_reference.py's emission).

Cases (wobs_adaptive_reference.CASES) are the smallest shapes that reach each form of the kernels: one wave at the smallest Dy,
the Lorenz and vind widths, an odd Dy over three waves without q2, Dx = 4 over five waves, the unit-normal Poisson emission,
every limit at once (N = 512, Dy = 32, Dx = 4) and the count instantiation under AESMC and SVO.  Tolerances are
tests/test_gpu_adaptive.py's -- the ELBO 1e-4 relative, X / Xanc / Xs 2e-4, logW / lse 5e-4, gradients 2e-3 of a tensor's largest
entry + 1e-6 -- and, for the effective sample size, MARGIN = 4 x ESS_GAP32_WIDE of N, where ESS_GAP32_WIDE is the largest
|ESS_fp32 - ESS_fp64| / N the fp32 CPU reference shows over these cases (tests/test_wobs_adaptive_host.py measures it and holds
it to this figure; profiles/wobs_adaptive.md records it) and 4 allows for the kernel's v_exp_f32 against libm."""
import functools
import glob
import os
import pickle

import numpy as np
import pytest
import torch

from tests import adaptive_reference as AR
from tests import ffbs_reference as FR
from tests import ffbsi_reference as FIR
from tests import helpers as Hh
from tests import wobs_adaptive_reference as WR
from tests.test_gpu_parity import _pairs

pytestmark = pytest.mark.gpu

MARGIN = 4 * WR.ESS_GAP32_WIDE
CASES = list(range(len(WR.CASES)))
_id = lambda i: WR.case_id(WR.CASES[i])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATIC_WORDS = ("filter_fwd_wobs_kernel", "filter_bwd_wobs_kernel", "filter_fwd_kernel", "filter_fwd_lpp_kernel",
                "filter_bwd_kernel", "filter_bwd_lpp_kernel", "filter_fwd_ad_kernel", "filter_fwd_lpp_ad_kernel",
                "filter_bwd_ad_kernel", "filter_bwd_lpp_ad_kernel", "fbs_")


def _hip(noise, teacher=None):
    """the reference's noise (+ teacher-forced idx_f / rs_f in its layouts) in the kernels' layout"""
    nz = Hh.noise_to_hip({**noise, **{k: v for k, v in (teacher or {}).items() if k == "idx_f"}}, "cuda")
    if "idx_f" in nz:
        nz.pop("u_f", None)
    if teacher and teacher.get("rs_f") is not None:
        nz["rs_f"] = teacher["rs_f"].to(torch.int32).contiguous().cuda()
    return nz


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _run(model, smc, obs, nz):
    model.zero_grad(set_to_none=True)
    z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    z.backward()
    torch.cuda.synchronize()
    return z.detach().clone(), log


@functools.lru_cache(maxsize=None)
def _free_run(i):
    """case i on the GPU, free running at its threshold, forward and reverse once: everything the value, decision and gradient
    tests share (computed once, never modified)"""
    case = WR.CASES[i]
    FLAGS, model, smc, obs, noise = WR.setup(case, "cuda")
    assert smc.wide_obs and smc.resample_ess == case[11]
    z, log = _run(model, smc, obs, _hip(noise))
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    z_ref, ref = WR.replay_with_hip(model, FLAGS, case, obs, noise, log)
    return dict(FLAGS=FLAGS, model=model, smc=smc, obs=obs, noise=noise, z=z, log=log, grads=grads, z_ref=z_ref, ref=ref)


def _check_grads_against(model, grads, P, label):
    by_param = {id(p): n for n, p in model.named_parameters()}
    rows = []
    for name, p, ref in _pairs(model, P):
        g = grads[by_param[id(p)]]
        g = torch.zeros_like(ref) if g is None else g.double().cpu()
        want = torch.zeros_like(ref) if ref.grad is None else ref.grad
        rows.append((name, float((g - want).abs().max()), max(float(want.abs().max()), 1e-6)))
    names = {n for n, _, _ in rows}
    assert len(rows) > 8 and any(s > 1e-3 for _, _, s in rows) and {"g.W0", "g.Wmu", "g.bmu"} <= names
    worst = max(rows, key=lambda v: v[1] / v[2])
    print("%s: worst gradient error / largest entry: %s %.3e" % (label, worst[0], worst[1] / worst[2]))
    bad = [v for v in rows if v[1] > 2e-3 * v[2] + 1e-6]
    assert not bad, "gradient mismatch (name, max abs err, largest entry): %s" % bad
    return rows


# ---- 1. the two ends -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", CASES, ids=_id)
@pytest.mark.parametrize("end", ["always", "never"])
def test_ends_bit_for_bit(built_lib, i, end):
    """ess_frac = 2 (always) against psvo_filter_forward_wobs with resample = 1: X, Fm, logW, lse, idx, Xanc and the ELBO bit for
    bit; ess_frac = 1e-9 (never) against resample = 0: X, Fm, logW, lse and the ELBO bit for bit.  Gradients against the static
    wide reverse pass within the suite's gradient tolerance."""
    case = WR.CASES[i]
    N = case[3]
    _, model_s, smc_s, obs, noise = WR.setup(case, "cuda", resample_ess=0.0)
    assert smc_s.resample_ess == 0.0 and smc_s.wide_obs
    smc_s.resample_particles = end == "always"
    _, model_a, smc_a, _, _ = WR.setup(case, "cuda")
    smc_a.resample_ess = 2.0 if end == "always" else 1e-9          # (outside the flag's range on purpose: the kernel's ends)
    nz = _hip(noise)
    z_s, log_s = _run(model_s, smc_s, obs, nz)
    g_s = _grads(model_s)
    z_a, log_a = _run(model_a, smc_a, obs, nz)
    g_a = _grads(model_a)
    f_s, f_a = log_s["filter"], log_a["filter"]
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
    """free running at the case's threshold; the fp64 reference replayed with the HIP indices and decisions"""
    r = _free_run(i)
    case, log, ref = WR.CASES[i], r["log"], r["ref"]
    T, B, N, tau = case[2], case[1], case[3], case[11]
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
    rule = AR.decide(ess_ref, tau, N)
    differ = rule != rs_hip
    excusable = (ess_ref / N - tau).abs() <= MARGIN
    assert not bool((differ & ~excusable).any()), "decisions off the rule: %s" % (differ & ~excusable).nonzero().tolist()
    assert int((differ & excusable).sum()) <= 0.05 * T * B
    assert 0 < int(rs_hip.sum()) < T * B          # some steps resample and some keep


# ---- 3. kernel forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,count", [(WR.ONE_WAVE, "false"), (WR.DX4, "false"), (WR.COUNT, "true")],
                         ids=["one-wave", "Dx4-five-waves", "count"])
def test_kernel_forms(built_lib, i, count):
    """the cases launch the adaptive wide kernels (the count case their count instantiation); no static wide filter kernel, no
    plain filter kernel and no affine-scan kernel runs"""
    case = WR.CASES[i]
    FLAGS, model, smc, obs, noise = WR.setup(case, "cuda")
    nz = _hip(noise)

    def run():
        z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        z.backward()
    _, names = Hh.kernel_names(run)
    # template arguments: <Dx, H, CNT> forward, <Dx, H, EXT = false, CNT> reverse
    for w, targs in (("filter_fwd_wobs_ad_kernel", "<%d, %s, %s>" % (case[4], case[6], count)),
                     ("filter_bwd_wobs_ad_kernel", "<%d, %s, false, %s>" % (case[4], case[6], count))):
        hit = [n for n in names if w in n]
        assert hit, (w, sorted(names))
        assert all(targs in n for n in hit), (targs, hit)
    assert any("mlp_wgrad_wobs_kernel" in n for n in names), sorted(names)
    assert not any(w in n for n in names for w in STATIC_WORDS), sorted(names)


# ---- 4. gradients -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", CASES, ids=_id)
def test_every_gradient(built_lib, i):
    """d log_ZSMC / d(every parameter) -- MLP_g's wide output layer and the encoder behind SVO included -- against fp64 autograd
    of the reference with the HIP forward's indices and decisions"""
    r = _free_run(i)
    case, model = WR.CASES[i], r["model"]
    z_ref, P = WR.oracle_grads(model, r["FLAGS"], case, r["obs"], r["noise"], WR.hip_teacher(r["log"]))
    assert abs(float(r["z"]) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    rows = _check_grads_against(model, r["grads"], P, _id(i))
    if case[0] == "SVO":
        assert any(n.startswith("y_smoother") and s > 1e-6 for n, _, s in rows)


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [WR.LORENZ, WR.LIMITS, WR.COUNT], ids=_id)
@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
def test_two_passes_are_bit_identical(built_lib, i, det):
    """forward + reverse twice, PSVO_TUNE_DETERMINISTIC off and on: the ELBO, the decisions and every .grad bit for bit"""
    from psvo_amd import _lib
    case = WR.CASES[i]
    FLAGS, model, smc, obs, noise = WR.setup(case, "cuda")
    nz = _hip(noise)
    res = []
    with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, det):
        for _ in range(2):
            z, log = _run(model, smc, obs, nz)
            res.append((z, log["filter"]["rs"].clone(), log["filter"]["ess"].clone(), _grads(model)))
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
    FLAGS, model, smc, obs, noise = WR.setup(WR.CASES[WR.LORENZ], "cuda")
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


# ---- 6. forced decisions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [WR.ONE_WAVE, WR.DX4, WR.COUNT], ids=_id)
def test_forced_decisions_are_honoured(built_lib, i):
    """noise["rs_f"], a fixed mixed pattern: rs_out == rs_in exactly, whatever the effective sample size says; values and every
    gradient match the reference under the same pattern"""
    case = WR.CASES[i]
    T, B, N = case[2], case[1], case[3]
    FLAGS, model, smc, obs, noise = WR.setup(case, "cuda")
    g = torch.Generator().manual_seed(11)
    forced = (torch.rand(T, B, generator=g) < 0.5).to(torch.int32)
    forced[0, 0], forced[1, 0] = 1, 0
    free = _free_run(i)["log"]["filter"]
    assert not torch.equal(free["rs"].cpu(), forced)
    z, log = _run(model, smc, obs, _hip(noise, {"rs_f": forced}))
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    filt = log["filter"]
    assert torch.equal(filt["rs"].cpu(), forced)
    assert torch.equal(filt["ess"][0], free["ess"][0])          # (step 0 is the same in both runs)
    teacher = {"idx_f": filt["idx"].permute(0, 2, 1).cpu().long(), "rs_f": forced.long()}
    z_ref, ref = WR.run_oracle(model, FLAGS, case, obs, noise, teacher=teacher)
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    assert torch.allclose(Hh.part_to_ref(filt["X"]), ref["X_prevs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert float(((filt["ess"].double().cpu() - ref["ess"]).abs() / N).max()) <= MARGIN
    _, P = WR.oracle_grads(model, FLAGS, case, obs, noise, teacher)
    _check_grads_against(model, grads, P, _id(i) + " forced")


# ---- 7. downstream -----------------------------------------------------------------------------------------------------------
def test_smoother_and_sampler_behind_the_wide_adaptive_filter(built_lib):
    """--FFBS and --FFBSi read X, Fm, logW of whatever filter ran: behind the wide adaptive filter they agree with their
    references fed that filter's outputs, at the tolerances of tests/test_gpu_ffbs.py / tests/test_gpu_ffbsi.py"""
    from tests.test_gpu_ffbs import EDGE_TOL, _check_draws, _yardstick
    from tests.test_gpu_ffbsi import K as K_PATH, ULP
    i = WR.LORENZ
    case = WR.CASES[i]
    T, B, N, Dx = case[2], case[1], case[3], case[4]
    FLAGS, model, smc, obs, noise = WR.setup(case, "cuda", FFBS=True, FFBSi=True)
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
    S = FR.scales(model.f_dist.get_sigma().detach().float().cpu(), T, B, Dx, N, dtype=torch.float32)
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


# ---- 8. the runner -----------------------------------------------------------------------------------------------------------
def _check_adaptive_run(hist, work, n_particles):
    elbo = np.asarray(hist["log_ZSMC_trains"], dtype=np.float64)
    assert len(elbo) >= 2 and np.isfinite(elbo).all()
    keys = ["adaptive_%s_%s" % (s, split) for s in ("rate", "ess_mean", "ess_min") for split in ("train", "test")]
    metrics = glob.glob(str(work / "rslts" / "**" / "metric_*.p"), recursive=True)
    assert metrics
    rates = []
    for path in metrics:
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        assert set(keys) <= set(m), sorted(m)
        for split in ("train", "test"):
            assert 0.0 <= m["adaptive_rate_" + split] <= 1.0, (path, m["adaptive_rate_" + split])
            assert 1.0 / n_particles - 1e-6 <= m["adaptive_ess_min_" + split] <= m["adaptive_ess_mean_" + split] <= 1.0 + 1e-5
            rates.append(m["adaptive_rate_" + split])
    # the resampled share of the run: some steps resampled and some kept
    assert 0.0 < float(np.mean(rates)) < 1.0, rates
    print("wide adaptive run: train ELBO %s" % np.array2string(elbo, precision=3))
    assert elbo[-1] > elbo[0], elbo


def test_runner_on_the_lorenz_slice(built_lib, tmp_path, monkeypatch):
    """--noPSVO --AESMC --Dy=10 --Dx=3 --resample_ess=0.5 --resample_ess_wide_obs on tests/golden/lorenz_slice.npz"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    d = np.load(os.path.join(GOLDEN, "lorenz_slice.npz"))
    work = tmp_path / "lorenz"
    work.mkdir()
    with open(work / "datadict", "wb") as f:          # the loader's format, as tests/test_gpu_wobs.py feeds it
        pickle.dump({k: d[k].astype(np.float64) for k in ("Ytrain", "Yvalid")}, f)
    monkeypatch.chdir(work)
    FLAGS = parse_flags(["--noPSVO", "--AESMC", "--Dy=10", "--Dx=3", "--resample_ess=0.5", "--resample_ess_wide_obs",
                         "--datadir=%s/" % work, "--datadict=datadict", "--epoch=4", "--print_freq=1", "--MSE_steps=5",
                         "--saving_num=4", "--n_particles=32", "--batch_size=4", "--lr=0.01", "--seed=1"])
    hist = runner.main(FLAGS)
    torch.cuda.synchronize()
    assert (FLAGS.n_train, FLAGS.n_test, FLAGS.time) == (8, 4, 100)
    _check_adaptive_run(hist, work, 32)


def test_runner_on_generated_counts(built_lib, tmp_path, monkeypatch):
    """--noPSVO --AESMC --generateTrainingData --count_emission --Dy=5 --resample_ess=0.5 --resample_ess_wide_obs"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    work = tmp_path / "counts"
    work.mkdir()
    monkeypatch.chdir(work)
    hist = runner.main(parse_flags(["--noPSVO", "--AESMC", "--generateTrainingData", "--count_emission", "--Dy=5",
                                    "--resample_ess=0.5", "--resample_ess_wide_obs", "--time=25", "--n_train=8", "--n_test=4",
                                    "--batch_size=4", "--n_particles=32", "--epoch=4", "--lr=0.01", "--seed=1"]))
    torch.cuda.synchronize()
    _check_adaptive_run(hist, work, 32)
