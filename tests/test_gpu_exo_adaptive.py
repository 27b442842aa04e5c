"""Adaptive resampling under exogenous inputs (FLAGS.Di with FLAGS.resample_ess and FLAGS.resample_ess_inputs;
psvo_filter_forward_wobs_input_adaptive / psvo_filter_backward_wobs_input_adaptive, the sixth compilation of
psvo_amd/csrc/filter_wobs_impl.h) on the GPU.

Cases: those of tests/exo_reference.py that resample at all (XA.RUNS) -- the smallest shape, ONE wave staging 2 H = 128 bias words,
a partly filled wave with a separate f, eight waves at every limit, T = 60.  Three bit identities tie the pair to the kernels it
is the intersection of: a zero input share gives the adaptive missing-observation pair (forward outputs and reverse rows), a
threshold above 1 the input pair resampling at every step, a threshold no ESS falls below the input pair that never resamples.
Mixed decisions are forced through noise["rs_f"] with non-zero inputs and compared -- values, the ELBO and every gradient, the
input rows W1[Dx:] on their own -- against fp64 autograd of tests/exo_adaptive_reference.py at the tolerances of
tests/test_gpu_exo.py, taken as they are: values allclose with atol 2e-4 (X) / 5e-4 (logW, lse) and rtol 1e-5, the ELBO 1e-4
relative, gradients 2e-3 of a tensor's largest entry + 1e-6 with the fp32-reference clause (K32)."""
import glob
import pickle

import numpy as np
import pytest
import torch

from tests import exo_adaptive_reference as XA
from tests import exo_reference as ER
from tests import helpers as Hh
from tests.test_gpu_exo import exo_setup
from tests.test_gpu_instantiations import K32
from tests.test_gpu_parity import _pairs, _setup

pytestmark = pytest.mark.gpu

RUNS, _id = XA.RUNS, XA.run_id
FILTER_KEYS = ("X", "Xanc", "Fm", "logW", "lse", "idx")


def _adaptive(run, seed, **extra):
    FLAGS, model, smc, obs, v, noise = exo_setup(run, seed, resample_ess=XA.TAU, resample_ess_inputs=True, **extra)
    assert smc.resample_ess == XA.TAU and smc.Di == run[1]
    return FLAGS, model, smc, obs, v, noise


def _hip(noise, teacher=None):
    """the reference's noise (+ teacher-forced idx_f / rs_f in its layouts) in the kernels' layout"""
    nz = Hh.noise_to_hip({**noise, **{k: v for k, v in (teacher or {}).items() if k == "idx_f"}}, "cuda")
    if "idx_f" in nz:
        nz.pop("u_f", None)
    if teacher and teacher.get("rs_f") is not None:
        nz["rs_f"] = teacher["rs_f"].to(torch.int32).contiguous().cuda()
    return nz


def _step(smc, model, obs, v, nz):
    model.zero_grad(set_to_none=True)
    z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz, inputs=v.float().cuda())
    z.backward()
    torch.cuda.synchronize()
    return z.detach().clone(), log, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


class _Rows:
    """what the reverse wrappers handed back while this is active: the rows d P / d F / d G and the per-sequence gradients"""
    KEYS = ("dP", "dF", "dG", "dmu2", "dm0", "dfm0", "dsig_q1", "dsig_q2", "dsig_f", "dsig_g", "dsig0", "dfsig0")

    def __init__(self, monkeypatch, name):
        from psvo_amd import ops
        self.seen = []
        real = getattr(ops, name)

        def spy(*a, **k):
            r = real(*a, **k)
            self.seen.append({key: (None if r.get(key) is None else r[key].clone()) for key in self.KEYS})
            return r
        monkeypatch.setattr(ops, name, spy)


# ---- 1. the bit identities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_zero_input_share_is_the_adaptive_missing_pair(built_lib, run, monkeypatch):
    """W1[Dx:] = 0, i.e. hb = 0: forward outputs, decisions, ESS and the reverse rows of psvo_filter_*_wobs_missing_adaptive on the
    same weights, bit for bit -- free running, so that the decisions are the kernels' own, and again under the forced mixed
    pattern, so that both kinds of step are in it whatever the model decides"""
    case, Di, _ = run
    Dx = case[5]
    FLAGS, model, smc, obs, v, noise = _adaptive(run, 3, missing_obs=True, resample_ess_missing_obs=True)
    with torch.no_grad():
        for tr in {model.q1_tran, model.f_tran}:
            tr.kernels[0][Dx:].zero_()
    F0, model0, smc0, _, _ = _setup(*case, seed=3, missing_obs=True, resample_ess=XA.TAU, resample_ess_missing_obs=True)
    assert smc0.Di == 0 and smc0.missing_obs and smc0.resample_ess == XA.TAU
    src = dict(model.named_parameters())
    with torch.no_grad():
        for n, p in model0.named_parameters():
            p.copy_(src[n][:Dx] if src[n].shape != p.shape else src[n])
    a = _Rows(monkeypatch, "filter_backward_wobs_input_adaptive")
    b = _Rows(monkeypatch, "filter_backward_wobs_missing_adaptive")
    assert float(v.abs().max()) > 1
    forced = XA.forced(case[2], case[1])
    for i, nz in enumerate((Hh.noise_to_hip(noise, "cuda"), _hip(noise, {"rs_f": forced}))):
        z, log, _ = _step(smc, model, obs, v, nz)
        model0.zero_grad(set_to_none=True)
        z0, log0 = smc0.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        z0.backward()
        torch.cuda.synchronize()
        assert len(a.seen) == i + 1 and len(b.seen) == i + 1
        for key in FILTER_KEYS + ("rs", "ess"):
            assert torch.equal(log["filter"][key], log0["filter"][key]), key
        assert torch.equal(z, z0.detach()) and torch.isfinite(z)
        print("%s %s: resampled %d of %d" % (_id(run), "forced" if i else "free", int(log["filter"]["rs"].sum()), forced.numel()))
        for key in _Rows.KEYS:
            x, y = a.seen[i][key], b.seen[i][key]
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), key
    assert torch.equal(log["filter"]["rs"].cpu(), forced)


@pytest.mark.parametrize("run", RUNS, ids=_id)
@pytest.mark.parametrize("end", ["always", "never"])
def test_ends_are_the_input_pair(built_lib, run, end):
    """ess_frac = 2 (always) against psvo_filter_forward_wobs_input with resample = 1: every forward output, the ELBO and every
    gradient bit for bit; ess_frac = 1e-30 (never) against resample = 0: X, Fm, logW, lse and the ELBO bit for bit"""
    FLAGS, model, smc_s, obs, v, noise = exo_setup(run, 3)
    smc_s.resample_particles = end == "always"
    smc_a = type(smc_s)(model, ER.run_flags(run, resample_ess=XA.TAU, resample_ess_inputs=True))
    smc_a.resample_ess = 2.0 if end == "always" else 1e-30          # (outside the flag's range on purpose: the kernel's ends)
    nz = Hh.noise_to_hip(noise, "cuda")
    z_s, log_s, g_s = _step(smc_s, model, obs, v, nz)
    z_a, log_a, g_a = _step(smc_a, model, obs, v, nz)
    f_s, f_a = log_s["filter"], log_a["filter"]
    N = run[0][3]
    assert bool((f_a["rs"] == (1 if end == "always" else 0)).all())
    assert torch.isfinite(f_a["ess"]).all() and float(f_a["ess"].min()) >= 1.0 - 1e-3 and float(f_a["ess"].max()) <= N * (1 + 1e-5)
    for k in ("X", "Fm", "logW", "lse") + (("idx", "Xanc") if end == "always" else ()):
        assert torch.equal(f_a[k], f_s[k]), k
    assert torch.equal(z_a, z_s) and torch.isfinite(z_a)
    assert g_a.keys() == g_s.keys() and len(g_a) > 4
    if end == "always":
        for n in g_s:
            assert torch.equal(g_a[n], g_s[n]), n
    else:       # (the static reverse kernel takes `!resample` where the adaptive one takes `!rs[t]`: the same terms)
        for n in g_s:
            scale = max(float(g_s[n].abs().max()), 1e-6)
            assert float((g_a[n] - g_s[n]).abs().max()) <= 2e-3 * scale + 1e-6, n


# ---- 2. mixed decisions against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_forced_mixed_decisions(built_lib, run):
    """noise["rs_f"], the fixed mixed pattern, with non-zero inputs: rs_out == rs_in exactly; values, the ELBO and every
    gradient, d W1[Dx:] and d v included, against fp64 autograd of the reference under the same pattern and indices"""
    obj, B, T, N, Dx = run[0][0], run[0][1], run[0][2], run[0][3], run[0][5]
    FLAGS, model, smc, obs, v, noise = _adaptive(run, 5)
    forced = XA.forced(T, B)
    assert float(v.abs().max()) > 1
    # forward alone first: the indices it draws are what the reference is teacher-forced with
    with torch.no_grad():
        _, log0 = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise, {"rs_f": forced}), inputs=v.float().cuda())
    teacher = {"idx_f": log0["filter"]["idx"].permute(0, 2, 1).cpu().long(), "rs_f": forced.long()}
    model.zero_grad()
    v_c = v.float().cuda().requires_grad_(True)
    z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise, teacher), inputs=v_c)
    z.backward()
    torch.cuda.synchronize()
    filt = log["filter"]
    assert set(filt) == {"lse", "Fm", "logW", "X", "Xanc", "idx", "eps", "u", "rs", "ess"}
    assert torch.equal(filt["rs"].cpu(), forced) and torch.equal(filt["idx"], log0["filter"]["idx"])
    assert torch.equal(log["ess"], filt["ess"].t()) and torch.equal(log["resampled"], (filt["rs"] != 0).t())
    z_ref, ref = XA.run(model, FLAGS, obj, obs, v, noise, teacher=teacher)
    err = lambda a, b: float((a.detach() - b).abs().max())
    lse_ref = torch.logsumexp(ref["log_Ws"], 1)
    gap = float(((filt["ess"].double().cpu() - ref["ess"]).abs() / N).max())
    print("%s forced: max abs err X %.3e logW %.3e lse %.3e ELBO rel %.3e |ESS - ESS_ref| / N %.3e"
          % (_id(run), err(Hh.part_to_ref(filt["X"]), ref["X_prevs"]), err(Hh.w_to_ref(filt["logW"]), ref["log_Ws"]),
             err(filt["lse"].double().cpu(), lse_ref), abs(float(z) - float(z_ref)) / abs(float(z_ref)), gap))
    assert torch.allclose(Hh.part_to_ref(filt["X"]), ref["X_prevs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.part_to_ref(filt["Xanc"]), ref["X_ancestors"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(filt["lse"].double().cpu(), lse_ref, atol=5e-4, rtol=1e-5)
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)
    assert abs(float(z_ref)) >= 1.0 and abs(float(z.detach()) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    assert torch.isfinite(filt["ess"]).all() and float(filt["ess"].min()) >= 1.0 - 1e-3 and float(filt["ess"].max()) <= N * (1 + 1e-5)
    # gradients
    _, P, dv_ref = XA.grads(model, FLAGS, obj, obs, v, noise, teacher)
    rows = [("inputs", err(v_c.grad.double().cpu(), dv_ref), max(float(dv_ref.abs().max()), 1e-6))]
    assert float(dv_ref.abs().max()) > 0
    for name, p, r in _pairs(model, P):
        g = torch.zeros_like(r) if p.grad is None else p.grad.detach().double().cpu()
        want = torch.zeros_like(r) if r.grad is None else r.grad
        assert torch.isfinite(g).all(), name
        rows.append((name, err(g, want), max(float(want.abs().max()), 1e-6)))
        if name in ("q1.W0", "f.W0"):       # the input rows on their own: they must not hide behind a larger state block
            assert float(want[Dx:].abs().max()) > 0, name
            rows.append((name + "[Dx:]", err(g[Dx:], want[Dx:]), max(float(want[Dx:].abs().max()), 1e-6)))
    worst = max(rows, key=lambda r: r[1] / r[2])
    print("%s forced: worst gradient error / largest entry: %s %.3e" % (_id(run), worst[0], worst[1] / worst[2]))
    over = [r for r in rows if r[1] > 2e-3 * r[2] + 1e-6]
    if over:        # the second clause: the fp32 reference's own error on the same tensor (computed only when it is needed)
        _, P32, dv32 = XA.grads(model, FLAGS, obj, obs, v, noise, teacher, dtype=torch.float32)
        err32 = {"inputs": err(dv32.double(), dv_ref)}
        for (name, _, r), (_, _, r32) in zip(_pairs(model, P), _pairs(model, P32)):
            want = torch.zeros_like(r) if r.grad is None else r.grad
            w32 = torch.zeros_like(r) if r32.grad is None else r32.grad.double()
            err32[name] = err(w32, want)
            if name in ("q1.W0", "f.W0"):
                err32[name + "[Dx:]"] = err(w32[Dx:], want[Dx:])
        bad = [(n, e, s, err32[n]) for n, e, s in over if e > K32 * err32[n]]
        assert not bad, "gradient mismatch (name, max abs err, own scale, fp32 reference's own err): %s" % bad
    names = {r[0] for r in rows}
    assert {"q1.W0", "q1.W0[Dx:]", "q1.b0", "g.W0", "inputs"} <= names and ("f.W0[Dx:]" in names) == (not run[0][8])


# ---- 3. reproducibility, capture, the runner ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("run", [RUNS[1], RUNS[3]], ids=_id)
def test_two_passes_are_bit_identical(built_lib, run, det):
    from psvo_amd import _lib
    FLAGS, model, smc, obs, v, noise = _adaptive(run, 5)
    nz = Hh.noise_to_hip(noise, "cuda")
    res = []
    with Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, det):
        for _ in range(2):
            z, log, g = _step(smc, model, obs, v, nz)
            res.append((z, log["filter"]["rs"].clone(), log["filter"]["ess"].clone(), g))
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.isfinite(a[0])
    assert a[3].keys() == b[3].keys() and len(a[3]) > 8
    for n, g in a[3].items():
        assert torch.isfinite(g).all() and torch.equal(g, b[3][n]), n


def test_step_replays_from_hipgraph(built_lib):
    """one local training step of the T = 60 case, eager and captured into a GraphedStep: the decision is made on the device, so
    the capture holds the whole step and a replay equals the eager step bit for bit.  (Threshold 0.25: the fp64 reference alone
    resamples at 46 of this run's 60 steps there and at all 60 at 0.5, and a captured decision should be a mixed one.)"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    run = RUNS[4]
    FLAGS, model, smc, obs, v, noise = exo_setup(run, 3, resample_ess=0.25, resample_ess_inputs=True)
    assert smc.resample_ess == 0.25
    nz = Hh.noise_to_hip(noise, "cuda")
    flat = FlatParams(model)
    obs_c, v_c = obs.float().cuda(), v.float().cuda()
    seen = {}

    def local():
        flat.zero_grad()
        z, log = smc.get_log_ZSMC(obs_c, None, noise=nz, inputs=v_c)
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


def test_smoothers_run_behind_it(built_lib):
    """--FFBS / --FFBSi / --MAP_path read X, Fm, logW of whatever filter ran: behind the adaptive input filter they run unchanged
    and leave the filter's own outputs alone"""
    run = RUNS[2]
    FLAGS, model, smc, obs, v, noise = _adaptive(run, 3, FFBS=True, FFBSi=True, MAP_path=True)
    plain = type(smc)(model, ER.run_flags(run, resample_ess=XA.TAU, resample_ess_inputs=True))
    nz = Hh.noise_to_hip(noise, "cuda")
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz, inputs=v.float().cuda())
        z0, log0 = plain.get_log_ZSMC(obs.float().cuda(), None, noise=nz, inputs=v.float().cuda())
    torch.cuda.synchronize()
    for k in FILTER_KEYS + ("rs", "ess"):
        assert torch.equal(log["filter"][k], log0["filter"][k]), k
    B, T, N, Dx = run[0][1], run[0][2], run[0][3], run[0][5]
    assert log["Xs"].shape == (B, T, N, Dx) and log["X_map"].shape == (B, T, Dx) and log["X_smooth_mean"].shape == (B, T, Dx)
    for k in ("Xs", "X_map", "X_smooth_mean"):
        assert torch.isfinite(log[k]).all(), k


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """--noPSVO --AESMC --generateTrainingData --Di=1 --resample_ess=0.5 --resample_ess_inputs for two epochs: a finite ELBO
    history and the adaptive_* keys in every metric file"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    monkeypatch.chdir(tmp_path)
    FLAGS = parse_flags(["--noPSVO", "--AESMC", "--generateTrainingData", "--Di=1", "--resample_ess=0.5", "--resample_ess_inputs",
                         "--Dy=1", "--Dx=2", "--time=20", "--n_train=4", "--n_test=4", "--batch_size=4", "--n_particles=16",
                         "--epoch=2", "--print_freq=1", "--MSE_steps=3", "--saving_num=4"])
    hist = runner.main(FLAGS)
    torch.cuda.synchronize()
    for key in ("log_ZSMC_trains", "log_ZSMC_tests"):
        assert len(hist[key]) >= 2 and np.isfinite(np.asarray(hist[key], dtype=np.float64)).all(), (key, hist[key])
    metrics = glob.glob(str(tmp_path / "rslts" / "**" / "metric_*.p"), recursive=True)
    assert metrics
    keys = ["adaptive_%s_%s" % (s, split) for s in ("rate", "ess_mean", "ess_min") for split in ("train", "test")]
    for path in metrics:
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        assert set(keys) <= set(m), sorted(m)
        for split in ("train", "test"):
            assert 0.0 <= m["adaptive_rate_" + split] <= 1.0
            assert 1.0 / 16 - 1e-6 <= m["adaptive_ess_min_" + split] <= m["adaptive_ess_mean_" + split] <= 1.0 + 1e-5
