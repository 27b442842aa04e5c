"""Exogenous inputs (FLAGS.Di; psvo_filter_forward_wobs_input / psvo_filter_backward_wobs_input, the fifth compilation of
psvo_amd/csrc/filter_wobs_impl.h, and psvo_mlp_wgrad_rowbias) on the GPU against the fp64 reference of tests/exo_reference.py.

Cases: the smallest shapes at which these kernels can go wrong (see CASES) -- one wave staging 2 H = 128 bias words, a partly
filled wave, the IWAE reverse step that has no inner barrier, eight waves at every limit, and T = 60 for both halves of the row
buffer many times -- plus one run under --missing_obs (MR.mask) and one under --count_emission.  Inputs are ER.inputs: seeded
standard normals, different at every step and sequence; tests/test_exo_host.py asserts, in the reference alone, that rolling,
swapping or zeroing them moves logW by at least 100 x the value tolerance on every case.

Tolerances are the suite's own (tests/test_gpu_missing.py): values allclose with atol 2e-4 (X) / 5e-4 (logW, lse) and rtol 1e-5,
the ELBO 1e-4 relative with |ELBO| >= 1 asserted, gradients 2e-3 of a tensor's largest entry + 1e-6 with the fp32-reference
clause (K32).  Model seeds 3 (values) and 5 (gradients).  tools/exo_reference_error.py prints the fp32 reference's own error on
these runs (profiles/exo_inputs.md has the table)."""
import glob

import numpy as np
import pytest
import torch

from tests import exo_reference as ER
from tests import helpers as Hh
from tests import missing_reference as MR
from tests.test_gpu_instantiations import K32
from tests.test_gpu_large import EDGE_TOL
from tests.test_gpu_parity import _pairs, _setup

pytestmark = pytest.mark.gpu

CASES, RUNS, _id = ER.CASES, ER.RUNS, ER.run_id


def exo_setup(run, seed, **extra):
    """_setup of the suite with --Di (and the variant's flag).  Returns (FLAGS, model, smc, obs (B,T,Dy) fp64, v (B,T,Di) fp64, noise)"""
    case, Di, variant = run
    B, T, Dy = case[1], case[2], case[6]
    kw = dict(Di=Di)
    if variant == "missing":
        kw["missing_obs"] = True
    if variant == "count":
        kw["count_emission"] = True
    kw.update(extra)
    FLAGS, model, smc, obs, noise = _setup(*case, seed=seed, **kw)
    assert smc.Di == Di and model.Di == Di and not smc.wide_obs
    assert model.q1_tran.kernels[0].shape[0] == case[5] + Di
    obs = ER.observations(run, seed, obs)
    return FLAGS, model, smc, obs, ER.inputs(B, T, Di, seed), noise


def _teacher(ref):
    return {"idx_f": ref["idx_f"]} if ref["idx_f"] is not None else {}


def _hip_noise(noise, teacher):
    nz = Hh.noise_to_hip({**noise, **teacher}, "cuda")
    if "idx_f" in nz:
        nz.pop("u_f", None)
    return nz


_err = lambda a, b: float((a - b).abs().max())


def _assert_values(z, log, z_ref, ref):
    filt = log["filter"]
    lse_ref = torch.logsumexp(ref["log_Ws"], 1)
    print("max abs err: X %.3e logW %.3e lse %.3e ELBO rel %.3e (ELBO %.4f)" % (
        _err(Hh.part_to_ref(filt["X"]), ref["X_prevs"]), _err(Hh.w_to_ref(filt["logW"]), ref["log_Ws"]),
        _err(filt["lse"].double().cpu(), lse_ref), abs(float(z) - float(z_ref)) / abs(float(z_ref)), float(z_ref)))
    assert torch.allclose(Hh.part_to_ref(filt["X"]), ref["X_prevs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.part_to_ref(filt["Xanc"]), ref["X_ancestors"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(filt["lse"].double().cpu(), lse_ref, atol=5e-4, rtol=1e-5)
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)
    assert abs(float(z_ref)) >= 1.0                   # (the relative tolerance has something to stand on)
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_teacher_forced_values(built_lib, run):
    """X, Xanc, logW, lse, Xs and the ELBO against fp64; indices teacher-forced"""
    obj = run[0][0]
    FLAGS, model, smc, obs, v, noise = exo_setup(run, 3)
    z_ref, ref = ER.run(model, FLAGS, obj, obs, v, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, _teacher(ref)), inputs=v.float().cuda())
    torch.cuda.synchronize()
    assert smc._desc().emission == (2 if run[2] == "count" else 0)
    assert set(log["filter"]) == {"lse", "Fm", "logW", "X", "Xanc", "idx", "eps", "u"}
    assert ("missing" in log) == (run[2] == "missing")
    assert torch.isfinite(log["filter"]["logW"]).all() and torch.isfinite(log["filter"]["lse"]).all()
    _assert_values(z, log, z_ref, ref)


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_free_running_draws(built_lib, run):
    """in-kernel draws against the reference's definition: no index differs"""
    obj = run[0][0]
    FLAGS, model, smc, obs, v, noise = exo_setup(run, 3)
    z_ref, ref = ER.run(model, FLAGS, obj, obs, v, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"), inputs=v.float().cuda())
    torch.cuda.synchronize()
    differ = 0
    if ref["idx_f"] is not None:
        differ += int((log["filter"]["idx"].permute(0, 2, 1).cpu().long() != ref["idx_f"]).sum())
    if differ:
        _, _, st = ER.replay_with_hip_indices(model, FLAGS, obj, obs, v, noise, log)
        print("draws=%d differing=%d flipped=%d worst edge distance=%.3e" % (st["draws"], differ, st["off"], st["worst"]))
        assert st["worst"] <= EDGE_TOL, "a draw that is not on a CDF edge: %s" % st
    assert differ == 0, "%d draws differ from the reference's (edge flips: see the printed distances)" % differ
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_every_gradient(built_lib, run):
    """d log_ZSMC / d(every parameter tensor, the input rows W1[Dx:] of q1 / f included, and the inputs themselves),
    teacher-forced indices, against fp64 autograd of the reference"""
    obj, Dx = run[0][0], run[0][5]
    FLAGS, model, smc, obs, v, noise = exo_setup(run, 5)
    _, ref0 = ER.run(model, FLAGS, obj, obs, v, noise)
    teacher = _teacher(ref0)
    z_ref, P, dv_ref = ER.grads(model, FLAGS, obj, obs, v, noise, teacher)
    model.zero_grad()
    v_c = v.float().cuda().requires_grad_(True)
    z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, teacher), inputs=v_c)
    z.backward()
    torch.cuda.synchronize()
    assert abs(float(z.detach()) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    rows = [("inputs", float((v_c.grad.double().cpu() - dv_ref).abs().max()), max(float(dv_ref.abs().max()), 1e-6))]
    assert float(dv_ref.abs().max()) > 0
    for name, p, ref in _pairs(model, P):
        g = torch.zeros_like(ref) if p.grad is None else p.grad.detach().double().cpu()
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        assert torch.isfinite(g).all(), name
        rows.append((name, float((g - r).abs().max()), max(float(r.abs().max()), 1e-6)))
        if name in ("q1.W0", "f.W0"):       # the input rows on their own: they must not hide behind a larger state block
            assert float(r[Dx:].abs().max()) > 0, name
            rows.append((name + "[Dx:]", float((g[Dx:] - r[Dx:]).abs().max()), max(float(r[Dx:].abs().max()), 1e-6)))
    worst = max(rows, key=lambda r: r[1] / r[2])
    print("worst gradient error / largest entry: %s %.3e" % (worst[0], worst[1] / worst[2]))
    over = [r for r in rows if r[1] > 2e-3 * r[2] + 1e-6]
    if over:        # the second clause: the fp32 reference's own error on the same tensor (computed only when it is needed)
        _, P32, dv32 = ER.grads(model, FLAGS, obj, obs, v, noise, teacher, dtype=torch.float32)
        err32 = {"inputs": float((dv32.double() - dv_ref).abs().max())}
        for (name, _, ref), (_, _, ref32) in zip(_pairs(model, P), _pairs(model, P32)):
            r = torch.zeros_like(ref) if ref.grad is None else ref.grad
            r32 = torch.zeros_like(ref) if ref32.grad is None else ref32.grad.double()
            err32[name] = float((r32 - r).abs().max())
            if name in ("q1.W0", "f.W0"):
                err32[name + "[Dx:]"] = float((r32[Dx:] - r[Dx:]).abs().max())
        bad = [(n, e, s, err32[n]) for n, e, s in over if e > K32 * err32[n]]
        assert not bad, "gradient mismatch (name, max abs err, own scale, fp32 reference's own err): %s" % bad
    names = {r[0] for r in rows}
    assert {"q1.W0", "q1.W0[Dx:]", "q1.b0", "g.W0", "inputs"} <= names and ("f.W0[Dx:]" in names) == (not run[0][8])


@pytest.mark.parametrize("S,L,H", [(3, 16, 16), (5, 40, 64), (2, 512, 32)])
def test_wgrad_rowbias_alone(built_lib, S, L, H):
    """psvo_mlp_wgrad_rowbias on its own against fp64: grad, and dhb segment by segment (a segment that read its neighbour's
    bias row shows); two calls are bit-identical; accumulate adds into grad only"""
    from psvo_amd import ops
    Din = Dout = 3
    g = torch.Generator().manual_seed(40 + S)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    X, dOut, hb = rn(S, Din, L), rn(S, Dout, L), rn(S, H) * 1.5      # (rows differ by O(1): neighbours have other relu masks)
    W1, b1, W2, b2 = rn(Din, H) * 0.7, rn(H) * 0.3, rn(H, Dout) * 0.7, rn(Dout)
    Xr = X.permute(0, 2, 1)                                          # (S, L, Din)
    hbr = hb.clone().requires_grad_(True)
    ps = [p.clone().requires_grad_(True) for p in (W1, b1, W2, b2)]
    out = torch.relu(Xr @ ps[0] + (ps[1] + hbr)[:, None, :]) @ ps[2] + ps[3]
    (out * dOut.permute(0, 2, 1)).sum().backward()
    ref = torch.cat([p.grad.reshape(-1) for p in ps])
    dev = lambda t: t.float().cuda().contiguous()
    w = tuple(dev(p) for p in (W1, b1, W2, b2))
    res = [ops.mlp_wgrad_rowbias(dev(X), dev(dOut), dev(hb), w, Din, H, Dout, axis=1) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    grad, dhb = res[0][0].double().cpu(), res[0][1].double().cpu()
    assert dhb.shape == (S, H) and float(hbr.grad.abs().max()) > 0
    # fp32 sums of L (dhb) and S L (grad) products of O(1) terms: 2e-3 of the largest entry + 1e-6, the suite's gradient bound
    for s in range(S):
        e, scale = float((dhb[s] - hbr.grad[s]).abs().max()), float(hbr.grad[s].abs().max())
        print("segment %d: dhb err %.3e of %.3e" % (s, e, scale))
        assert e <= 2e-3 * scale + 1e-6, (s, e, scale)
        if S > 1:       # (the check can tell segments apart)
            assert float((hbr.grad[s] - hbr.grad[(s + 1) % S]).abs().max()) > 100 * (2e-3 * scale + 1e-6)
    a = Din * H
    for name, lo, hi in (("dW1", 0, a), ("db1", a, a + H), ("dW2", a + H, a + H + H * Dout), ("db2", a + H + H * Dout, None)):
        e, scale = float((grad[lo:hi] - ref[lo:hi]).abs().max()), float(ref[lo:hi].abs().max())
        print("%s err %.3e of %.3e" % (name, e, scale))
        assert e <= 2e-3 * scale + 1e-6, (name, e, scale)
    acc = torch.ones_like(res[0][0])
    g2, dhb2 = ops.mlp_wgrad_rowbias(dev(X), dev(dOut), dev(hb), w, Din, H, Dout, grad=acc, axis=1)
    torch.cuda.synchronize()
    assert torch.equal(dhb2, res[0][1]) and torch.allclose(g2, res[0][0] + 1.0, atol=1e-5 * float(res[0][0].abs().max()) + 1e-6)


def _step(smc, model, obs_c, v_c, nz):
    model.zero_grad(set_to_none=True)
    z, _ = smc.get_log_ZSMC(obs_c, None, noise=nz, inputs=v_c)
    z.backward()
    torch.cuda.synchronize()
    return z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("run", [RUNS[1], RUNS[3]], ids=_id)
def test_two_passes_are_bit_identical(built_lib, run, deterministic):
    """forward + backward twice in one process, with and without PSVO_DETERMINISTIC: the ELBO and every .grad bit for bit"""
    from psvo_amd import _lib, ops
    lib = _lib.load()
    key = _lib.PSVO_TUNE_DETERMINISTIC
    before = lib.psvo_get_tuning(key)
    try:
        _lib.check(lib.psvo_set_tuning(key, int(deterministic)), "psvo_set_tuning")
        assert ops.deterministic() == deterministic
        FLAGS, model, smc, obs, v, noise = exo_setup(run, 5)
        nz = Hh.noise_to_hip(noise, "cuda")
        res = [_step(smc, model, obs.float().cuda(), v.float().cuda(), nz) for _ in range(2)]
    finally:
        lib.psvo_set_tuning(key, before)
    assert torch.equal(res[0][0], res[1][0]) and torch.isfinite(res[0][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 8
    for n, g in res[0][1].items():
        assert torch.isfinite(g).all() and torch.equal(g, res[1][1][n]), n


def test_step_replays_from_hipgraph(built_lib):
    """one local training step of case 3, eager and captured into a GraphedStep: a replay equals the eager step bit for bit, and
    after the static input buffer is overwritten the replay follows the new inputs"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    run = RUNS[2]
    FLAGS, model, smc, obs, v, noise = exo_setup(run, 3)
    nz = Hh.noise_to_hip(noise, "cuda")
    flat = FlatParams(model)
    obs_c, s_v = obs.float().cuda(), v.float().cuda().clone()
    v2 = ER.inputs(run[0][1], run[0][2], run[1], 77).float().cuda()

    def local():
        flat.zero_grad()
        z, _ = smc.get_log_ZSMC(obs_c, None, noise=nz, inputs=s_v)
        z.backward()
        return z.detach()
    eager = []
    for src in (v.float().cuda(), v2):
        s_v.copy_(src)
        eager.append((local().clone(), flat.grad.clone()))
        torch.cuda.synchronize()
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][1], eager[1][1])
    s_v.copy_(v.float().cuda())
    step = GraphedStep(local)
    for src, (z_e, g_e) in ((v.float().cuda(), eager[0]), (v2, eager[1]), (v.float().cuda(), eager[0])):
        s_v.copy_(src)
        flat.grad.fill_(float("nan"))
        z_g = step()
        torch.cuda.synchronize()
        assert torch.isfinite(z_e) and torch.equal(z_g, z_e)
        assert torch.equal(flat.grad, g_e)


def test_di_zero_is_the_missing_route(built_lib):
    """--Di=0 under --missing_obs: the node, the launches and the bits of the route as it was -- no entry point of this feature is
    called, the forward values equal a direct launch of psvo_filter_forward_wobs_missing on the arguments the node was given, and
    ELBO and gradients repeat bit for bit"""
    from psvo_amd import ops
    case = CASES[2][0]
    B, T, Dy = case[1], case[2], case[6]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=5, missing_obs=True)
    assert FLAGS.Di == 0 and smc.Di == 0 and model.q1_tran.Di == 0 and model.q1_tran.kernels[0].shape[0] == case[5]
    obs = MR.knock_out(obs, MR.mask(B, T, Dy, 5)[0])
    nz = Hh.noise_to_hip(noise, "cuda")
    names, seen = [], {}
    real = ops.filter_forward_wobs_missing

    def spy(desc, *args, **kw):
        seen["args"], seen["desc"] = args, desc
        return real(desc, *args, **kw)
    ops.set_timing_hook(lambda name, phase, stream: names.append(name) if phase == 0 else None)
    ops.filter_forward_wobs_missing = spy
    try:
        res = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
            z.backward()
            torch.cuda.synchronize()
            res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
                        log["filter"]))
    finally:
        ops.set_timing_hook(None)
        ops.filter_forward_wobs_missing = real
    assert not [n for n in names if "input" in n or "rowbias" in n], names
    assert {"psvo_filter_forward_wobs_missing", "psvo_filter_backward_wobs_missing", "psvo_mlp_wgrad"} <= set(names)
    assert names[:len(names) // 2] == names[len(names) // 2:]
    assert torch.equal(res[0][0], res[1][0])
    for n, g in res[0][1].items():
        assert torch.equal(g, res[1][1][n]), n
    with torch.no_grad():
        direct = real(seen["desc"], *seen["args"])
    torch.cuda.synchronize()
    for key in ("X", "Xanc", "Fm", "logW", "lse", "idx"):
        assert torch.equal(direct[key], res[1][2][key]), key


@pytest.mark.parametrize("run", [RUNS[6], RUNS[1]], ids=_id)
def test_zero_input_rows_are_the_missing_route(built_lib, run):
    """--Di > 0 with W1[Dx:] = 0: every value equals the --missing_obs route of the same weights bit for bit"""
    case, Di, variant = run
    obj, Dx = case[0], case[5]
    FLAGS, model, smc, obs, v, noise = exo_setup(run, 3, missing_obs=True)
    with torch.no_grad():
        for tr in {model.q1_tran, model.f_tran}:
            tr.kernels[0][Dx:].zero_()
    F0, model0, smc0, _, _ = _setup(*case, seed=3, missing_obs=True)
    assert smc0.Di == 0 and smc0.missing_obs
    src = dict(model.named_parameters())
    with torch.no_grad():
        for n, p in model0.named_parameters():
            p.copy_(src[n][:Dx] if src[n].shape != p.shape else src[n])
    nz = Hh.noise_to_hip(noise, "cuda")
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz, inputs=v.float().cuda())
        z0, log0 = smc0.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    torch.cuda.synchronize()
    assert float(v.abs().max()) > 1
    for key in ("X", "Xanc", "Fm", "logW", "lse", "idx"):
        assert torch.equal(log["filter"][key], log0["filter"][key]), key
    assert torch.equal(z, z0) and torch.isfinite(z)


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """--generateTrainingData --Di=1 --noPSVO --AESMC for two epochs at tiny shapes, --FFBS --FFBSi --MAP_path behind it: finite
    ELBO history, metric files written"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    monkeypatch.chdir(tmp_path)
    FLAGS = parse_flags(["--noPSVO", "--AESMC", "--generateTrainingData", "--Di=1", "--Dy=1", "--Dx=2", "--time=20", "--n_train=4",
                         "--n_test=4", "--batch_size=4", "--n_particles=16", "--epoch=2", "--print_freq=1", "--MSE_steps=3",
                         "--saving_num=4", "--FFBS", "--FFBSi", "--MAP_path"])
    hist = runner.main(FLAGS)
    torch.cuda.synchronize()
    for key in ("log_ZSMC_trains", "log_ZSMC_tests"):
        assert len(hist[key]) >= 2 and np.isfinite(np.asarray(hist[key], dtype=np.float64)).all(), (key, hist[key])
    assert glob.glob(str(tmp_path / "rslts" / "**" / "metric_*.p"), recursive=True)
    assert glob.glob(str(tmp_path / "rslts" / "**" / "y_hat_*.p"), recursive=True)
