"""Wide observations (3 <= Dy <= 32) for the filter objectives SVO / AESMC / IWAE on the GPU: psvo_filter_forward_wobs,
psvo_filter_backward_wobs and psvo_mlp_wgrad_wobs (psvo_amd/csrc/filter_wobs.hip) against the fp64 oracle.

Cases are the smallest shapes that reach each way the kernels can go wrong (see CASES).  Tolerances are those of the plain
path: values as tests/test_gpu_parity.py::test_teacher_forced_parity, draws as ::test_free_running_indices (a differing draw is
reported through helpers.replay_with_hip_indices with its distance from the CDF edge, EDGE_TOL of tests/test_gpu_large.py),
gradients under the rule of tests/test_gpu_instantiations.py (2e-3 of a tensor's largest entry, or K32 = 4 times the fp32
oracle's own error on that tensor; on these cases the fp32 oracle stays below 1 % of the first bound, which is the one that
binds), the weight gradient on its own as tests/test_gpu_golden.py::test_mlp_wgrad_kernels, the smoother as
tests/test_gpu_ffbs.py."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import psvo_oracle as O
from tests import ffbs_reference as R
from tests import helpers as Hh
from tests import test_gpu_ffbs as TF
from tests.test_gpu_instantiations import K32
from tests.test_gpu_large import EDGE_TOL
from tests.test_gpu_parity import _check_grads, _oracle_grads, _pairs, _setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

CASES = [
    # (objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q), extra flags
    (("AESMC", 2, 6, 16, 1, 2, 3, 16, True, True), {}),              # smallest wide Dy; N under one wave
    (("AESMC", 2, 7, 100, 1, 3, 10, 32, False, True), {}),           # Lorenz shape; N not a wave multiple; separate f
    (("SVO", 2, 8, 32, 1, 2, 20, 32, True, True), {}),               # vind shape; encoder input width 20
    (("IWAE", 2, 8, 96, 1, 3, 32, 64, True, True), {}),              # widest Dy; no resampling
    (("SVO", 2, 6, 130, 1, 3, 17, 64, True, False), {}),             # odd Dy; N > 128; no q2
    (("AESMC", 2, 5, 300, 1, 4, 5, 64, False, False), {}),           # Dx 4; N > 256
    (("AESMC", 2, 6, 40, 1, 2, 10, 32, True, True), dict(poisson_emission=True)),
    (("AESMC", 1, 5, 512, 1, 4, 32, 32, False, True), {}),           # every limit at once
    (("AESMC", 1, 120, 64, 1, 3, 10, 32, True, True), {}),           # long recurrence
]
LORENZ_CASE = CASES[1]
NEW_TENSORS = ("g.W0", "g.b0", "g.Wmu", "g.bmu", "g.sigma")          # what this feature newly produces


def _id(v):
    if isinstance(v, tuple):
        return "-".join(map(str, v))
    return ",".join(sorted(v)) or "plain"


def _teacher(ref):
    return {"idx_f": ref["idx_f"]} if ref["idx_f"] is not None else {}


def _hip_noise(noise, teacher):
    nz = Hh.noise_to_hip({**noise, **teacher}, "cuda")
    if "idx_f" in nz:
        nz.pop("u_f", None)
    return nz


@pytest.mark.parametrize("case,extra", CASES, ids=_id)
def test_teacher_forced_values(built_lib, case, extra):
    """X, Xanc, logW, lse, Xs and the ELBO against the fp64 oracle at the tolerances of test_teacher_forced_parity.

    The random model is the one of seed 3, the seed of the free-running test, not _setup's default 0.  What decides is the
    oracle alone: with seed 0 the T = 120 model is expansive along the teacher-forced ancestry, and the oracle evaluated in
    fp32 leaves its own fp64 values by 6.8e-2 in X and 1.08 in logW at t = 119 (320 and 1200 times the tolerance; the error
    grows from 6e-7 at t = 0 by about a factor of 3 per 10 steps), so no fp32 evaluation can meet an absolute 2e-4 there and
    the comparison would measure that model's sensitivity, not the kernel.  With seed 3 the fp32 oracle stays below 7 % of
    every tolerance on all nine cases (T = 120: 1.0e-6 in X, 2.7e-5 in logW), so a failure here is the kernel's."""
    obj = case[0]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=3, **extra)
    assert smc.wide_obs
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    nz = _hip_noise(noise, _teacher(ref))
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    torch.cuda.synchronize()
    filt = log["filter"]
    print("max abs err: X %.3e logW %.3e lse %.3e ELBO rel %.3e" % (
        float((Hh.part_to_ref(filt["X"]) - ref["X_prevs"]).abs().max()),
        float((Hh.w_to_ref(filt["logW"]) - ref["log_Ws"]).abs().max()),
        float((filt["lse"].double().cpu() - torch.logsumexp(ref["log_Ws"], 1)).abs().max()),
        abs(float(z) - float(z_ref)) / abs(float(z_ref))))
    assert torch.allclose(Hh.part_to_ref(filt["X"]), ref["X_prevs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.part_to_ref(filt["Xanc"]), ref["X_ancestors"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(filt["lse"].double().cpu(), torch.logsumexp(ref["log_Ws"], 1), atol=5e-4, rtol=1e-5)
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))


@pytest.mark.parametrize("case,extra", CASES, ids=_id)
def test_free_running_draws(built_lib, case, extra):
    """in-kernel multinomial draws against the oracle's definition: no index differs"""
    obj = case[0]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=3, **extra)
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()
    if ref["idx_f"] is not None:
        idx = log["filter"]["idx"].permute(0, 2, 1).cpu().long()
        differ = int((idx != ref["idx_f"]).sum())
        if differ:
            _, _, st = Hh.replay_with_hip_indices(model, FLAGS, obj, obs, noise, log)
            print("draws=%d differing=%d flipped=%d worst edge distance=%.3e" % (st["draws"], differ, st["off"], st["worst"]))
            assert st["worst"] <= EDGE_TOL, "a draw that is not on a CDF edge: %s" % st
        assert differ == 0, "%d draws differ from the oracle's (edge flips: see the printed distances)" % differ
    else:
        n = torch.arange(case[3], dtype=torch.int32, device="cuda")
        assert torch.equal(log["filter"]["idx"], n.expand_as(log["filter"]["idx"]))
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)


WORST = {}       # case id -> (tensor, error / its tensor's largest entry): printed for profiles/wobs_filter.md


@pytest.mark.parametrize("case,extra", CASES, ids=_id)
def test_every_gradient(built_lib, case, extra):
    """d log_ZSMC / d(every parameter), teacher-forced indices, against fp64 autograd of the oracle"""
    obj = case[0]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=5, **extra)
    _, ref0 = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = _teacher(ref0)
    z_ref, P = _oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    nz = _hip_noise(noise, teacher)
    model.zero_grad()
    z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    z.backward()
    torch.cuda.synchronize()
    assert abs(float(z.detach()) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    rows = []
    for name, p, ref in _pairs(model, P):
        g = torch.zeros_like(ref) if p.grad is None else p.grad.detach().double().cpu()
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        rows.append((name, float((g - r).abs().max()), max(float(r.abs().max()), 1e-6)))
    names = [n for n, _, _ in rows]
    assert all(n in names for n in NEW_TENSORS if not (n == "g.sigma" and extra.get("poisson_emission")))
    worst = max(rows, key=lambda r: r[1] / r[2])
    WORST[_id(case)] = (worst[0], worst[1] / worst[2])
    print("worst gradient error / largest entry: %s %.3e" % WORST[_id(case)])
    over = [r for r in rows if r[1] > 2e-3 * r[2] + 1e-6]
    if over:        # the second clause: the fp32 oracle's own error on the same tensor (computed only when it is needed)
        _, P32 = _oracle_grads(model, FLAGS, obj, obs, noise, teacher, dtype=torch.float32)
        err32 = {}
        for (name, _, ref), (_, _, ref32) in zip(_pairs(model, P), _pairs(model, P32)):
            r = torch.zeros_like(ref) if ref.grad is None else ref.grad
            r32 = torch.zeros_like(ref) if ref32.grad is None else ref32.grad.double()
            err32[name] = float((r32 - r).abs().max())
        bad = [(n, e, s, err32[n]) for n, e, s in over if e > K32 * err32[n]]
        assert not bad, ("gradient mismatch (name, max abs err, own scale, fp32 oracle's own err) -- g's tensors %s are the ones "
                         "the wide-observation kernels newly produce: %s" % (list(NEW_TENSORS), bad))


@pytest.mark.parametrize("case,extra", [CASES[1], CASES[3]], ids=_id)
def test_two_passes_are_bit_identical(built_lib, case, extra):
    """forward + backward twice in one process, deterministic mode off: the ELBO and every .grad bit for bit"""
    from psvo_amd import ops
    assert not ops.deterministic()
    FLAGS, model, smc, obs, noise = _setup(*case, seed=5, **extra)
    nz = Hh.noise_to_hip(noise, "cuda")
    res = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        z.backward()
        torch.cuda.synchronize()
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 4
    for n, g in res[0][1].items():
        assert torch.isfinite(g).all() and torch.equal(g, res[1][1][n]), n


# ---- psvo_mlp_wgrad_wobs on its own ----------------------------------------------------------------------------------------
def _wgrad_case(shape, Din, H, Dout):
    """rows, an MLP, the kernel's result and the fp64 gradients (the relu mask as the kernel's f32 fma chain sees it:
    tests/test_gpu_golden.py::test_mlp_wgrad_kernels)"""
    g = torch.Generator().manual_seed(sum(shape) + H + 10 * Din + Dout)
    X = torch.randn(*(shape[:2] + (Din,) + shape[3:]), generator=g)
    dOut = torch.randn(*(shape[:2] + (Dout,) + shape[3:]), generator=g)
    W1 = torch.randn(Din, H, generator=g) / Din ** 0.5
    b1 = 0.3 * torch.randn(H, generator=g)
    W2 = torch.randn(H, Dout, generator=g) / H ** 0.5
    b2 = 0.3 * torch.randn(Dout, generator=g)
    w = tuple(t.cuda() for t in (W1, b1, W2, b2))
    Xc, dc = X.cuda(), dOut.cuda()
    ps = [t.double().cuda().requires_grad_(True) for t in (W1, b1, W2, b2)]
    rows = Xc.double().movedim(2, -1).reshape(-1, Din)
    pre = b1.cuda()[None, :].expand(rows.shape[0], H)
    for i in range(Din):
        pre = (rows[:, i:i + 1] * ps[0][i].detach()[None, :] + pre.double()).float()
    out = ((rows @ ps[0] + ps[1]) * (pre > 0)) @ ps[2] + ps[3]
    out.backward(dc.double().movedim(2, -1).reshape(-1, Dout))
    return Xc, dc, w, ps


def _wgrad_check(shape, Din, H, Dout):
    from psvo_amd import ops
    Xc, dc, w, ps = _wgrad_case(shape, Din, H, Dout)
    got = ops.mlp_wgrad_wobs(Xc, dc, w, Din, H, Dout)                     # accumulate = 0
    torch.cuda.synchronize()
    assert got.numel() == ops.mlp_grad_size(Din, H, Dout)
    off = 0
    for name, t in zip(("dW1", "db1", "dW2", "db2"), ps):
        a, b = got[off:off + t.numel()].double(), t.grad.reshape(-1)
        err = float((a - b).abs().max())
        print("%s Din=%d H=%d Dout=%d: max abs err %.3e of largest entry %.3e" % (name, Din, H, Dout, err, float(b.abs().max())))
        assert torch.allclose(a, b, atol=1e-4 * float(b.abs().max()) + 1e-6, rtol=1e-4), (name, Din, H, Dout)
        off += t.numel()
    acc = torch.ones_like(got)
    ops.mlp_wgrad_wobs(Xc, dc, w, Din, H, Dout, grad=acc)                 # accumulate = 1
    again = ops.mlp_wgrad_wobs(Xc, dc, w, Din, H, Dout)
    torch.cuda.synchronize()
    assert torch.allclose(acc, got + 1.0, atol=1e-5 * float(got.abs().max()) + 1e-6, rtol=1e-5)
    assert torch.equal(again, got)                                        # fixed-order sums


@pytest.mark.parametrize("Din", [2, 3, 4])
@pytest.mark.parametrize("H", [16, 32, 64])
@pytest.mark.parametrize("Dout", [3, 5, 10, 17, 20, 32])
def test_mlp_wgrad_wobs(built_lib, Dout, H, Din):
    """S = 7 segments of L = 37 rows: 259 rows, no multiple of the 64-row tile, segments straddling tiles"""
    _wgrad_check((7, 1, 0, 37), Din, H, Dout)


def test_mlp_wgrad_wobs_many_rows(built_lib):
    """40 x 3 segments of 33 rows (3960 rows): several workgroups, several tiles per workgroup, a ragged last tile"""
    _wgrad_check((40, 3, 0, 33), 3, 32, 10)


# ---- the smoother behind a wide filter -------------------------------------------------------------------------------------
def test_ffbs_behind_the_wide_filter(built_lib, monkeypatch):
    """--FFBS at Dy = 10: smoothed weights, ess_smooth and X_smooth_mean against tests/ffbs_reference.py on the wide filter's own
    outputs (yardstick of tests/test_gpu_ffbs.py); with autograd on, the ELBO and gradients are bit-identical with and without"""
    from psvo_amd import ops
    case = ("AESMC", 2, 7, 100, 1, 3, 10, 32, False, True)
    obj, B, T, N, M, Dx = case[:6]
    FLAGS, model, cls, obs, noise = TF._setup(*case, FFBS=True)
    smc = cls(model, FLAGS)
    assert smc.wide_obs and smc.FFBS
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs, None, noise=noise)
    torch.cuda.synchronize()
    filt = log["filter"]
    assert log["Xs"].shape == (B, T, N, Dx) and log["X_smooth_mean"].shape == (B, T, Dx) and log["ess_smooth"].shape == (B, T)
    X, Fm, logW = (filt[k].cpu() for k in ("X", "Fm", "logW"))
    S = R.scales(model.f_dist.get_sigma().detach().float().cpu(), T, B, Dx, N, dtype=torch.float32)
    q64 = R.quantities(X.double(), Fm.double(), S.double(), logW.double())
    q32 = R.quantities(X, Fm, S, logW)
    hip = {"p": log["logW_smooth"].double().cpu().exp(), "Xmean": log["X_smooth_mean"].transpose(0, 1).double().cpu(),
           "ess": log["ess_smooth"].transpose(0, 1).double().cpu()}
    for v in hip.values():
        assert torch.isfinite(v).all()
    TF._yardstick("wobs-" + _id(case), hip, q64, q32)
    sm = log["smoother"]
    TF._check_draws(log["logW_smooth"], noise["u_s"], sm["idx"], filt["X"], sm["Xs"])

    def refuse(*a, **k):
        raise AssertionError("ops.ffbs_smooth was called under autograd")
    monkeypatch.setattr(ops, "ffbs_smooth", refuse)
    res = []
    for ffbs in (True, False):
        smc = cls(model, Hh.make_flags(obj, **{**FLAGS.as_dict(), "FFBS": ffbs}))
        model.zero_grad(set_to_none=True)
        z, _ = smc.get_log_ZSMC(obs, None, noise=noise)
        z.backward()
        torch.cuda.synchronize()
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 4
    for n, g in res[0][1].items():
        assert torch.equal(g, res[1][1][n]), n


# ---- the training step ---------------------------------------------------------------------------------------------------
def test_step_replays_from_hipgraph(built_lib):
    """one local training step at the Lorenz-shaped case, eager and captured into a GraphedStep: a replay equals the eager step
    bit for bit (the wide kernels sum in fixed orders), and rewrites every gradient itself"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    case, extra = LORENZ_CASE
    FLAGS, model, smc, obs, noise = _setup(*case, seed=3, **extra)
    nz = Hh.noise_to_hip(noise, "cuda")
    flat = FlatParams(model)
    obs_c = obs.float().cuda()

    def local():
        flat.zero_grad()
        z, _ = smc.get_log_ZSMC(obs_c, None, noise=nz)
        z.backward()
        return z.detach()
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


def _run_main(tmp_path, monkeypatch, name, data, argv, Dx, Dy):
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    work = tmp_path / name
    work.mkdir()
    with open(work / "datadict", "wb") as f:          # the loader's format, as tests/notebook_curve.py feeds fhn_notebook.npz
        pickle.dump({k: v.astype(np.float64) for k, v in data.items()}, f)
    monkeypatch.chdir(work)
    FLAGS = parse_flags(["--noPSVO", "--Dx=%d" % Dx, "--Dy=%d" % Dy, "--datadir=%s/" % work, "--datadict=datadict",
                         "--epoch=2", "--print_freq=1", "--MSE_steps=5", "--saving_num=4", "--save_trajectory"] + argv)
    hist = runner.main(FLAGS)
    torch.cuda.synchronize()
    for key in ("log_ZSMC_trains", "log_ZSMC_tests"):
        assert len(hist[key]) >= 2 and np.isfinite(np.asarray(hist[key], dtype=np.float64)).all(), (key, hist[key])
    for key in ("R_square_trains", "R_square_tests"):
        for r in hist[key]:
            r = np.asarray(r, dtype=np.float64)
            assert r.shape == (FLAGS.MSE_steps + 1,) and np.isfinite(r).all(), (key, r)
    metrics = glob.glob(str(work / "rslts" / "**" / "metric_*.p"), recursive=True)
    assert metrics
    return FLAGS, hist, work


def test_runner_on_the_lorenz_slice(built_lib, tmp_path, monkeypatch):
    d = np.load(os.path.join(GOLDEN, "lorenz_slice.npz"))
    data = {"Ytrain": d["Ytrain"], "Yvalid": d["Yvalid"]}
    FLAGS, hist, work = _run_main(tmp_path, monkeypatch, "lorenz", data, ["--AESMC", "--n_particles=32", "--batch_size=4"], 3, 10)
    assert (FLAGS.n_train, FLAGS.n_test, FLAGS.time) == (8, 4, 100)


def test_runner_on_the_vind_slice_with_ffbs(built_lib, tmp_path, monkeypatch):
    d = np.load(os.path.join(GOLDEN, "vind_slice.npz"))
    data = {"Ytrain": d["Ytrain"], "Yvalid": d["Yvalid"], "Xtrain": d["Xtrain"], "Xtest": d["Xvalid"]}
    FLAGS, hist, work = _run_main(tmp_path, monkeypatch, "vind", data,
                                  ["--SVO", "--FFBS", "--n_particles=16", "--batch_size=4"], 2, 20)
    assert (FLAGS.n_train, FLAGS.n_test, FLAGS.time) == (8, 4, 30)
    for path in glob.glob(str(work / "rslts" / "**" / "metric_*.p"), recursive=True):
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        for split in ("train", "test"):
            assert 1 <= m["ffbs_ess_min_" + split] <= m["ffbs_ess_mean_" + split] <= 16


# ---- what the wide kernels do not cover ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,extra,word", [
    (("PSVO", 2, 5, 16, 4, 2, 3, 32, True, True), {}, "PSVO"),
    (("PSVOwR", 2, 5, 16, 4, 2, 3, 32, True, True), {}, "PSVO"),
    (("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True), dict(output_cov=True, diag_cov=True), "output_cov"),
    (("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True), dict(q1_layers="32,32", g_layers="32,32"), "one hidden layer"),
    (("AESMC", 2, 5, 16, 1, 2, 33, 32, True, True), {}, "32"),
], ids=["PSVO", "PSVOwR", "output_cov", "two-layers", "Dy33"])
def test_refusals(built_lib, case, extra, word):
    with pytest.raises(ValueError, match=word):
        _setup(*case, **extra)
