"""Missing observations (FLAGS.missing_obs; psvo_filter_forward_wobs_missing / psvo_filter_backward_wobs_missing, the third
compilation of psvo_amd/csrc/filter_wobs_impl.h) on the GPU against the fp64 reference of tests/missing_reference.py.

Cases are the smallest shapes at which these kernels can go wrong (see CASES); the count form runs on three of them.  The mask
is MR.mask: seeded, the same for the reference and the kernel, asserted in _missing.  It holds about 30 % of the entries missing
independently, one step with every output missing, one output missing at every step (Dy >= 2), where B = 2 sequence 1 missing
from t = T-2 on, and step 0 of sequence 0 observed in every output but the never-observed one.  On the B = 2 shapes these
elements together leave 21 .. 47 % of the entries observed (the empty step and the ragged tail alone take 40 % of a T = 5
batch), so "at least half observed" is asserted on the B = 1 shapes, where it can hold; what that share is for -- an ELBO large
enough for a relative tolerance -- is asserted directly on every case: |ELBO| >= 1.

Tolerances are the suite's own (tests/test_gpu_count.py): values allclose with atol 2e-4 (X) / 5e-4 (logW, lse) and rtol 1e-5,
the ELBO 1e-4 relative, gradients 2e-3 of a tensor's largest entry + 1e-6 with the fp32-reference clause (K32).  Seeds as there:
model seed 3 for values and draws, 5 for gradients.

What backs the tolerances: the fp32 reference on the CPU against its own fp64 values, on these ten cases with these seeds, masks
and the tests' own models (tools/missing_reference_error.py prints the table; profiles/missing_obs.md has it):
    X 1.1e-05, logW 1.4e-03 (where |logW| reaches 3250: the IWAE case, whose weights accumulate without resampling; 8.6e-05 on
    every other case), lse 4.1e-05, ELBO 1.3e-07 relative, 0.079 of the allclose bound atol + rtol |reference| over every
    compared element (the IWAE case; 0.032 or less on every other case), gradients 4.1e-06 of a tensor's largest entry (the
    bound is 2e-3); the smallest |ELBO| is 7.6 (seed 3) / 5.5 (seed 5),
each well below a third of its tolerance, so a failure here is the kernel's, not the model's."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch

from tests import count_reference as CR
from tests import helpers as Hh
from tests import missing_reference as MR
from tests.test_gpu_instantiations import K32
from tests.test_gpu_large import EDGE_TOL
from tests.test_gpu_parity import _pairs, _setup
from tests.test_gpu_wobs import _run_main

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

CASES = [
    # (objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q)
    ("AESMC", 2, 5, 16, 1, 2, 1, 16, True, True),          # Dy = 1, the plain weight gradient, one wave
    ("SVO", 2, 6, 40, 1, 3, 2, 32, False, True),           # Dy = 2, separate f, bi-LSTM on zero-filled input, partly filled wave
    ("AESMC", 2, 5, 16, 1, 2, 3, 16, True, True),          # smallest wide Dy and H
    ("SVO", 2, 6, 40, 1, 3, 10, 32, False, True),          # Lorenz widths
    ("IWAE", 2, 5, 24, 1, 4, 17, 64, True, False),         # no resampling, no q2, odd Dy, the 32-unit chunks of bwd_input
    ("AESMC", 1, 4, 512, 1, 4, 32, 32, False, True),       # the 512-lane kernels at every limit
    ("SVO", 1, 60, 32, 1, 3, 10, 32, True, True),          # long recurrence, both halves of the row buffer many times
]
# (case, count emission): every case with the Gaussian emission, cases 3, 4 and 6 again with the count form
RUNS = [(c, False) for c in CASES] + [(CASES[2], True), (CASES[3], True), (CASES[5], True)]
_id = lambda r: "-".join(map(str, r[0])) + ("-count" if r[1] else "")


def _missing(run, seed, mask=True, **extra):
    """_setup of the suite under --missing_obs (and --count_emission), the observations knocked out by MR.mask.
    Returns (FLAGS, model, smc, obs with NaN (B,T,Dy) fp64, noise, e_never)"""
    case, count = run
    obj, B, T, Dy = case[0], case[1], case[2], case[6]
    kw = dict(missing_obs=True, **({"count_emission": True} if count else {}))
    kw.update(extra)
    FLAGS, model, smc, obs, noise = _setup(*case, seed=seed, **kw)
    assert smc.missing_obs and model.missing_obs and not smc.wide_obs
    if count:
        obs = CR.counts(B, T, Dy, 100 + seed)
    if not mask:
        return FLAGS, model, smc, obs, noise, None
    miss, t_all, e_never = MR.mask(B, T, Dy, seed)
    # the pattern, asserted
    assert torch.equal(miss, MR.mask(B, T, Dy, seed)[0])
    assert bool(miss[:, t_all].all()) and (e_never is None) == (Dy == 1)
    rest = [e for e in range(Dy) if e != e_never]
    assert e_never is None or bool(miss[:, :, e_never].all())
    assert not bool(miss[0, 0, rest].any())
    free = torch.ones(B, T, Dy, dtype=torch.bool)
    free[:, t_all] = False
    free[0, 0] = False
    if e_never is not None:
        free[:, :, e_never] = False
    if B == 2:
        assert bool(miss[1, T - 2:].all())
        free[1, T - 2:] = False
    n, k = int(free.sum()), int(miss[free].sum())
    assert abs(k - MR.RATE * n) <= 4.0 * (MR.RATE * (1 - MR.RATE) * n) ** 0.5, (k, n)      # about 30 % of the rest, independently
    observed = 1.0 - float(miss.float().mean())
    assert observed >= (0.5 if B == 1 else 0.2), observed
    obs = MR.knock_out(obs, miss)
    assert torch.equal(torch.isnan(obs), miss)
    return FLAGS, model, smc, obs, noise, e_never


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
    FLAGS, model, smc, obs, noise, _ = _missing(run, 3)
    z_ref, ref = MR.run_oracle(model, FLAGS, obj, obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, _teacher(ref)))
    torch.cuda.synchronize()
    assert smc._desc().emission == (2 if run[1] else 0)
    assert torch.equal(log["missing"].cpu(), torch.isnan(obs)) and log["missing"].dtype == torch.bool
    assert set(log["filter"]) == {"lse", "Fm", "logW", "X", "Xanc", "idx", "eps", "u"}
    assert torch.isfinite(log["filter"]["logW"]).all() and torch.isfinite(log["filter"]["lse"]).all()
    _assert_values(z, log, z_ref, ref)


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_free_running_draws(built_lib, run):
    """in-kernel draws against the reference's definition: no index differs"""
    obj = run[0][0]
    FLAGS, model, smc, obs, noise, _ = _missing(run, 3)
    z_ref, ref = MR.run_oracle(model, FLAGS, obj, obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()
    differ = 0
    if ref["idx_f"] is not None:
        differ += int((log["filter"]["idx"].permute(0, 2, 1).cpu().long() != ref["idx_f"]).sum())
    if differ:
        _, _, st = MR.replay_with_hip_indices(model, FLAGS, obj, obs, noise, log)
        print("draws=%d differing=%d flipped=%d worst edge distance=%.3e" % (st["draws"], differ, st["off"], st["worst"]))
        assert st["worst"] <= EDGE_TOL, "a draw that is not on a CDF edge: %s" % st
    assert differ == 0, "%d draws differ from the reference's (edge flips: see the printed distances)" % differ
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)


def _compare_gradients(model, FLAGS, obj, obs, noise, teacher, P):
    rows = []
    for name, p, ref in _pairs(model, P):
        g = torch.zeros_like(ref) if p.grad is None else p.grad.detach().double().cpu()
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        assert torch.isfinite(g).all(), name
        rows.append((name, float((g - r).abs().max()), max(float(r.abs().max()), 1e-6)))
    worst = max(rows, key=lambda r: r[1] / r[2])
    print("worst gradient error / largest entry: %s %.3e" % (worst[0], worst[1] / worst[2]))
    over = [r for r in rows if r[1] > 2e-3 * r[2] + 1e-6]
    if over:        # the second clause: the fp32 reference's own error on the same tensor (computed only when it is needed)
        _, P32 = MR.oracle_grads(model, FLAGS, obj, obs, noise, teacher, dtype=torch.float32)
        err32 = {}
        for (name, _, ref), (_, _, ref32) in zip(_pairs(model, P), _pairs(model, P32)):
            r = torch.zeros_like(ref) if ref.grad is None else ref.grad
            r32 = torch.zeros_like(ref) if ref32.grad is None else ref32.grad.double()
            err32[name] = float((r32 - r).abs().max())
        bad = [(n, e, s, err32[n]) for n, e, s in over if e > K32 * err32[n]]
        assert not bad, "gradient mismatch (name, max abs err, own scale, fp32 reference's own err): %s" % bad
    return [n for n, _, _ in rows]


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_every_gradient(built_lib, run):
    """d log_ZSMC / d(every parameter), teacher-forced indices, against fp64 autograd of the reference; the never-observed
    output's column of the output layer, its bias and its scale get exactly 0.0 on the GPU, every other g.* gradient is there"""
    obj, count = run[0][0], run[1]
    FLAGS, model, smc, obs, noise, e_never = _missing(run, 5)
    _, ref0 = MR.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = _teacher(ref0)
    z_ref, P = MR.oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    model.zero_grad()
    z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, teacher))
    z.backward()
    torch.cuda.synchronize()
    assert abs(float(z.detach()) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    names = _compare_gradients(model, FLAGS, obj, obs, noise, teacher, P)
    assert {"g.W0", "g.b0", "g.Wmu", "g.bmu"} <= set(names) and ("g.sigma" in names) == (not count)
    Dy = run[0][6]
    others = [e for e in range(Dy) if e != e_never]
    for name, p, ref in _pairs(model, P):
        if not name.startswith("g."):
            continue
        assert p.grad is not None, name
        g = p.grad.detach().cpu()
        if name in ("g.W0", "g.b0"):
            assert float(g.abs().max()) > 0 and float(ref.grad.abs().max()) > 0, name
            continue
        cols = g if g.dim() == 1 else g.abs().amax(0)           # g.Wmu (H, Dy) by output; g.bmu, g.sigma (Dy,)
        if e_never is not None:
            col = g[e_never] if g.dim() == 1 else g[:, e_never]
            assert bool((col == 0.0).all()), (name, col)
            rcol = ref.grad[e_never] if g.dim() == 1 else ref.grad[:, e_never]
            assert bool((rcol == 0.0).all()), name
        if name == "g.sigma":       # (a scale held at its floor g_sigma_min has no gradient: the reference says where)
            rcols = ref.grad.abs()
            assert bool(((cols[others].abs() > 0) == (rcols[others] > 0)).all()) and bool((rcols[others] > 0).any()), (name, cols)
        else:
            assert bool((cols[others].abs() > 0).all()), (name, cols)


@pytest.mark.parametrize("count", [False, True], ids=["gaussian", "count"])
def test_nothing_observed(built_lib, count):
    """case 3's shape with every entry NaN: lse, logW and every gradient finite; lse within atol 5e-4 of the reference (the ELBO is
    near 0 there, so no relative comparison); no gradient reaches the emission network"""
    run = (CASES[2], count)
    obj = run[0][0]
    FLAGS, model, smc, obs, noise, _ = _missing(run, 5, mask=False)
    obs = torch.full_like(obs, float("nan"))
    _, ref = MR.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = _teacher(ref)
    _, P = MR.oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    model.zero_grad()
    z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, teacher))
    z.backward()
    torch.cuda.synchronize()
    filt = log["filter"]
    assert torch.isfinite(z) and torch.isfinite(filt["lse"]).all() and torch.isfinite(filt["logW"]).all()
    assert bool(log["missing"].all())
    print("nothing observed: ELBO %.6f (reference %.6f), lse err %.3e" % (
        float(z.detach()), float(torch.logsumexp(ref["log_Ws"], 1).sum(0).mean()),
        _err(filt["lse"].detach().double().cpu(), torch.logsumexp(ref["log_Ws"], 1))))
    assert torch.allclose(filt["lse"].detach().double().cpu(), torch.logsumexp(ref["log_Ws"], 1), atol=5e-4, rtol=0.0)
    seen = 0
    for name, p, r in _pairs(model, P):
        if p.grad is None:
            continue
        assert torch.isfinite(p.grad).all(), name
        seen += 1
        if name.startswith("g."):
            assert float(p.grad.abs().max()) == 0.0, name
    assert seen > 8
    _compare_gradients(model, FLAGS, obj, obs, noise, teacher, P)


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_all_observed_is_the_static_route(built_lib, run):
    """nothing missing: the missing route agrees with the route the same model takes without the flag -- the static wide kernels
    at Dy >= 3, the plain kernels (FilterFunction) at Dy <= 2 -- within the value tolerances, with identical draws"""
    case, count = run
    obj, Dy = case[0], case[6]
    FLAGS, model, smc, obs, noise, _ = _missing(run, 3, mask=False)
    assert not bool(torch.isnan(obs).any())
    model.missing_obs = False           # (the same weights on the route without the flag)
    plain = type(smc)(model, Hh.make_flags(obj, **{**FLAGS.as_dict(), "missing_obs": False}))
    assert not plain.missing_obs and plain.wide_obs == (Dy >= 3)
    nz = Hh.noise_to_hip(noise, "cuda")
    out = []
    for s in (smc, plain):
        with torch.no_grad():
            z, log = s.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        torch.cuda.synchronize()
        out.append((z, log["filter"], log["Xs"]))
    (z_m, f_m, xs_m), (z_p, f_p, xs_p) = out
    print("missing vs static route: X %.3e logW %.3e lse %.3e" % (
        _err(f_m["X"], f_p["X"]), _err(f_m["logW"], f_p["logW"]), _err(f_m["lse"], f_p["lse"])))
    assert torch.equal(f_m["idx"], f_p["idx"])
    assert torch.allclose(f_m["X"], f_p["X"], atol=2e-4, rtol=1e-5) and torch.allclose(f_m["Xanc"], f_p["Xanc"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(f_m["logW"], f_p["logW"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(f_m["lse"], f_p["lse"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(xs_m, xs_p, atol=2e-4, rtol=1e-5)
    assert abs(float(z_m) - float(z_p)) <= 1e-4 * abs(float(z_p))


def test_all_observed_count_needs_the_flag_at_small_dy(built_lib):
    """the count emission at Dy <= 2 exists on the missing route only"""
    case = ("AESMC", 2, 5, 16, 1, 2, 2, 16, True, True)
    with pytest.raises(ValueError, match="no count form"):
        _setup(*case, count_emission=True)
    FLAGS, model, smc, obs, noise = _setup(*case, seed=3, count_emission=True, missing_obs=True)
    obs = CR.counts(2, 5, 2, 103)
    z_ref, ref = MR.run_oracle(model, FLAGS, "AESMC", obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, _teacher(ref)))
    torch.cuda.synchronize()
    _assert_values(z, log, z_ref, ref)


def test_causality(built_lib, monkeypatch):
    """case 4 with sequence 0 missing from t = L on: X, logW and lse of t < L are bit-identical to a launch at T = L on the same
    inputs truncated (same instantiation, same code: what a step computes depends on nothing behind it)"""
    from psvo_amd import ops
    run = (CASES[3], False)
    FLAGS, model, smc, obs, noise, _ = _missing(run, 3)
    T, L = run[0][2], 4
    obs[0, L:] = float("nan")
    seen = {}
    real = ops.filter_forward_wobs_missing

    def spy(desc, *args, **kw):
        seen["args"], seen["desc"] = args, desc
        return real(desc, *args, **kw)
    monkeypatch.setattr(ops, "filter_forward_wobs_missing", spy)
    with torch.no_grad():
        _, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()
    full = log["filter"]
    q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs_TB, eps, u, idx_in = seen["args"]
    assert idx_in is None and obs_TB.shape[0] == T and bool(torch.isnan(obs_TB[L:, 0]).all())
    d = seen["desc"]
    desc = ops.make_desc(d.B, L, d.N, 1, d.Dx, d.Dy, d.H, resample=bool(d.resample), two_q=bool(d.two_q),
                         bootstrap=bool(d.bootstrap), emission=d.emission, layers=d.layers)
    cut = lambda t: t[:L].contiguous()
    with torch.no_grad():
        short = real(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, cut(mu2), m0, sig0, fm0, fsig0, cut(obs_TB), cut(eps), cut(u))
    torch.cuda.synchronize()
    for key in ("X", "logW", "lse", "Xanc", "idx", "Fm"):
        assert torch.equal(full[key][:L], short[key]), key
    assert torch.isfinite(full["lse"]).all()


@pytest.mark.parametrize("run", [(CASES[1], False), (CASES[3], False), (CASES[5], True)], ids=_id)
def test_two_passes_are_bit_identical(built_lib, run):
    """forward + backward twice in one process, deterministic mode off: the ELBO and every .grad bit for bit"""
    from psvo_amd import ops
    assert not ops.deterministic()
    FLAGS, model, smc, obs, noise, _ = _missing(run, 5)
    nz = Hh.noise_to_hip(noise, "cuda")
    res = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        z.backward()
        torch.cuda.synchronize()
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and torch.isfinite(res[0][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 8
    for n, g in res[0][1].items():
        assert torch.isfinite(g).all() and torch.equal(g, res[1][1][n]), n


def test_step_replays_from_hipgraph(built_lib):
    """one local training step of case 4, eager and captured into a GraphedStep: a replay equals the eager step bit for bit;
    the obs buffer carries the NaNs"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    FLAGS, model, smc, obs, noise, _ = _missing((CASES[3], False), 3)
    nz = Hh.noise_to_hip(noise, "cuda")
    flat = FlatParams(model)
    obs_c = obs.float().cuda()
    assert bool(torch.isnan(obs_c).any())

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


@pytest.mark.parametrize("run", [(CASES[1], False), (CASES[3], True)], ids=_id)
def test_ffbs_and_ffbsi_behind_it(built_lib, run):
    """--FFBS --FFBSi under no_grad behind the missing-observation filter: they read X, Fm and logW only, so everything they
    return is finite and log["Xs"] holds no NaN"""
    FLAGS, model, smc, obs, noise, _ = _missing(run, 3, FFBS=True, FFBSi=True)
    assert smc.FFBS and smc.FFBSi
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(z)
    for key in ("Xs", "Xs_filter", "Xs_marginal", "X_smooth_mean", "ess_smooth", "logW_smooth", "path_logq"):
        assert torch.isfinite(log[key]).all(), key
    assert not bool(torch.isnan(log["Xs"]).any())
    B, T, N, Dx = run[0][1], run[0][2], run[0][3], run[0][5]
    assert log["Xs"].shape == (B, T, N, Dx) and int(log["path_distinct"].min()) >= 1


def _lorenz_with_gaps():
    """the Lorenz slice with 30 % of the entries knocked out and sequence i missing from step 60 + 5 i on"""
    d = np.load(os.path.join(GOLDEN, "lorenz_slice.npz"))
    rng = np.random.RandomState(11)
    out = {}
    for key in ("Ytrain", "Yvalid"):
        y = np.array(d[key], dtype=np.float64)
        y[rng.uniform(size=y.shape) < 0.3] = np.nan
        for i in range(y.shape[0]):
            y[i, 60 + 5 * i:] = np.nan
        out[key] = y
    return out


def test_runner_end_to_end(built_lib, tmp_path, monkeypatch):
    """two epochs on the Lorenz slice with gaps through psvo_amd.runner: finite history and R^2 (asserted by _run_main), the
    missing share of metric_*.p is the data's, every saved y_hat is finite at the missing positions too"""
    data = _lorenz_with_gaps()
    assert data["Ytrain"].shape == (8, 100, 10) and np.isnan(data["Ytrain"][7, 95:]).all()
    FLAGS, hist, work = _run_main(tmp_path, monkeypatch, "gaps", data,
                                  ["--AESMC", "--missing_obs", "--n_particles=32", "--batch_size=4"], 3, 10)
    assert FLAGS.missing_obs and (FLAGS.n_train, FLAGS.n_test, FLAGS.time) == (8, 4, 100)
    metrics = glob.glob(str(work / "rslts" / "**" / "metric_*.p"), recursive=True)
    assert len(metrics) >= 2
    for path in metrics:
        with open(path, "rb") as fh:
            m = pickle.load(fh)
        assert m["missing_share_train"] == pytest.approx(float(np.isnan(data["Ytrain"]).mean()), abs=1e-12)
        assert m["missing_share_test"] == pytest.approx(float(np.isnan(data["Yvalid"]).mean()), abs=1e-12)
        assert 0.3 < m["missing_share_train"] < 0.7
    yh = glob.glob(str(work / "rslts" / "**" / "y_hat_*.p"), recursive=True)
    assert yh, "no y_hat file was written"
    for path in yh:
        with open(path, "rb") as fh:
            for k, a in enumerate(pickle.load(fh)["y_hat"]):
                a = np.asarray(a)
                assert np.isfinite(a).all() and a.shape == (4, 100 - k, 10)
    assert np.isnan(data["Yvalid"][:4]).any()


def test_runner_generates_data_with_gaps(built_lib, tmp_path, monkeypatch):
    """--generateTrainingData --missing_obs --missing_rate=0.3 at Dy = 1, the default FHN data, for two epochs"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    monkeypatch.chdir(tmp_path)
    FLAGS = parse_flags(["--noPSVO", "--AESMC", "--generateTrainingData", "--missing_obs", "--missing_rate=0.3", "--Dy=1", "--Dx=2",
                         "--time=30", "--n_train=8", "--n_test=4", "--batch_size=4", "--n_particles=16", "--epoch=2",
                         "--print_freq=1", "--MSE_steps=5", "--saving_num=4"])
    hist = runner.main(FLAGS)
    torch.cuda.synchronize()
    for key in ("log_ZSMC_trains", "log_ZSMC_tests"):
        assert len(hist[key]) >= 2 and np.isfinite(np.asarray(hist[key], dtype=np.float64)).all(), (key, hist[key])
    for key in ("R_square_trains", "R_square_tests"):
        for r in hist[key]:
            assert np.isfinite(np.asarray(r, dtype=np.float64)).all(), (key, r)
    metrics = glob.glob(str(tmp_path / "rslts" / "**" / "metric_*.p"), recursive=True)
    assert metrics
    with open(metrics[0], "rb") as fh:
        m = pickle.load(fh)
    n, p = 8 * 30, 0.3
    assert abs(m["missing_share_train"] - p) <= 4.0 * (p * (1 - p) / n) ** 0.5


def test_a_nan_without_the_flag_is_a_nan_elbo(built_lib):
    """what the feature is for: on the static wide route one NaN observation turns the ELBO into NaN"""
    case = CASES[2]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=3)
    obs[0, 2, 1] = float("nan")
    with torch.no_grad():
        z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()
    assert torch.isnan(z)
    FLAGS, model, smc, _, noise = _setup(*case, seed=3, missing_obs=True)
    with torch.no_grad():
        z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(z)


@pytest.mark.parametrize("case,extra,word", [
    (("PSVO", 2, 5, 16, 4, 2, 1, 32, True, True), dict(), r"--missing_obs with --PSVO / --PSVOwR"),
    (("PSVOwR", 2, 5, 16, 4, 2, 1, 32, True, True), dict(), r"--missing_obs with --PSVO / --PSVOwR"),
    (("PSVO", 2, 5, 16, 4, 2, 3, 32, True, True), dict(BSim_wide_obs=True), r"--missing_obs with --PSVO / --PSVOwR"),
    (("AESMC", 2, 5, 16, 1, 2, 1, 32, True, True), dict(resample_ess=0.5), r"--missing_obs with --resample_ess"),
    (("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True), dict(particle_forecast=True), r"--missing_obs with --particle_forecast"),
    (("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True), dict(output_cov=True, diag_cov=True), r"--missing_obs with output_cov"),
    (("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True), dict(q1_layers="32,32", g_layers="32,32"), "one hidden layer"),
    (("AESMC", 2, 5, 16, 1, 2, 33, 32, True, True), dict(), r"Dy = 33.*1 <= Dy <= 32"),
    (("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True), dict(missing_rate=1.0), r"--missing_rate = 1\.0.*\[0, 1\)"),
], ids=["PSVO", "PSVOwR", "PSVO-wide", "resample_ess", "particle_forecast", "output_cov", "two-layers", "Dy33", "rate"])
def test_refusals(built_lib, case, extra, word):
    with pytest.raises(ValueError, match=word):
        _setup(*case, missing_obs=True, **extra)
