"""PSVO on missing observations (FLAGS.missing_obs with FLAGS.BSim_missing_obs) on the GPU: psvo_bsim_forward_wobs_missing,
psvo_bsim_backward_wobs_missing (psvo_amd/csrc/bsim_wobs_ms.hip, the second compilation of bsim_wobs.hip) and
psvo_filter_backward_wobs_missing_ext against the fp64 reference of tests/missing_bsim_reference.py.

Shapes are those of tests/test_gpu_wobs_bsim.py at their smallest: T 6, B 2, M 4 and N 64 (one wave of the filter, one full
workgroup of the backward simulation), N 40 (no multiple of 64: partly filled waves) and N 130 (three waves of the filter, three
workgroups per sequence and a padded tile in the backward simulation).  CASES covers Dy in {1, 2, 3, 10, 32}, Dx in {2, 3, 4}
and the three emission forms.  The mask is MR.mask (about 30 % missing, one step with every output missing, one output never
observed at Dy >= 2, a ragged tail on sequence 1); the indices idx_f and sel_b are teacher-forced, so no draw can flip.

Tolerances, quantity by quantity:
  * values, from the forward-kernel checks of tests/test_gpu_wobs_bsim.py: bwX atol 2e-4, flp / glp / Omega atol 5e-4, each with
    rtol 1e-5 (::test_teacher_forced_values); score 2e-3 + 1e-5 of its largest entry (::test_entry_points_alone); the ELBO 1e-4
    relative; the filter's X / logW / lse as there (atol 2e-4 / 5e-4 / 5e-4);
  * gradients, from its reverse-kernel check ::test_every_gradient, which is also the rule of tests/test_gpu_missing.py for the
    filter side: 2e-3 of a tensor's largest entry + 1e-6, with the fp32-reference clause (K32).
Seeds as there: model seed 3 for values, 5 for gradients."""
import glob
import itertools
import pickle

import numpy as np
import pytest
import torch

from tests import count_reference as CR
from tests import helpers as Hh
from tests import missing_bsim_reference as MB
from tests import missing_reference as MR
from tests.test_gpu_instantiations import K32
from tests.test_gpu_parity import _pairs, _setup

pytestmark = pytest.mark.gpu

ON = dict(missing_obs=True, BSim_missing_obs=True)
B, T, M = 2, 6, 4
GAUSS, POISSON, COUNT = "gaussian", "poisson", "count"
EMISSION = {GAUSS: {}, POISSON: dict(poisson_emission=True), COUNT: dict(count_emission=True)}
CASES = [
    # (N, Dx, Dy, H, bootstrap, emission)
    (64, 2, 1, 16, True, GAUSS),            # Dy = 1: the plain weight gradient of MLP_g, one wave
    (40, 3, 2, 32, False, GAUSS),           # Dy = 2, separate f, partly filled waves
    (130, 4, 3, 64, True, GAUSS),           # smallest wide Dy, Dx 4, several waves / workgroups, the 32-unit chunks of bwd_input
    (64, 3, 10, 32, True, POISSON),         # Lorenz widths, unit-normal form
    (40, 2, 32, 32, True, COUNT),           # widest Dy, count form
    (130, 2, 10, 32, False, COUNT),         # count form over several workgroups, separate f
    (40, 4, 1, 16, True, POISSON),          # Dy = 1 again, unit-normal form (no never-observed output at Dy = 1)
    (64, 4, 2, 32, True, COUNT),            # the count form at a width of the plain kernels
    (130, 3, 32, 64, True, GAUSS),          # widest Dy and H over several workgroups
]
_id = lambda c: "-".join(map(str, c))


def _case(case, seed, mask=True, flags=ON, **extra):
    """_setup of the suite under the two flags, the observations knocked out by MR.mask.
    Returns (FLAGS, model, smc, obs (B,T,Dy) fp64 with NaN, noise, t_all, e_never)"""
    N, Dx, Dy, H, boot, em = case[:6]
    FLAGS, model, smc, obs, noise = _setup("PSVO", B, T, N, case[6] if len(case) > 6 else M, Dx, Dy, H, boot, True, seed=seed,
                                           **{**flags, **EMISSION[em], **extra})
    if em == COUNT:
        obs = CR.counts(B, T, Dy, 100 + seed)
    if not mask:
        return FLAGS, model, smc, obs, noise, None, None
    assert smc.missing_obs and smc.wide_obs and smc.uses_backward_simulation
    miss, t_all, e_never = MR.mask(B, T, Dy, seed)
    obs = MR.knock_out(obs, miss)
    assert bool(miss[:, t_all].all()) and (e_never is None) == (Dy == 1) and bool(miss[1, T - 2:].all())
    return FLAGS, model, smc, obs, noise, t_all, e_never


_REF = {}


def _reference(case, seed):
    """the fp64 reference of a (case, seed), computed once: (z_ref, ref log, teacher)"""
    key = (case, seed)
    if key not in _REF:
        FLAGS, model, smc, obs, noise, _, _ = _case(case, seed)
        z_ref, ref = MB.run_oracle(model, FLAGS, obs, noise)
        _REF[key] = (z_ref, ref, MB.teacher(ref))
    return _REF[key]


_err = lambda a, b: float((a - b).abs().max())


def _assert_values(z, log, z_ref, ref):
    filt, bs = log["filter"], log["bsim"]
    score_ref = (ref["f_log_probs"] + ref["g_log_probs"] - ref["bw_log_Omegas"]).sum(0).permute(1, 0)       # (B, N)
    e_score = _err(bs["score"].double().cpu(), score_ref)
    print("max abs err: X %.3e logW %.3e bwX %.3e flp %.3e glp %.3e Omega %.3e score %.3e ELBO rel %.3e (ELBO %.4f)" % (
        _err(Hh.part_to_ref(filt["X"]), ref["X_prevs"]), _err(Hh.w_to_ref(filt["logW"]), ref["log_Ws"]),
        _err(Hh.part_to_ref(bs["bwX"]), ref["bw_Xs"]), _err(Hh.w_to_ref(bs["flp"]), ref["f_log_probs"]),
        _err(Hh.w_to_ref(bs["glp"]), ref["g_log_probs"]), _err(Hh.w_to_ref(bs["Omega"]), ref["bw_log_Omegas"]), e_score,
        abs(float(z) - float(z_ref)) / abs(float(z_ref)), float(z_ref)))
    for v in list(filt.values()) + list(bs.values()) + [log["Xs"], z]:
        assert v is None or not v.is_floating_point() or torch.isfinite(v).all()
    assert torch.allclose(Hh.part_to_ref(filt["X"]), ref["X_prevs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(filt["lse"].double().cpu(), torch.logsumexp(ref["log_Ws"], 1), atol=5e-4, rtol=1e-5)
    assert torch.allclose(Hh.part_to_ref(bs["bwX"]), ref["bw_Xs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(bs["flp"]), ref["f_log_probs"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(bs["glp"]), ref["g_log_probs"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(bs["Omega"]), ref["bw_log_Omegas"], atol=5e-4, rtol=1e-5)
    assert e_score <= 2e-3 + 1e-5 * float(score_ref.abs().max())
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)
    assert abs(float(z_ref)) >= 1.0                   # (the relative tolerance has something to stand on)
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_teacher_forced_values(built_lib, case):
    """score, flp, glp, Omega, bwX, the filter's outputs and the ELBO against fp64; glp == 0 exactly where nothing was observed;
    every output finite although obs holds NaN"""
    FLAGS, model, smc, obs, noise, t_all, _ = _case(case, 3)
    z_ref, ref, teacher = _reference(case, 3)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=MB.hip_noise(noise, teacher))
    torch.cuda.synchronize()
    assert smc._desc().emission == {GAUSS: 0, POISSON: 1, COUNT: 2}[case[5]]
    assert torch.equal(log["missing"].cpu(), torch.isnan(obs)) and log["missing"].dtype == torch.bool
    assert set(log["bsim"]) == {"score", "bwX", "flp", "glp", "Omega", "sel"}
    assert set(log["filter"]) == {"lse", "Fm", "logW", "X", "Xanc", "idx", "eps", "u"}
    assert torch.equal(log["bsim"]["sel"].permute(0, 2, 1).cpu().long(), ref["idx_b"])
    glp = log["bsim"]["glp"]                          # (T, B, N)
    assert bool((glp[t_all] == 0.0).all()) and bool((glp[T - 2:, 1] == 0.0).all())
    assert bool((ref["g_log_probs"][t_all] == 0.0).all())
    _assert_values(z, log, z_ref, ref)


def _compare_gradients(model, FLAGS, obs, noise, teacher, P):
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
        _, P32 = MB.oracle_grads(model, FLAGS, obs, noise, teacher, dtype=torch.float32)
        err32 = {}
        for (name, _, ref), (_, _, ref32) in zip(_pairs(model, P), _pairs(model, P32)):
            r = torch.zeros_like(ref) if ref.grad is None else ref.grad
            r32 = torch.zeros_like(ref) if ref32.grad is None else ref32.grad.double()
            err32[name] = float((r32 - r).abs().max())
        bad = [(n, e, s, err32[n]) for n, e, s in over if e > K32 * err32[n]]
        assert not bad, "gradient mismatch (name, max abs err, own scale, fp32 reference's own err): %s" % bad
    return [n for n, _, _ in rows]


def _gradients_against_the_reference(case, seed=5):
    FLAGS, model, smc, obs, noise, t_all, e_never = _case(case, seed)
    _, _, teacher = _reference(case, seed)
    z_ref, P = MB.oracle_grads(model, FLAGS, obs, noise, teacher)
    model.zero_grad()
    z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=MB.hip_noise(noise, teacher))
    z.backward()
    torch.cuda.synchronize()
    assert abs(float(z.detach()) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    names = _compare_gradients(model, FLAGS, obs, noise, teacher, P)
    for prefix in ("g.", "q1.", "q1_inv.", "BSim_q2.", "BSim_q_init."):          # what the two kernels and the EXT filter feed
        assert any(n.startswith(prefix) for n in names), prefix
    return model, P, e_never


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_gradient(built_lib, case):
    """d log_ZSMC / d(every parameter) against fp64 autograd of the reference; the never-observed output's column of g's output
    layer, its bias and its scale get exactly 0.0 on the GPU; every other output's are there"""
    model, P, e_never = _gradients_against_the_reference(case)
    count, Dy = case[5] == COUNT, case[2]
    others = [e for e in range(Dy) if e != e_never]
    seen = set()
    for name, p, ref in _pairs(model, P):
        if not name.startswith("g.") or name in ("g.W0", "g.b0"):
            continue
        assert p.grad is not None, name
        g = p.grad.detach().cpu()
        seen.add(name)
        if e_never is not None:
            col = g[e_never] if g.dim() == 1 else g[:, e_never]
            rcol = ref.grad[e_never] if g.dim() == 1 else ref.grad[:, e_never]
            assert bool((col == 0.0).all()) and bool((rcol == 0.0).all()), (name, col)
        if name != "g.sigma":       # (a scale held at its floor has no gradient: the comparison above says where)
            cols = g.abs() if g.dim() == 1 else g.abs().amax(0)
            assert bool((cols[others] > 0).all()), (name, cols)
    assert {"g.Wmu", "g.bmu"} <= seen and ("g.sigma" in seen) == (case[5] == GAUSS) and not (count and "g.sigma" in seen)


# ---- all observed: the static wide route ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[2] >= 3], ids=_id)
def test_all_observed_is_the_static_route(built_lib, case):
    """no NaN at Dy >= 3: the same model on psvo_filter_forward_wobs / psvo_bsim_forward_wobs / psvo_bsim_backward_wobs /
    psvo_filter_backward_wobs_ext (FLAGS.BSim_wide_obs).  The count form is bit-identical, values and gradients; the Gaussian
    forms add c_e term by term and stay within the rounding tests/test_gpu_missing.py::test_all_observed_is_the_static_route
    allows (its value tolerances), with identical picks, free-running"""
    count = case[5] == COUNT
    FLAGS, model, smc, obs, noise, _, _ = _case(case, 3, mask=False)
    assert smc.missing_obs and not bool(torch.isnan(obs).any())
    model.missing_obs = False           # (the same weights on the route without the flags)
    plain = type(smc)(model, Hh.make_flags("PSVO", **{**FLAGS.as_dict(), "missing_obs": False, "BSim_missing_obs": False,
                                                      "BSim_wide_obs": True}))
    assert not plain.missing_obs and plain.wide_obs
    nz = Hh.noise_to_hip(noise, "cuda")
    out = []
    for s in (smc, plain):
        model.zero_grad(set_to_none=True)
        z, log = s.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        z.backward()
        torch.cuda.synchronize()
        out.append((z.detach().clone(), log["filter"], log["bsim"],
                    {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    (z_m, f_m, b_m, g_m), (z_p, f_p, b_p, g_p) = out
    print("missing vs static route: logW %.3e glp %.3e Omega %.3e score %.3e" % (
        _err(f_m["logW"], f_p["logW"]), _err(b_m["glp"], b_p["glp"]), _err(b_m["Omega"], b_p["Omega"]),
        _err(b_m["score"], b_p["score"])))
    assert torch.equal(f_m["idx"], f_p["idx"]) and torch.equal(b_m["sel"], b_p["sel"])
    if count:
        assert torch.equal(z_m, z_p)
        for k in ("X", "Xanc", "Fm", "logW", "lse"):
            assert torch.equal(f_m[k].detach(), f_p[k].detach()), k
        for k in ("score", "bwX", "flp", "glp", "Omega"):
            assert torch.equal(b_m[k].detach(), b_p[k].detach()), k
        assert g_m.keys() == g_p.keys() and len(g_m) > 8
        for k in g_m:
            assert torch.equal(g_m[k], g_p[k]), k
        return
    close = lambda a, b, atol: torch.allclose(a.detach(), b.detach(), atol=atol, rtol=1e-5)
    assert close(f_m["X"], f_p["X"], 2e-4) and close(f_m["logW"], f_p["logW"], 5e-4) and close(f_m["lse"], f_p["lse"], 5e-4)
    assert close(b_m["bwX"], b_p["bwX"], 2e-4)
    for k in ("flp", "glp", "Omega"):
        assert close(b_m[k], b_p[k], 5e-4), k
    assert abs(float(z_m) - float(z_p)) <= 1e-4 * abs(float(z_p))


# ---- reproducibility ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[1], CASES[5], CASES[8]], ids=_id)
def test_two_passes_are_bit_identical(built_lib, case):
    """forward + backward twice in one process, deterministic mode off: the ELBO and every .grad bit for bit"""
    from psvo_amd import ops
    assert not ops.deterministic()
    FLAGS, model, smc, obs, noise, _, _ = _case(case, 5)
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


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=_id)
def test_step_replays_from_hipgraph(built_lib, case):
    """one local training step, eager and captured into a GraphedStep: a replay equals the eager step bit for bit; the obs
    buffer carries the NaNs"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    FLAGS, model, smc, obs, noise, _, _ = _case(case, 3)
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


# ---- every instantiation once -----------------------------------------------------------------------------------------------------
# (Dx, H, M, CNT) of bsim_wobs_fwd_kernel / bsim_wobs_bwd_kernel in their missing form: 72 each; the 18 (Dx, H, CNT) forms of
# filter_bwd_wobs_ms_kernel<.., EXT = true> run behind them (every one four times).  One tiny problem each, N 12 / 20 / 36 as in
# tests/test_gpu_instantiations.py, the wirings and the widths alternating over the sweep; values and every gradient against
# the reference.
EVERY = list(itertools.product((2, 3, 4), (16, 32, 64), (4, 8, 16, 32), (False, True)))


@pytest.mark.parametrize("k,combo", list(enumerate(EVERY)), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_every_instantiation(built_lib, k, combo):
    Dx, H, Mk, cnt = combo
    case = ((20, 36, 12)[k % 3], Dx, (1, 2, 3, 10, 32)[k % 5], H, k % 3 != 1, COUNT if cnt else (GAUSS, POISSON)[k % 2], Mk)
    FLAGS, model, smc, obs, noise, t_all, _ = _case(case, 5)
    z_ref, ref, teacher = _reference(case, 5)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=MB.hip_noise(noise, teacher))
    torch.cuda.synchronize()
    d = smc._desc(Mk)
    assert (d.Dx, d.H, d.M, d.emission == 2) == combo
    assert bool((log["bsim"]["glp"][t_all] == 0.0).all())
    _assert_values(z, log, z_ref, ref)
    _gradients_against_the_reference(case)
    _REF.pop((case, 5), None)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dy,extra", [(1, []), (10, ["--count_emission"]),
                                      (1, ["--particle_forecast", "--particle_forecast_missing_obs"]),
                                      (10, ["--count_emission", "--particle_forecast", "--particle_forecast_missing_obs"])],
                         ids=["Dy1", "Dy10", "Dy1-forecast", "Dy10-forecast"])
def test_runner_generates_data_with_gaps(built_lib, tmp_path, monkeypatch, Dy, extra):
    """--PSVO --missing_obs --BSim_missing_obs --generateTrainingData --missing_rate=0.3 for two epochs: finite history, the
    missing share written; with the particle forecast on gappy data behind it.  (The generated data set is the FHN model's: one
    Gaussian output, or counts through data_generator.count_loading at any width -- so Dy = 10 is generated as counts.)"""
    from psvo_amd import runner
    from psvo_amd.flags import parse_flags
    monkeypatch.chdir(tmp_path)
    FLAGS = parse_flags(["--PSVO", "--missing_obs", "--BSim_missing_obs", "--generateTrainingData", "--missing_rate=0.3",
                         "--Dy=%d" % Dy, "--Dx=2", "--time=20", "--n_train=8", "--n_test=4", "--batch_size=4", "--n_particles=16",
                         "--n_particles_for_BSim_proposal=4", "--epoch=2", "--print_freq=1", "--MSE_steps=3", "--saving_num=4"]
                        + extra)
    hist = runner.main(FLAGS)
    torch.cuda.synchronize()
    for key in ("log_ZSMC_trains", "log_ZSMC_tests"):
        assert len(hist[key]) >= 2 and np.isfinite(np.asarray(hist[key], dtype=np.float64)).all(), (key, hist[key])
    metrics = glob.glob(str(tmp_path / "rslts" / "**" / "metric_*.p"), recursive=True)
    assert metrics
    with open(metrics[0], "rb") as fh:
        m = pickle.load(fh)
    n, p = 8 * 20 * Dy, 0.3
    assert abs(m["missing_share_train"] - p) <= 4.0 * (p * (1 - p) / n) ** 0.5 and 0.0 < m["missing_share_test"] < 1.0
    if "--particle_forecast" in extra:
        assert np.isfinite(np.asarray(m["forecast_lpd_per_entry_test"], dtype=np.float64)).any()


# ---- what stays refused -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj,extra,word", [
    ("PSVO", dict(missing_obs=True), r"--missing_obs with --PSVO / --PSVOwR"),
    ("PSVOwR", ON, r"--BSim_missing_obs with --PSVOwR"),
    ("PSVO", dict(ON, output_cov=True, diag_cov=True), r"--missing_obs with output_cov"),
    ("PSVO", dict(ON, q1_layers="32,32", g_layers="32,32"), "one hidden layer"),
    ("PSVO", dict(ON, resample_ess=0.5), r"--resample_ess.*PSVO"),
], ids=["unflagged", "PSVOwR", "output_cov", "two-layers", "resample_ess"])
def test_refusals(built_lib, obj, extra, word):
    with pytest.raises(ValueError, match=word):
        _setup(obj, 2, 5, 16, 4, 2, 3, 32, True, True, **extra)
