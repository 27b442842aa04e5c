"""Count emission (FLAGS.count_emission, psvo_desc.emission = 2) on the GPU: the count forms of the wide-observation kernels
(psvo_amd/csrc/filter_wobs.hip, bsim_wobs.hip) against the fp64 reference of tests/count_reference.py.

Cases are the smallest shapes at which these kernels can go wrong (see CASES).  Observations are counts
torch.poisson(4 U[0, 1)), seeded; they contain zeros.  Tolerances are the suite's own: values as
tests/test_gpu_wobs_bsim.py::test_teacher_forced_values, the ELBO 1e-4 relative, draws as ::test_free_running_draws, gradients
2e-3 of a tensor's largest entry + 1e-6 with the fp32-reference clause (K32) of ::test_every_gradient.  Seeds as there: model
seed 3 for values and draws, 5 for gradients.

What backs the tolerances: the fp32 reference on the CPU against its own fp64 values, on these nine cases with these seeds and
the tests' own models (tools/count_reference_error.py prints the table), stays at or below
    X 1.7e-05, logW 3.7e-04 (where |logW| reaches 910: case 3, whose weights accumulate without resampling), lse 1.7e-04,
    bwX 6.3e-06, flp 9.3e-05, glp 4.7e-05, Omega 2.6e-05, ELBO 1.9e-07 relative,
    0.15 of the allclose bound atol + rtol |reference| over every compared element (case 3; 0.071 on every other case),
    gradients 4.9e-04 of a tensor's largest entry (case 7; the bound is 2e-3),
each at or below a third of its tolerance, so a failure here is the kernel's, not the model's."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch

from tests import count_reference as CR
from tests import helpers as Hh
from tests.test_gpu_instantiations import K32
from tests.test_gpu_large import EDGE_TOL
from tests.test_gpu_parity import _pairs, _setup
from tests.test_gpu_wobs import _run_main

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

CASES = [
    # (objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q)
    ("AESMC", 2, 5, 16, 1, 2, 3, 16, True, True),          # smallest Dy and H, one wave
    ("SVO", 2, 6, 40, 1, 3, 10, 32, False, True),          # Lorenz widths, separate f, partly filled wave
    ("IWAE", 2, 5, 24, 1, 4, 17, 64, True, False),         # no resampling, no q2, odd Dy, the 32-unit chunks of bwd_input
    ("AESMC", 1, 4, 512, 1, 4, 32, 32, False, True),       # the 512-lane kernels at every limit
    ("SVO", 1, 60, 32, 1, 3, 10, 32, True, True),          # long recurrence, both halves of the row buffer many times
    ("PSVO", 2, 5, 16, 4, 2, 3, 16, True, True),           # smallest wide Dy with a backward simulation
    ("PSVO", 2, 6, 40, 8, 3, 10, 32, False, True),         # Lorenz widths, separate f, N no multiple of the chains per workgroup
    ("PSVO", 1, 5, 24, 32, 3, 32, 64, True, True),         # widest Dy, H and M
    ("PSVO", 2, 5, 130, 4, 4, 17, 64, False, True),        # several workgroups per sequence, the AGPR-heavy Dx = 4 form
]
_id = lambda c: "-".join(map(str, c))


def count_flags(obj, **extra):
    kw = dict(count_emission=True)
    if obj == "PSVO":
        kw["BSim_wide_obs"] = True
    kw.update(extra)
    return kw


def _count(case, seed, **extra):
    """_setup of the suite under --count_emission, its Gaussian observations replaced by seeded counts"""
    obj, B, T, Dy = case[0], case[1], case[2], case[6]
    FLAGS, model, smc, _, noise = _setup(*case, seed=seed, **count_flags(obj, **extra))
    if not extra:
        assert smc.wide_obs and FLAGS.count_emission
    return FLAGS, model, smc, CR.counts(B, T, Dy, 100 + seed), noise


def _teacher(obj, ref):
    t = {"idx_f": ref["idx_f"]} if ref["idx_f"] is not None else {}
    if obj == "PSVO":
        t["idx_b"] = ref["idx_b"]
    return t


def _hip_noise(noise, teacher):
    nz = Hh.noise_to_hip({**noise, **teacher}, "cuda")
    if "idx_f" in nz:
        nz.pop("u_f", None)
    if "sel_b" in nz:
        nz.pop("u_b", None)
    return nz


_err = lambda a, b: float((a - b).abs().max())


def _assert_values(obj, z, log, z_ref, ref):
    filt = log["filter"]
    lse_ref = torch.logsumexp(ref["log_Ws"], 1)
    line = "max abs err: X %.3e logW %.3e lse %.3e" % (_err(Hh.part_to_ref(filt["X"]), ref["X_prevs"]),
                                                       _err(Hh.w_to_ref(filt["logW"]), ref["log_Ws"]),
                                                       _err(filt["lse"].double().cpu(), lse_ref))
    if obj == "PSVO":
        bs = log["bsim"]
        line += " bwX %.3e flp %.3e glp %.3e Omega %.3e" % (
            _err(Hh.part_to_ref(bs["bwX"]), ref["bw_Xs"]), _err(Hh.w_to_ref(bs["flp"]), ref["f_log_probs"]),
            _err(Hh.w_to_ref(bs["glp"]), ref["g_log_probs"]), _err(Hh.w_to_ref(bs["Omega"]), ref["bw_log_Omegas"]))
    print(line + " ELBO rel %.3e" % (abs(float(z) - float(z_ref)) / abs(float(z_ref))))
    assert torch.allclose(Hh.part_to_ref(filt["X"]), ref["X_prevs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.part_to_ref(filt["Xanc"]), ref["X_ancestors"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(filt["lse"].double().cpu(), lse_ref, atol=5e-4, rtol=1e-5)
    if obj == "PSVO":
        assert torch.allclose(Hh.part_to_ref(bs["bwX"]), ref["bw_Xs"], atol=2e-4, rtol=1e-5)
        assert torch.allclose(Hh.w_to_ref(bs["flp"]), ref["f_log_probs"], atol=5e-4, rtol=1e-5)
        assert torch.allclose(Hh.w_to_ref(bs["glp"]), ref["g_log_probs"], atol=5e-4, rtol=1e-5)
        assert torch.allclose(Hh.w_to_ref(bs["Omega"]), ref["bw_log_Omegas"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_teacher_forced_values(built_lib, case):
    """X, Xanc, logW, lse -- for PSVO also bwX, flp, glp, Omega -- Xs and the ELBO against fp64; indices teacher-forced"""
    obj = case[0]
    FLAGS, model, smc, obs, noise = _count(case, 3)
    assert float(obs.min()) == 0.0 and bool((obs == obs.floor()).all())
    z_ref, ref = CR.run_oracle(model, FLAGS, obj, obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, _teacher(obj, ref)))
    torch.cuda.synchronize()
    assert smc._desc(case[4]).emission == 2
    _assert_values(obj, z, log, z_ref, ref)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_free_running_draws(built_lib, case):
    """in-kernel draws of the filter and of the sub-particle pick against the reference's definition: no index differs"""
    obj = case[0]
    FLAGS, model, smc, obs, noise = _count(case, 3)
    z_ref, ref = CR.run_oracle(model, FLAGS, obj, obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()
    differ = 0
    if ref["idx_f"] is not None:
        differ += int((log["filter"]["idx"].permute(0, 2, 1).cpu().long() != ref["idx_f"]).sum())
    if obj == "PSVO":
        differ += int((log["bsim"]["sel"].permute(0, 2, 1).cpu().long() != ref["idx_b"]).sum())
    if differ:
        _, _, st = CR.replay_with_hip_indices(model, FLAGS, obj, obs, noise, log)
        print("draws=%d differing=%d flipped=%d worst edge distance=%.3e" % (st["draws"], differ, st["off"], st["worst"]))
        assert st["worst"] <= EDGE_TOL, "a draw that is not on a CDF edge: %s" % st
    assert differ == 0, "%d draws differ from the reference's (edge flips: see the printed distances)" % differ
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    assert torch.allclose(log["Xs"].double().cpu(), ref["Xs"], atol=2e-4, rtol=1e-5)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_gradient(built_lib, case):
    """d log_ZSMC / d(every parameter), teacher-forced indices, against fp64 autograd of the reference"""
    obj = case[0]
    FLAGS, model, smc, obs, noise = _count(case, 5)
    _, ref0 = CR.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = _teacher(obj, ref0)
    z_ref, P = CR.oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    model.zero_grad()
    z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, teacher))
    z.backward()
    torch.cuda.synchronize()
    assert abs(float(z.detach()) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    rows = []
    for name, p, ref in _pairs(model, P):
        g = torch.zeros_like(ref) if p.grad is None else p.grad.detach().double().cpu()
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        rows.append((name, float((g - r).abs().max()), max(float(r.abs().max()), 1e-6)))
    names = [n for n, _, _ in rows]
    assert {"g.W0", "g.b0", "g.Wmu", "g.bmu"} <= set(names) and "g.sigma" not in names
    for name, p, ref in _pairs(model, P):
        if name.startswith("g."):       # the emission network is trained by the count likelihood: its gradient is there
            assert p.grad is not None and float(p.grad.abs().max()) > 0 and float(ref.grad.abs().max()) > 0, name
    worst = max(rows, key=lambda r: r[1] / r[2])
    print("worst gradient error / largest entry: %s %.3e" % (worst[0], worst[1] / worst[2]))
    over = [r for r in rows if r[1] > 2e-3 * r[2] + 1e-6]
    if over:        # the second clause: the fp32 reference's own error on the same tensor (computed only when it is needed)
        _, P32 = CR.oracle_grads(model, FLAGS, obj, obs, noise, teacher, dtype=torch.float32)
        err32 = {}
        for (name, _, ref), (_, _, ref32) in zip(_pairs(model, P), _pairs(model, P32)):
            r = torch.zeros_like(ref) if ref.grad is None else ref.grad
            r32 = torch.zeros_like(ref) if ref32.grad is None else ref32.grad.double()
            err32[name] = float((r32 - r).abs().max())
        bad = [(n, e, s, err32[n]) for n, e, s in over if e > K32 * err32[n]]
        assert not bad, "gradient mismatch (name, max abs err, own scale, fp32 reference's own err): %s" % bad


LARGE = (0, 1, 2, 3, 7, 8, 9, 20, 50, 200, 1000, 10000)


def test_large_counts(built_lib):
    """case 2's shape with the observation rows overwritten by LARGE cycled over the outputs: logW and lse under the same
    allclose rule.  The log-factorial reaches 8.2e4 there; the printed error is the record of its accuracy in the sums."""
    case = CASES[1]
    obj = case[0]
    FLAGS, model, smc, obs, noise = _count(case, 3)
    Dy = case[6]
    obs = torch.tensor([LARGE[(e + r) % len(LARGE)] for r in range(obs.shape[0] * obs.shape[1]) for e in range(Dy)],
                       dtype=torch.float64).reshape(obs.shape)
    assert set(obs.flatten().tolist()) == set(float(v) for v in LARGE)
    z_ref, ref = CR.run_oracle(model, FLAGS, obj, obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, _teacher(obj, ref)))
    torch.cuda.synchronize()
    filt = log["filter"]
    lse_ref = torch.logsumexp(ref["log_Ws"], 1)
    print("large counts: max abs err logW %.3e (largest |logW| %.3e) lse %.3e" % (
        _err(Hh.w_to_ref(filt["logW"]), ref["log_Ws"]), float(ref["log_Ws"].abs().max()), _err(filt["lse"].double().cpu(), lse_ref)))
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(filt["lse"].double().cpu(), lse_ref, atol=5e-4, rtol=1e-5)


def test_emission_1_is_still_the_unit_normal(built_lib):
    """--poisson_emission and --count_emission on the same integer observations: different ELBOs, each its own reference's"""
    case = CASES[0]
    obj = case[0]
    got = {}
    for flag in ("poisson_emission", "count_emission"):
        FLAGS, model, smc, _, noise = _setup(*case, seed=3, **{flag: True})
        obs = CR.counts(case[1], case[2], case[6], 103)
        run = Hh.run_oracle if flag == "poisson_emission" else CR.run_oracle
        z_ref, ref = run(model, FLAGS, obj, obs, noise)
        with torch.no_grad():
            z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, _teacher(obj, ref)))
        torch.cuda.synchronize()
        assert smc._desc().emission == (1 if flag == "poisson_emission" else 2)
        assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref)), flag
        assert torch.allclose(Hh.w_to_ref(log["filter"]["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5), flag
        got[flag] = (float(z), float(z_ref))
    print("ELBO: unit normal %.6f, count %.6f" % (got["poisson_emission"][0], got["count_emission"][0]))
    assert abs(got["poisson_emission"][1] - got["count_emission"][1]) > 1e-2 * abs(got["count_emission"][1])
    assert abs(got["poisson_emission"][0] - got["count_emission"][0]) > 1e-2 * abs(got["count_emission"][0])


@pytest.mark.parametrize("case", [CASES[1], CASES[8]], ids=_id)
def test_two_passes_are_bit_identical(built_lib, case):
    """forward + backward twice in one process, deterministic mode off: the ELBO and every .grad bit for bit"""
    from psvo_amd import ops
    assert not ops.deterministic()
    FLAGS, model, smc, obs, noise = _count(case, 5)
    nz = Hh.noise_to_hip(noise, "cuda")
    res = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        z.backward()
        torch.cuda.synchronize()
        res.append((z.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 8
    for n, g in res[0][1].items():
        assert torch.isfinite(g).all() and torch.equal(g, res[1][1][n]), n


def test_step_replays_from_hipgraph(built_lib):
    """one local training step of case 7, eager and captured into a GraphedStep: a replay equals the eager step bit for bit"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    FLAGS, model, smc, obs, noise = _count(CASES[6], 3)
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


def _lorenz_counts():
    """counts drawn from the latent states of the Lorenz slice: Dy = 10, rate softplus(C x / 10 + 1) with the runner's loading
    (psvo_amd.utils.data_generator.count_loading) extended by a third column of alternating signs"""
    from psvo_amd.utils.data_generator import count_loading
    d = np.load(os.path.join(GOLDEN, "lorenz_slice.npz"))
    C, off = count_loading(10, 3)
    C[:, 2] = np.where(np.arange(10) % 2 == 0, 1.0, -1.0)
    rng = np.random.RandomState(7)
    draw = lambda X: rng.poisson(np.logaddexp(0.0, X @ C.T / 10.0 + off)).astype(np.float64)
    return {"Ytrain": draw(d["State_train"]), "Yvalid": draw(d["State_valid"])}


@pytest.mark.parametrize("argv,N", [
    (["--AESMC", "--count_emission", "--FFBSi", "--n_particles=32", "--batch_size=4"], 32),
    (["--PSVO", "--BSim_wide_obs", "--count_emission", "--n_particles=16", "--n_particles_for_BSim_proposal=4",
      "--batch_size=4"], 16),
], ids=["AESMC-FFBSi", "PSVO"])
def test_runner_end_to_end(built_lib, tmp_path, monkeypatch, argv, N):
    """two epochs on count data through psvo_amd.runner: finite history and R^2 (asserted by _run_main), every saved y_hat a
    rate (strictly positive), trajectories of shape (100, N, 3)"""
    data = _lorenz_counts()
    assert data["Ytrain"].min() == 0 and data["Ytrain"].shape == (8, 100, 10)
    FLAGS, hist, work = _run_main(tmp_path, monkeypatch, "counts", data, argv, 3, 10)
    assert FLAGS.count_emission and (FLAGS.n_train, FLAGS.n_test, FLAGS.time) == (8, 4, 100)
    yh = glob.glob(str(work / "rslts" / "**" / "y_hat_*.p"), recursive=True)
    assert yh, "no y_hat file was written"
    for path in yh:
        with open(path, "rb") as fh:
            for a in pickle.load(fh)["y_hat"]:
                a = np.asarray(a)
                assert np.isfinite(a).all() and (a > 0).all() and a.shape[-1] == 10
    tr = glob.glob(str(work / "rslts" / "**" / "trajectory_*.p"), recursive=True)
    assert tr, "no trajectory file was written"
    for path in tr:
        with open(path, "rb") as fh:
            assert np.asarray(pickle.load(fh)["Xs"]).shape[-3:] == (100, N, 3)


@pytest.mark.parametrize("case,extra,word", [
    (("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True), dict(count_emission=True, poisson_emission=True),
     r"--count_emission with --poisson_emission"),
    (("AESMC", 2, 5, 16, 1, 2, 2, 32, True, True), dict(count_emission=True), r"3 <= Dy <= 32.*plain kernels.*no count form"),
    (("PSVO", 2, 5, 16, 4, 2, 1, 32, True, True), dict(count_emission=True, BSim_wide_obs=True),
     r"3 <= Dy <= 32.*plain kernels.*no count form"),
    (("PSVO", 2, 5, 16, 4, 2, 3, 32, True, True), dict(count_emission=True), r"Dy = 3 with PSVO / PSVOwR.*Dy <= 2"),
    (("PSVOwR", 2, 5, 16, 4, 2, 3, 32, True, True), dict(count_emission=True, BSim_wide_obs=True), "PSVOwR"),
    (("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True), dict(count_emission=True, output_cov=True, diag_cov=True), "output_cov"),
    (("AESMC", 2, 5, 16, 1, 2, 3, 32, True, True), dict(count_emission=True, q1_layers="32,32", g_layers="32,32"),
     "one hidden layer"),
    (("AESMC", 2, 5, 16, 1, 2, 33, 32, True, True), dict(count_emission=True), r"Dy = 33.*3 <= Dy <= 32"),
], ids=["both-flags", "Dy2", "Dy1-PSVO", "PSVO-no-flag", "PSVOwR", "output_cov", "two-layers", "Dy33"])
def test_refusals(built_lib, case, extra, word):
    with pytest.raises(ValueError, match=word):
        _setup(*case, **extra)
