"""The step of the four-lanes-per-particle forward filter (N <= 128) with the lanes' MLP weight slices held in registers: read
from LDS once in front of the time loop (MlpLds::Slice) instead of in every step.  Which slices are registers is decided per
instantiation (filter_fwd_impl.h: kRegGQ, kRegF); the others, and the two-layer MLPs, read LDS as before.

The shapes are the smallest at which a step of this kernel can go wrong -- a slice loaded for the wrong lane or MLP, a value read
before the barrier that publishes it, a staged array overwritten while a slower wave still reads it:
  T = 1 .. 5        the peeled step alone, the first ordinary one, and a few more behind it
  N = 3             a partial quad row;  16: one wave, one block;  17: two waves, the second nearly empty (its maximum is -inf
                    unless its one particle wins);  33, 113: a partial last block, idx clamped to N - 1;  64;  128: all eight waves
  wirings           every one that adds or drops a staged array, a weight slice, a barrier path or a kernel build
  T = 64, N = 128   a longer chain: a stale word shows up as an index far from any CDF edge
  twice             the same inputs again, byte for byte

Method and tolerances are those of tests/test_gpu_filter_inputs.py (whose helpers run the cases): values against the fp64 oracle
re-run with the kernel's indices, every index the oracle's own draw or within EDGE_TOL of a CDF edge, gradients to 2e-3 of a
tensor's largest entry; the adaptive cases as tests/test_gpu_adaptive.py.  PSVO_TUNE_FILTER_BWD = 0 throughout, so the reverse
pass is the persistent quad kernel reading what this kernel wrote."""
import pytest
import torch

from psvo_amd import _lib
from tests import adaptive_reference as AR
from tests import helpers as Hh
from tests.test_gpu_adaptive import MARGIN, _hip
from tests.test_gpu_filter_inputs import _TWO, _free_run_against_oracle, _id, _pass, _teacher_forced
from tests.test_gpu_large import EDGE_TOL, _compare
from tests.test_gpu_parity import _pairs, _setup

pytestmark = pytest.mark.gpu

# objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q
PARITY = [(("AESMC", 2, t, 33, 1, 2, 1, 32, True, True), {}) for t in (1, 2, 3, 4, 5)]
WAVES = [(("AESMC", 2, t, n, 1, 2, 1, 32, True, True), {}) for n in (3, 16, 17, 33, 64, 113, 128) for t in (2, 5)]
WIRINGS = [w for n in (17, 128) for w in [
    (("AESMC", 2, 5, n, 1, 2, 1, 32, False, True), {}),          # non-bootstrap: the staged sf array and MLP_f's slice
    (("AESMC", 2, 5, n, 1, 2, 1, 32, True, False), {}),          # without mu2
    (("AESMC", 2, 5, n, 1, 2, 1, 32, False, False), {}),
    (("IWAE", 2, 5, n, 1, 2, 1, 32, True, True), {}),            # resampling off: the other path behind the barrier
    (("IWAE", 2, 5, n, 1, 3, 2, 32, False, True), {}),
    (("AESMC", 2, 5, n, 1, 2, 1, 32, True, True), _TWO),         # two hidden layers: the weights stay in LDS
    (("AESMC", 2, 5, n, 1, 3, 2, 32, False, True), _TWO),
    (("AESMC", 2, 5, n, 1, 2, 2, 32, True, True), {}),           # Dx in {2, 3} x Dy in {1, 2}
    (("AESMC", 2, 5, n, 1, 3, 1, 32, True, True), {}),
    (("AESMC", 2, 5, n, 1, 3, 2, 32, False, True), {}),          # (MLP_f's slice read from LDS: the three do not fit)
    (("AESMC", 2, 5, n, 1, 4, 1, 16, True, True), {}),           # the H = 16, Dx = 4 one-layer build
    (("AESMC", 2, 5, n, 1, 4, 2, 16, False, True), {}),
]]
OBJECTIVES = [(("PSVO", 4, 12, 32, 8, 2, 1, 32, True, True), {}),          # the `tiny` sizes: the backward simulation consumes the outputs
              (("PSVO", 2, 5, 17, 4, 2, 1, 32, False, True), {})]
TEACHER = [(("AESMC", 2, 5, n, 1, 2, 1, 32, True, True), {}) for n in (17, 128)]


@pytest.mark.parametrize("case,extra", PARITY, ids=map(_id, PARITY))
def test_step_buffer_parity(built_lib, case, extra):
    _free_run_against_oracle(case, extra, seed=41)


@pytest.mark.parametrize("case,extra", WAVES, ids=map(_id, WAVES))
def test_step_waves_and_blocks(built_lib, case, extra):
    _free_run_against_oracle(case, extra, seed=43)


@pytest.mark.parametrize("case,extra", WIRINGS, ids=map(_id, WIRINGS))
def test_step_wirings(built_lib, case, extra):
    _free_run_against_oracle(case, extra, seed=45)


@pytest.mark.parametrize("case,extra", OBJECTIVES, ids=map(_id, OBJECTIVES))
def test_step_objectives(built_lib, case, extra):
    _free_run_against_oracle(case, extra, seed=47)


@pytest.mark.parametrize("case,extra", TEACHER, ids=map(_id, TEACHER))
def test_step_teacher_forced(built_lib, case, extra):
    """idx_in: no search, the gather alone reads the staged arrays"""
    with Hh.tuning(_lib.PSVO_TUNE_FILTER_BWD, 0):
        _teacher_forced(case, extra)


def test_step_long_chain(built_lib):
    """AESMC, B = 4, T = 64, N = 128: every index the oracle's draw or within EDGE_TOL of a CDF edge, every value in tolerance"""
    case = ("AESMC", 4, 64, 128, 1, 2, 1, 32, True, True)
    FLAGS, model, smc, obs, noise = _setup(*case, seed=49)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()
    z_ref, ref, st = Hh.replay_with_hip_indices(model, FLAGS, case[0], obs, noise, log)
    print("draws=%d flipped=%d worst edge distance=%.3e" % (st["draws"], st["off"], st["worst"]))
    assert st["draws"] >= 63 * 4 * 128
    assert st["worst"] <= EDGE_TOL, st
    _compare(case[0], log, ref, z, z_ref)
    assert torch.allclose(log["filter"]["lse"].double().cpu(), torch.logsumexp(ref["log_Ws"], 1), atol=5e-4, rtol=1e-5)


# ---- the adaptive build: the draw made every step and inherited at some --------------------------------------------------------
# (objective, B, T, N, Dx, Dy, hidden layers, bootstrap, two_q, further flags, model seed) as tests/adaptive_reference.CASES;
# flags, seeds and the threshold (TAU unless resample_ess says otherwise) chosen with the fp64 reference on the CPU so that, free
# running, it resamples at some steps and keeps at others, with no step's ESS / N within 0.005 of the threshold (at N = 128 this
# model's ESS / N stays below 0.5 at every step)
ADAPTIVE = [("AESMC", 2, 5, 17, 2, 1, "32", True, True, {}, 3),
            ("AESMC", 2, 5, 128, 2, 1, "32", True, True, dict(calm=0.5, resample_ess=0.2), 3),
            ("AESMC", 2, 5, 17, 2, 1, "32", False, True, {}, 3)]


def _adaptive_grads_ok(model, FLAGS, case, obs, noise, log, z):
    z_ref, P = AR.oracle_grads(model, FLAGS, case[0], obs, noise, AR.hip_teacher(log))
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    rows = []
    for name, p, ref in _pairs(model, P):
        g = torch.zeros_like(ref) if p.grad is None else p.grad.double().cpu()
        want = torch.zeros_like(ref) if ref.grad is None else ref.grad
        rows.append((name, float((g - want).abs().max()), max(float(want.abs().max()), 1e-6)))
    bad = [v for v in rows if v[1] > 2e-3 * v[2] + 1e-6]
    assert len(rows) > 8 and not bad, "gradient mismatch (name, max abs err, largest entry): %s" % bad


def _adaptive_values_ok(case, log, ref, z, z_ref):
    N, filt = case[3], log["filter"]
    assert abs(float(z) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    assert torch.allclose(Hh.part_to_ref(filt["X"]), ref["X_prevs"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.part_to_ref(filt["Xanc"]), ref["X_ancestors"], atol=2e-4, rtol=1e-5)
    assert torch.allclose(Hh.w_to_ref(filt["logW"]), ref["log_Ws"], atol=5e-4, rtol=1e-5)
    assert torch.allclose(filt["lse"].double().cpu(), torch.logsumexp(ref["log_Ws"], 1), atol=5e-4, rtol=1e-5)
    assert float(((filt["ess"].double().cpu() - ref["ess"]).abs() / N).max()) <= MARGIN


@pytest.mark.parametrize("case", ADAPTIVE, ids=AR.case_id)
def test_step_adaptive_threshold(built_lib, case):
    """free running at the case's threshold: some steps resample and some keep; values, decisions and every gradient as tests/test_gpu_adaptive.py"""
    T, B, N = case[2], case[1], case[3]
    FLAGS, model, smc, obs, noise = AR.setup(case, "cuda")
    with Hh.tuning(_lib.PSVO_TUNE_FILTER_BWD, 0):
        model.zero_grad(set_to_none=True)
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise))
        z.backward()
        torch.cuda.synchronize()
    rs = log["filter"]["rs"].cpu() != 0
    assert 0 < int(rs.sum()) < T * B, rs
    z_ref, ref = AR.replay_with_hip(model, FLAGS, case[0], obs, noise, log)
    _adaptive_values_ok(case, log, ref, z.detach(), z_ref)
    tau = float(FLAGS.resample_ess)
    differ = AR.decide(ref["ess"], tau, N) != rs
    assert not bool((differ & ~((ref["ess"] / N - tau).abs() <= MARGIN)).any()), differ.nonzero().tolist()
    _adaptive_grads_ok(model, FLAGS, case, obs, noise, log, z.detach())


@pytest.mark.parametrize("case", ADAPTIVE[:2], ids=AR.case_id)
def test_step_adaptive_alternating(built_lib, case):
    """forced decisions 0 / 1 in turn (and in turn over the sequences): honoured exactly, values and gradients on those decisions"""
    T, B = case[2], case[1]
    FLAGS, model, smc, obs, noise = AR.setup(case, "cuda")
    forced = torch.tensor([[(t + b) & 1 for b in range(B)] for t in range(T)], dtype=torch.int32)
    with Hh.tuning(_lib.PSVO_TUNE_FILTER_BWD, 0):
        model.zero_grad(set_to_none=True)
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip(noise, {"rs_f": forced}))
        z.backward()
        torch.cuda.synchronize()
    assert torch.equal(log["filter"]["rs"].cpu(), forced)
    z_ref, ref = AR.replay_with_hip(model, FLAGS, case[0], obs, noise, log)
    _adaptive_values_ok(case, log, ref, z.detach(), z_ref)
    _adaptive_grads_ok(model, FLAGS, case, obs, noise, log, z.detach())


# ---- the same inputs twice ------------------------------------------------------------------------------------------------------
REPEAT = [(("PSVO", 4, 12, 32, 8, 2, 1, 32, True, True), {}), (("AESMC", 2, 5, 128, 1, 2, 1, 32, False, True), {}),
          (("AESMC", 4, 64, 128, 1, 2, 1, 32, True, True), {})]


@pytest.mark.parametrize("case,extra", REPEAT, ids=map(_id, REPEAT))
def test_step_repeatable(built_lib, case, extra):
    """every output and every gradient byte-equal (a word read before the barrier that publishes it, or a staged array overwritten while
    a slower wave still reads it, does not repeat).  PSVO_TUNE_DETERMINISTIC = 1: the reverse sums in a fixed order, so that a
    difference can only come from the forward pass."""
    FLAGS, model, smc, obs, noise = _setup(*case, seed=51, **extra)
    nz = Hh.noise_to_hip(noise, "cuda")
    runs = []
    for _ in range(2):
        with Hh.tuning(_lib.PSVO_TUNE_FILTER_BWD, 0), Hh.tuning(_lib.PSVO_TUNE_DETERMINISTIC, 1):
            z, log = _pass(model, smc, obs, nz)
        out = {"z": z.cpu().clone(), "Xs": log["Xs"].detach().cpu().clone()}
        for part, keys in (("filter", ("X", "Xanc", "Fm", "logW", "idx", "lse")), ("bsim", ("bwX", "flp", "glp", "Omega", "sel"))):
            out.update({part + "." + k: log[part][k].detach().cpu().clone() for k in keys if part in log})
        out.update({"grad." + n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None})
        runs.append(out)
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) > 8
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8)
    diff = [k for k in runs[0] if runs[0][k].dtype != runs[1][k].dtype or not torch.equal(raw(runs[0][k]), raw(runs[1][k]))]
    assert not diff, diff
