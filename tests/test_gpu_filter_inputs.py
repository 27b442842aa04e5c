"""The four-lanes-per-particle filter kernels (N <= 128) fetch a step's inputs once per quad: lane p loads fields p, p + 4, ..
of the particle's field list and the quad hands them round with v_mov_dpp.  These cases are the smallest shapes at which a
quad can read the wrong field or the wrong neighbour: a partial quad row (N = 3), an exact DPP row (16), one particle into the
next row (17), all eight waves (128); the peeled steps alone (T = 1), one ordinary step between them (2), a non-zero sequence
offset (3, B = 2); widths at which the field list changes length and crosses a multiple of four; every wiring that adds or
drops a field.

Every case runs with PSVO_TUNE_FILTER_BWD = 0: by default a reverse pass with bootstrap, resampling and no upstream gradient
goes to the affine scan (fbs_*), and these tests are about filter_bwd_lpp_kernel.  Every shape is one that both quad kernels
are instantiated for (one hidden layer: Dx <= 3 at H = 32; Dx = 4 with two hidden layers), except the H = 16 case, which is
there for the forward kernel's Dx = 4 one-layer build.

Each case is run free, with its gradients.  Values: the fp64 oracle is re-run with the kernel's own indices (helpers.
replay_with_hip_indices), every value must agree to the tolerances of tests/test_gpu_parity.py and every index must be the
oracle's draw or lie within EDGE_TOL of a CDF edge (tests/test_gpu_large.py).  Gradients: autograd of the fp64 oracle on the
same indices, 2e-3 of a tensor's largest entry (test_gpu_parity._check_grads)."""
import pytest
import torch

from psvo_amd import _lib
from tests import helpers as Hh
from tests.test_gpu_large import EDGE_TOL, _compare, _hip_noise, _teacher
from tests.test_gpu_parity import _check_grads, _oracle_grads, _setup

pytestmark = pytest.mark.gpu

_NT = [(n, t) for n in (3, 16, 17, 128) for t in (1, 2, 3)]
_WIDTHS = [(2, 1), (3, 2), (2, 2), (3, 1)]
_TWO = dict(q1_layers="32,32", f_layers="32,32", g_layers="32,32")
# objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q.  Every (N, T) pair with the default wiring (bootstrap, two proposals,
# resampling) and no upstream gradient, the widths in turn: 16 or 18 fields in the reverse kernel, 6 to 9 in the forward one
GRID = [(("AESMC", 2, t, n, 1, dx, dy, 32, True, True), {}) for k, (n, t) in enumerate(_NT) for dx, dy in [_WIDTHS[k % 4]]]
# ... and the instantiation of the flagship workload (Dx = 2, Dy = 1) with the upstream dFm / dlogW / dlse of a backward simulation
GRID += [(("PSVO", 2, t, n, 4, 2, 1, 32, True, True), {}) for n in (16, 17, 128) for t in (2, 3)]
WIRINGS = [
    (("AESMC", 2, 3, 17, 1, 4, 1, 16, True, True), {}),                  # Dx = 4 in the one-layer forward quad kernel
    (("AESMC", 2, 3, 17, 1, 4, 2, 32, False, True), _TWO),               # two hidden layers, Dx = 4, P1 and MLP_f loads
    (("AESMC", 2, 2, 16, 1, 4, 1, 32, True, True), _TWO),                # ... with bootstrap (the last slot is skipped)
    (("AESMC", 2, 3, 17, 1, 2, 1, 32, False, True), {}),                 # non-bootstrap
    (("AESMC", 2, 1, 128, 1, 3, 2, 32, False, True), {}),
    (("AESMC", 2, 3, 17, 1, 3, 1, 32, False, False), {}),                # ... without mu2
    (("AESMC", 2, 3, 17, 1, 2, 1, 32, True, False), {}),                 # one proposal (no mu2)
    (("AESMC", 2, 2, 3, 1, 3, 2, 32, True, False), {}),
    (("IWAE", 2, 3, 17, 1, 2, 1, 32, True, True), {}),                   # resampling off
    (("IWAE", 2, 2, 128, 1, 3, 2, 32, False, True), {}),
]
# the `tiny` sizes of bench.py: PSVO hands dFm / dlogW / dlse to the reverse filter, AESMC none of them
OBJECTIVES = [
    (("PSVO", 4, 12, 32, 8, 2, 1, 32, True, True), {}),
    (("AESMC", 4, 12, 32, 8, 2, 1, 32, True, True), {}),
    (("PSVO", 2, 3, 17, 4, 3, 1, 32, False, True), {}),
    (("SVO", 2, 3, 17, 1, 2, 2, 32, True, True), {}),
]


def _id(p):
    case, extra = p
    return "-".join(map(str, case)) + ("-2L" if extra else "")


def _pass(model, smc, obs, nz):
    model.zero_grad()
    z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    z.backward()
    torch.cuda.synchronize()
    return z.detach(), log


def _free_run_against_oracle(case, extra, seed, route=0):
    with Hh.tuning(_lib.PSVO_TUNE_FILTER_BWD, route):
        _free_run(case, extra, seed)


def _free_run(case, extra, seed):
    obj = case[0]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=seed, **extra)
    nz = Hh.noise_to_hip(noise, "cuda")
    z, log = _pass(model, smc, obs, nz)
    if FLAGS.IWAE:                                   # (no draws: nothing to replay)
        z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
        teacher = {}
    else:
        z_ref, ref, st = Hh.replay_with_hip_indices(model, FLAGS, obj, obs, noise, log)
        print("draws=%d flipped=%d worst edge distance=%.3e" % (st["draws"], st["off"], st["worst"]))
        assert st["worst"] <= EDGE_TOL, st
        teacher = Hh.hip_indices(log, obj)
    _compare(obj, log, ref, z, z_ref)
    assert torch.allclose(log["filter"]["lse"].double().cpu(), torch.logsumexp(ref["log_Ws"], 1), atol=5e-4, rtol=1e-5)
    zg, P = _oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    assert abs(float(z) - float(zg)) <= 1e-4 * abs(float(zg))
    _check_grads(model, P, rerun=lambda: _pass(model, smc, obs, nz))


@pytest.mark.parametrize("case,extra", GRID, ids=map(_id, GRID))
def test_quad_inputs_shapes(built_lib, case, extra):
    _free_run_against_oracle(case, extra, seed=31)


@pytest.mark.parametrize("case,extra", WIRINGS, ids=map(_id, WIRINGS))
def test_quad_inputs_wirings(built_lib, case, extra):
    _free_run_against_oracle(case, extra, seed=33)


@pytest.mark.parametrize("case,extra", OBJECTIVES, ids=map(_id, OBJECTIVES))
def test_quad_inputs_objectives(built_lib, case, extra):
    _free_run_against_oracle(case, extra, seed=35)


def test_quad_inputs_default_route(built_lib):
    """the flagship wiring as shipped (PSVO_TUNE_FILTER_BWD = 1: with an upstream gradient the quad kernel runs)"""
    _free_run_against_oracle(*OBJECTIVES[0], seed=36, route=1)


TEACHER = [(("AESMC", 2, 3, 17, 1, 2, 1, 32, True, True), {}), (("PSVO", 2, 3, 16, 4, 3, 2, 32, False, True), {})]


@pytest.mark.parametrize("case,extra", TEACHER, ids=map(_id, TEACHER))
def test_quad_inputs_teacher_forced(built_lib, case, extra):
    """the oracle's ancestor indices go in (idx_f shares the field of the uniforms): values and every gradient"""
    with Hh.tuning(_lib.PSVO_TUNE_FILTER_BWD, 0):
        _teacher_forced(case, extra)


def _teacher_forced(case, extra):
    obj = case[0]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=37, **extra)
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = _teacher(ref, obj)
    nz = _hip_noise(noise, teacher)
    z, log = _pass(model, smc, obs, nz)
    assert torch.equal(log["filter"]["idx"].permute(0, 2, 1).cpu().long(), ref["idx_f"])
    _compare(obj, log, ref, z, z_ref)
    zg, P = _oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    assert abs(float(z) - float(zg)) <= 1e-4 * abs(float(zg))
    _check_grads(model, P, rerun=lambda: _pass(model, smc, obs, nz))


REPEAT = [(("PSVO", 4, 12, 32, 8, 2, 1, 32, True, True), {}), (("AESMC", 2, 3, 17, 1, 3, 2, 32, False, True), {}),
          (("AESMC", 2, 2, 3, 1, 4, 2, 32, False, True), _TWO)]


@pytest.mark.parametrize("case,extra", REPEAT, ids=map(_id, REPEAT))
def test_quad_inputs_repeatable(built_lib, case, extra):
    """the same inputs twice: every output and every gradient byte-equal (a broadcast from a lane that was not loaded, or a
    field read before its load has landed, does not repeat)"""
    FLAGS, model, smc, obs, noise = _setup(*case, seed=39, **extra)
    nz = Hh.noise_to_hip(noise, "cuda")
    runs = []
    for _ in range(2):
        with Hh.tuning(_lib.PSVO_TUNE_FILTER_BWD, 0):
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
