"""bsim_bwd2_kernel (the reverse backward simulation, "j on lanes") requests a step's inputs and the next forward tile a step
ahead and waits for them in one place, the rotation that ends the step.  These cases are the smallest shapes at which a word
moved across a wait can be consumed before it has landed, or a load can read the wrong step:

  T = 2 (no ordinary step, only the tile staged in front of the loop), 3 (one ordinary step, one tile staged inside the
  loop), 4 (both tile buffers restaged inside the loop), 5.  T = 1, where the two peeled steps would coincide, is not a
  shape the library runs: psvo_bsim_forward / psvo_bsim_backward return PSVO_ERR_INVALID for T < 2, so the kernel's T == 1
  path cannot be reached through the ABI (test_single_step_is_refused pins that down instead);
  N = 3 (a partial tile: the entry index clamps), 16, 17, 128 (several workgroups), and 300 at Dx = 3 (the tile's second 256
  entries travel through the second register set);
  M = 4, 8, 16, 32 (chains per wave, and with them the tail of lanes without a chain);
  (Dx, Dy) = (2, 1), (2, 2), (3, 1), (3, 2): Dx <= 2 requests at the top of the step, Dx = 3 behind the pair phase;
  B = 2 everywhere, so the sequence offset is not zero; one and two hidden layers (two: the v1 kernel family, which shares
  the host path).

GRID crosses N and T and walks (Dx, Dy) and M along both, so that each of the sixteen (width, M) pairs occurs once.  Every
case runs teacher-forced (the oracle's indices go in) under the library's default route, values and every gradient against the
fp64 oracle with the tolerances of tests/test_gpu_parity.py and tests/test_gpu_large.py.  One shape runs v1 as the control
and one each the three matrix-instruction variants of v2 (Dx = 2, where tests/test_gpu_parity.py::test_bsim_backward_variants
runs them).  Three shapes run twice on the same inputs and must repeat byte for byte."""
import pytest
import torch

from psvo_amd import _lib
from tests import helpers as Hh
from tests.test_gpu_large import _compare, _hip_noise, _teacher
from tests.test_gpu_parity import _check_grads, _oracle_grads, _setup

pytestmark = pytest.mark.gpu

_NS, _TS = (3, 16, 17, 128), (2, 3, 4, 5)
_WIDTHS = [(2, 1), (2, 2), (3, 1), (3, 2)]
_MS = (4, 8, 16, 32)
_TWO = dict(q1_layers="32,32", g_layers="32,32")
# objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q.  (i + j, 2 i + j) mod 4 is a bijection of the 4 x 4 grid
GRID = [(("PSVO", 2, t, n, _MS[(2 * i + j) % 4]) + _WIDTHS[(i + j) % 4] + (32, True, True), {})
        for i, n in enumerate(_NS) for j, t in enumerate(_TS)]
# more than 256 tile entries at Dx = 3
GRID += [(("PSVO", 2, 2, 300, 8, 3, 1, 32, True, True), {}), (("PSVO", 2, 3, 300, 4, 3, 2, 32, True, True), {}),
         (("PSVO", 2, 5, 300, 16, 3, 1, 32, True, True), {})]
# two hidden layers
GRID += [(("PSVO", 2, 3, 17, 4, 2, 1, 32, True, True), _TWO), (("PSVO", 2, 2, 16, 8, 3, 2, 32, True, True), _TWO)]
# PSVO_TUNE_BSIM_BWD: 0 = v1, 2 .. 4 = the matrix-instruction variants of v2
VARIANTS = [(0, ("PSVO", 2, 3, 17, 8, 2, 1, 32, True, True)), (2, ("PSVO", 2, 3, 17, 4, 2, 2, 32, True, True)),
            (3, ("PSVO", 2, 5, 128, 16, 2, 1, 32, True, True)), (4, ("PSVO", 2, 2, 16, 32, 2, 1, 32, True, True))]
REPEAT = [("PSVO", 2, 3, 17, 4, 2, 1, 32, True, True), ("PSVO", 2, 5, 128, 16, 2, 2, 32, True, True),
          ("PSVO", 2, 3, 16, 8, 3, 1, 32, True, True)]


def _id(p):
    case, extra = p
    return "-".join(map(str, case)) + ("-2L" if extra else "")


def _pass(model, smc, obs, nz):
    model.zero_grad()
    z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
    z.backward()
    torch.cuda.synchronize()
    return z.detach(), log


def _teacher_forced(case, extra, seed, variant=-1):
    obj = case[0]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=seed, **extra)
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = _teacher(ref, obj)
    nz = _hip_noise(noise, teacher)
    with Hh.tuning(_lib.PSVO_TUNE_BSIM_BWD, variant):
        z, log = _pass(model, smc, obs, nz)
    _compare(obj, log, ref, z, z_ref)
    zg, P = _oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    assert abs(float(z) - float(zg)) <= 1e-4 * abs(float(zg))
    _check_grads(model, P)


@pytest.mark.parametrize("case,extra", GRID, ids=map(_id, GRID))
def test_prefetch_shapes(built_lib, case, extra):
    _teacher_forced(case, extra, seed=41)


def test_single_step_is_refused(built_lib):
    """T = 1: the backward simulation is refused by the ABI (PSVO_ERR_INVALID -> ValueError), nothing is launched"""
    FLAGS, model, smc, obs, noise = _setup("PSVO", 2, 1, 16, 4, 2, 1, 32, True, True, seed=41)
    with pytest.raises(ValueError):
        smc.get_log_ZSMC(obs.float().cuda(), None, noise=Hh.noise_to_hip(noise, "cuda"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("variant,case", VARIANTS, ids=lambda v: str(v) if isinstance(v, int) else "-".join(map(str, v)))
def test_prefetch_variants(built_lib, variant, case):
    _teacher_forced(case, {}, seed=43, variant=variant)


@pytest.mark.parametrize("case", REPEAT, ids=lambda c: "-".join(map(str, c)))
def test_prefetch_repeatable(built_lib, case):
    """the same inputs twice: every output and every gradient byte-equal (a word consumed before its load has landed does not
    repeat)"""
    FLAGS, model, smc, obs, noise = _setup(*case, seed=45)
    nz = Hh.noise_to_hip(noise, "cuda")
    runs = []
    for _ in range(2):
        z, log = _pass(model, smc, obs, nz)
        out = {"z": z.cpu().clone(), "Xs": log["Xs"].detach().cpu().clone()}
        for part, keys in (("filter", ("X", "Xanc", "Fm", "logW", "idx", "lse")), ("bsim", ("bwX", "flp", "glp", "Omega", "sel"))):
            out.update({part + "." + k: log[part][k].detach().cpu().clone() for k in keys})
        out.update({"grad." + n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None})
        runs.append(out)
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) > 8
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8)
    diff = [k for k in runs[0] if runs[0][k].dtype != runs[1][k].dtype or not torch.equal(raw(runs[0][k]), raw(runs[1][k]))]
    assert not diff, diff
