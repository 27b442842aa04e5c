"""bsim_bwd2_kernel ("j on lanes" reverse backward simulation) after the instructions that compute nothing were taken out
of its time step: the per-j sums d F'_j / d W^_j take round 0's term instead of adding it to a zero, the lane offsets of the
arrays stay what they are while the step moves the scalar base, the late row stores and the d Fm / d logW fold address with a
32-bit lane offset, and the cross-lane sums over lane bits 2, 4 and 5 add both operands of a stage in place (no select).

Every case runs the objective teacher-forced (the oracle's indices go in) with PSVO_TUNE_BSIM_BWD set, so that
ops.bsim_forward(save=True) / ops.bsim_backward run the kernel under test whatever the default route of the shape is, and
compares the ELBO and EVERY parameter gradient with the fp64 oracle.  Yardstick of tests/test_gpu_instantiations.py, per
tensor: err <= max(2e-3 * scale + 1e-6, 4 x the error the oracle itself makes on that tensor in fp32); the fp32 oracle is
only run for a case in which some tensor misses the first clause (the assertion is the same).  The same inputs twice must give
torch.equal gradients.

Shapes (B = 2 everywhere: a sequence offset that is not zero):
  N = 5    lanes without a chain, one partial workgroup, a tile of 5 entries padded to 128
  N = 24   part of one chunk
  N = 130  NP = 256: two chunks at Dx = 2, so a chunk's per-j sums are started twice per step and the U / V sums run across
           chunks; more than one workgroup per sequence
  T = 2, 3, 5   the first and the last step's arms with none, one and three ordinary steps between them
  M = 4, 16     eight and two chains per wave
  one case each for the pair exponents on v_mfma_f32_16x16x4_f32 and on v_mfma_f32_16x16x32_bf16 (tuning 3 and 4: JM = 2, 3),
  Dx = 3 (chunks of four tiles) and Dx = 4 with v2 forced (rounds outer, two tiles per chunk).
One case runs a training step eager and replayed from the captured graph."""
import itertools

import pytest
import torch

from psvo_amd import _lib
from tests import helpers as Hh
from tests import test_gpu_parity as TP

pytestmark = pytest.mark.gpu

K32 = 4.0
V2 = 1              # PSVO_TUNE_BSIM_BWD: v2 with the per-j sums on the VALU (JM = 0)
# objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q
GRID = [(V2, ("PSVO", 2, t, n, m, 2, dy, 32, True, True))
        for dy, m, n, t in itertools.product((1, 2), (4, 16), (5, 24, 130), (2, 3, 5))]
OTHER = [(3, ("PSVO", 2, 3, 24, 16, 2, 1, 32, True, True)), (4, ("PSVO", 2, 3, 24, 16, 2, 1, 32, True, True)),
         (V2, ("PSVO", 2, 3, 20, 8, 3, 1, 32, True, True)), (V2, ("PSVO", 2, 3, 20, 8, 4, 1, 32, True, True))]


def _id(v):
    return str(v) if isinstance(v, int) else "-".join(map(str, v))


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _run(variant, case, seed):
    obj = case[0]
    FLAGS, model, smc, obs, noise = TP._setup(*case, seed=seed)
    _, ref0 = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = {"idx_f": ref0["idx_f"], "idx_b": ref0["idx_b"]}
    z_ref, P = TP._oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    nz = Hh.noise_to_hip({**noise, **teacher}, "cuda")
    nz.pop("u_f", None); nz.pop("u_b", None)
    runs = []
    with Hh.tuning(_lib.PSVO_TUNE_BSIM_BWD, variant):
        for _ in range(2):
            model.zero_grad()
            z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
            z.backward()
            torch.cuda.synchronize()
            runs.append((z.detach().clone(), _grads(model)))
    assert abs(float(runs[0][0]) - float(z_ref)) <= 1e-4 * abs(float(z_ref))
    # the two calls against each other
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1].keys() == runs[1][1].keys() and len(runs[0][1]) > 8
    diff = [n for n in runs[0][1] if not torch.equal(runs[0][1][n], runs[1][1][n])]
    assert not diff, "gradients differ between two calls: %s" % diff
    # every gradient against the fp64 oracle
    rows = []
    for name, p, ref in TP._pairs(model, P):
        g = torch.zeros_like(ref) if p.grad is None else p.grad.detach().double().cpu()
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        rows.append((name, float((g - r).abs().max()), max(float(r.abs().max()), 1e-6), r))
    if all(err <= 2e-3 * scale + 1e-6 for _, err, scale, _ in rows):
        return
    _, P32 = TP._oracle_grads(model, FLAGS, obj, obs, noise, teacher, dtype=torch.float32)
    bad = []
    for (name, err, scale, r), (_, _, ref32) in zip(rows, TP._pairs(model, P32)):
        r32 = torch.zeros_like(r) if ref32.grad is None else ref32.grad.double()
        err32 = float((r32 - r).abs().max())
        if err > max(2e-3 * scale + 1e-6, K32 * err32):
            bad.append((name, err, scale, err32))
    assert not bad, "gradient mismatch (name, max abs err, own scale, fp32 oracle's own err): %s" % bad


@pytest.mark.parametrize("variant,case", GRID, ids=_id)
def test_diet_shapes(built_lib, variant, case):
    _run(variant, case, seed=51)


@pytest.mark.parametrize("variant,case", OTHER, ids=_id)
def test_diet_other_instantiations(built_lib, variant, case):
    _run(variant, case, seed=53)


def test_diet_step_replays_from_hipgraph(built_lib):
    """a local training step with v2 forced, eager and captured into a GraphedStep: every replay equals the eager step bit for
    bit and rewrites every gradient itself"""
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    FLAGS, model, smc, obs, noise = TP._setup("PSVO", 2, 5, 130, 16, 2, 1, 32, True, True, seed=55)
    nz = Hh.noise_to_hip(noise, "cuda")
    flat = FlatParams(model)
    obs_c = obs.float().cuda()

    def local():
        flat.zero_grad()
        z, _ = smc.get_log_ZSMC(obs_c, None, noise=nz)
        z.backward()
        return z.detach()
    with Hh.tuning(_lib.PSVO_TUNE_BSIM_BWD, V2):
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
