"""bsim_fwd_kernel after the instructions that compute nothing were taken out of its step (profiles/bsim_fwd_valu_diet.md):
the first 16-entry block of a step assigns the running sums instead of rescaling zeros, the cross-half add of the quad / half
merge comes behind the `i == q` select, and the cross-lane sums and maxima go through add_xor / max_xor (common.h).  These
are the smallest shapes at which each of those can go wrong.  B = 2 and H = 32 throughout; with two half-chains (HS = 2) the
forward tile is padded to NP = 32 ceil(N / 32) entries and a quad lane walks nqh = NP / 8 of them per half:

  which block is a step's first, and whether a later block still rescales:
    N = 17 (nqh 4: one 4-entry block, the general form as first block), 33 (nqh 8: one 8-entry block), 96 (nqh 12 = 8 + 4),
    112 (nqh 16: the first-block form alone, what C* runs), 192 (nqh 24 = 16 + 8: a general block follows the first-block
    form and must rescale), 224 (nqh 28 = 16 + 8 + 4: all three arms), 256 (nqh 32: two 16-entry blocks, the second in the
    loop), 512 (nqh 64: four); T = 3 or 4;
  a lane whose whole slice is padding (W' = -inf: sum 0 and maximum -inf through the merge): N = 3 and N = 5;
  the cross-half stage on each mask: M = 4 (xor 4), 8 (xor 8), 16 (permlane16), 32 (permlane32), each with HS = 2;
  HS = 1, which has no cross-half stage: the B N M = 131072 shape of tests/test_gpu_bsim_fwd_prefetch.py, forward values;
  widths (Dx, Dy) = (2, 1), (2, 2), (3, 1), (3, 2) walked along the grid, one Dx = 4 case (the unpeeled loop) and one with two
  hidden layers.

Every grid case runs teacher-forced against the fp64 oracle, values and every gradient, with the tolerances of
tests/test_gpu_parity.py and tests/test_gpu_large.py.  The free-running arm (the one the benchmark runs): three shapes run
with uniforms, then with the run's own indices fed back, then with the uniforms again, byte-equal in all three."""
import pytest
import torch

from tests import helpers as Hh
from tests.test_gpu_bsim_fwd_prefetch import WHOLE_CHAIN, _differing, _outputs, _pass
from tests.test_gpu_large import _compare, _hip_noise, _teacher
from tests.test_gpu_parity import _check_grads, _oracle_grads, _setup

pytestmark = pytest.mark.gpu

_WIDTHS = [(2, 1), (2, 2), (3, 1), (3, 2)]
_MS = (4, 8, 16, 32)
_TWO = dict(q1_layers="32,32", g_layers="32,32")


def _case(n, t, m, width):
    return ("PSVO", 2, t, n, m) + width + (32, True, True)


# first walk: every N once, M and the width moving together; second walk: the block-structure shapes again with M and the
# width shifted against each other, so that each arm meets every mask and Dx = 2 and 3
_NS1 = (3, 5, 17, 33, 96, 112, 192, 224, 256, 512)
_NS2 = (17, 96, 112, 192, 224, 256)
GRID = [(_case(n, 3 + i % 2 if n < 256 else 3, _MS[i % 4] if n < 256 else _MS[i % 2], _WIDTHS[i % 4]), {})
        for i, n in enumerate(_NS1)]
GRID += [(_case(n, 4 - j % 2 if n < 256 else 3, _MS[(j + 2) % 4] if n < 256 else 4, _WIDTHS[(j + 1) % 4]), {})
         for j, n in enumerate(_NS2)]
GRID += [(_case(192, 3, 8, (4, 1)), {}),        # Dx = 4: the unpeeled time loop
         (_case(192, 3, 16, (2, 1)), _TWO)]     # two hidden layers, two waves per SIMD
FREE = [_case(17, 3, 4, (2, 1)), _case(192, 4, 16, (3, 2)), _case(112, 3, 8, (4, 1))]


def _id(p):
    case, extra = p
    return "-".join(map(str, case)) + ("-2L" if extra else "")


def test_grid_covers_what_it_claims():
    cases = [c for c, _ in GRID]
    assert {c[3] for c in cases} >= {3, 5, 17, 33, 96, 112, 192, 224, 256, 512}
    for n in (112, 192, 224):      # every block structure with every cross-half mask family and both narrow Dx
        assert {c[5] for c in cases if c[3] == n} >= {2, 3}
    assert {c[4] for c in cases} == set(_MS) and {(c[5], c[6]) for c in cases} >= set(_WIDTHS)
    assert all(c[1] * c[3] * c[4] < 131072 for c in cases)      # two half-chains everywhere


@pytest.mark.parametrize("case,extra", GRID, ids=map(_id, GRID))
def test_diet_shapes(built_lib, case, extra):
    obj = case[0]
    FLAGS, model, smc, obs, noise = _setup(*case, seed=61, **extra)
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    teacher = _teacher(ref, obj)
    z, log = _pass(model, smc, obs, _hip_noise(noise, teacher))
    _compare(obj, log, ref, z, z_ref)
    zg, P = _oracle_grads(model, FLAGS, obj, obs, noise, teacher)
    assert abs(float(z) - float(zg)) <= 1e-4 * abs(float(zg))
    _check_grads(model, P)


def test_diet_whole_chain_lanes(built_lib):
    """HS = 1 (no cross-half stage anywhere), reached by size: forward values against the oracle"""
    obj = WHOLE_CHAIN[0]
    assert WHOLE_CHAIN[1] * WHOLE_CHAIN[3] * WHOLE_CHAIN[4] == 131072
    FLAGS, model, smc, obs, noise = _setup(*WHOLE_CHAIN, seed=63)
    z_ref, ref = Hh.run_oracle(model, FLAGS, obj, obs, noise)
    with torch.no_grad():
        z, log = smc.get_log_ZSMC(obs.float().cuda(), None, noise=_hip_noise(noise, _teacher(ref, obj)))
    torch.cuda.synchronize()
    _compare(obj, log, ref, z, z_ref)


@pytest.mark.parametrize("case", FREE, ids=lambda c: "-".join(map(str, c)))
def test_diet_free_running(built_lib, case):
    """uniforms in; the run's own indices fed back; the uniforms again: one result, byte for byte"""
    FLAGS, model, smc, obs, noise = _setup(*case, seed=65)
    nz = Hh.noise_to_hip(noise, "cuda")
    assert "u_b" in nz and "sel_b" not in nz
    free, sel = _outputs(model, smc, obs, nz)
    fed = {k: v for k, v in nz.items() if k != "u_b"}
    fed["sel_b"] = sel.contiguous()
    forced, _ = _outputs(model, smc, obs, fed)
    again, _ = _outputs(model, smc, obs, nz)
    assert not _differing(free, forced), _differing(free, forced)
    assert not _differing(free, again), _differing(free, again)
