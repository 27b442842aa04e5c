"""Deterministic mode (PSVO_TUNE_DETERMINISTIC = 1, or torch.use_deterministic_algorithms(True)): the fixed-order routes run,
the gradients repeat bit for bit, they still match the fp64 oracle, and a captured GraphedStep keeps the mode it was captured
under.

Routes under the mode (include/psvo_hip.h): the persistent reverse filter takes filter_bwd_kernel<.., true> where the default
adds with LDS float atomics in arrival order (N > 256: no per-wave copies fit), the cov reverse filter filter_cov_bwd_kernel<..,
true> wherever it is not the affine scan and has more than one wave, and the cov backward simulations (PSVO and PSVOwR)
bsim_cov_bwd_kernel<.., true> with bsim_cov_det_fold (and, PSVOwR, bsim_cov_det_gather) after every step.  The DET filter
kernels keep c <= waves copies of the scatter targets and add in ceil(waves / c) phases; N = 300 (five waves) and N = 400 (seven
waves; Dx = 4 without bootstrap: fewer copies than waves, several phases) cover the wave counts that are not a power of two."""
import contextlib
import re

import pytest
import torch

from psvo_amd import _lib
from tests import helpers as Hh
from tests import test_gpu_parity as TP
from tests.test_gpu_streams import _reproducible

pytestmark = pytest.mark.gpu

DET = _lib.PSVO_TUNE_DETERMINISTIC
COV = dict(output_cov=True, diag_cov=True)
# (objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q)
PLAIN_512 = ("AESMC", 4, 8, 512, 4, 2, 1, 32, False, True)            # no bootstrap: the persistent reverse filter
C5_SMALL = ("PSVO", 4, 30, 512, 16, 4, 1, 32, True, True)              # C5 shapes; PSVO_TUNE_FILTER_BWD = 0: persistent
COV_CASES = [("SVO", 4, 8, 128, 4, 2, 1, 32, False, True), ("AESMC", 4, 8, 512, 4, 2, 1, 32, False, True),
             ("IWAE", 4, 8, 512, 4, 2, 2, 32, True, True), ("AESMC", 4, 8, 128, 4, 3, 1, 32, True, True),
             ("PSVO", 4, 6, 128, 8, 2, 1, 32, True, True), ("PSVO", 4, 4, 512, 4, 2, 1, 32, False, True),
             ("PSVOwR", 4, 6, 128, 8, 2, 1, 32, True, True), ("PSVOwR", 4, 4, 512, 4, 2, 1, 32, False, True)]
ODD_WAVES = [("AESMC", 4, 8, 300, 4, 2, 1, 32, False, True),      # five waves
             ("AESMC", 4, 8, 400, 4, 4, 1, 64, False, True)]      # seven waves, fewer copies than waves (cov)


@contextlib.contextmanager
def torch_deterministic(warn_only=False):
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=warn_only)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


def _ids(c):
    return "-".join(map(str, c))


def _one_pass(case, extra, seed=3):
    FLAGS, model, smc, obs, noise = TP._setup(*case, seed=seed, **extra)
    nz = Hh.noise_to_hip(noise, "cuda")

    def run():
        model.zero_grad()
        z, _ = smc.get_log_ZSMC(obs.float().cuda(), None, noise=nz)
        z.backward()
        torch.cuda.synchronize()
    return run


def _det_instances(names, family):
    return [n for n in names if re.search(r"(^|[^A-Za-z0-9_])%s<[^>]*\btrue>" % family, n)]


@pytest.mark.parametrize("case,extra,family", [(PLAIN_512, {}, "filter_bwd_kernel"),
                                               (COV_CASES[0], COV, "filter_cov_bwd_kernel"),
                                               (COV_CASES[1], COV, "filter_cov_bwd_kernel"),
                                               (COV_CASES[4], COV, "bsim_cov_bwd_kernel"),
                                               (COV_CASES[6], COV, "bsim_cov_bwd_kernel")],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else None)
def test_fixed_order_route_runs(built_lib, case, extra, family):
    run = _one_pass(case, extra)
    with Hh.tuning(DET, 0):
        _, names = Hh.kernel_names(run)
    assert not _det_instances(names, family), "the default mode ran a fixed-order kernel: %s" % sorted(names)
    assert not [n for n in names if "bsim_cov_det_" in n]
    with Hh.tuning(DET, 1):
        _, names = Hh.kernel_names(run)
    assert _det_instances(names, family), "%s<.., true> did not run under the mode; kernels: %s" % (family, sorted(names))
    if family == "bsim_cov_bwd_kernel":
        assert [n for n in names if "bsim_cov_det_fold" in n], sorted(names)
        assert bool([n for n in names if "bsim_cov_det_gather" in n]) == (case[0] == "PSVOwR"), sorted(names)
    with Hh.tuning(DET, 0), torch_deterministic():
        _, names = Hh.kernel_names(run)
        assert _det_instances(names, family), "torch.use_deterministic_algorithms did not select %s<.., true>" % family
        assert _lib.load().psvo_get_tuning(DET) == 0      # (the wrapper restored the switch)


@pytest.mark.parametrize("case", COV_CASES, ids=_ids)
def test_cov_gradients_are_bit_reproducible(built_lib, case):
    with torch_deterministic():
        _reproducible(TP._setup(*case, seed=21, **COV))


def test_plain_n512_gradients_are_bit_reproducible(built_lib):
    with torch_deterministic(), Hh.tuning(_lib.PSVO_TUNE_FILTER_BWD, 0):
        _reproducible(TP._setup(*PLAIN_512, seed=22))
        _reproducible(TP._setup(*C5_SMALL, seed=23))


@pytest.mark.parametrize("case", ODD_WAVES, ids=_ids)
def test_odd_wave_counts_are_bit_reproducible(built_lib, case):
    with torch_deterministic():
        _reproducible(TP._setup(*case, seed=25))
        _reproducible(TP._setup(*case, seed=26, **COV))


@pytest.mark.parametrize("case", COV_CASES[:2] + COV_CASES[4:] + ODD_WAVES[1:], ids=_ids)
def test_fixed_order_cov_routes_match_the_oracle(built_lib, case):
    """teacher-forced indices, every gradient (both heads of every MLP, sigma_con) at the bars of test_gpu_parity"""
    from tests.test_gpu_variants import OracleOnce
    OracleOnce(case, seed=7, **COV).hip(settings=((DET, 1),))


def test_fixed_order_n512_route_matches_the_oracle(built_lib):
    """teacher-forced indices (a free-running draw over 512 particles need not pick the oracle's ancestors)"""
    from tests.test_gpu_variants import PERSISTENT, OracleOnce
    OracleOnce(PLAIN_512, seed=7).hip(settings=((DET, 1),), route=PERSISTENT,
                                      names_check=lambda names: _det_instances(names, PERSISTENT) or pytest.fail(
                                          "filter_bwd_kernel<.., true> did not run: %s" % sorted(names)))


def test_graphed_step_keeps_its_capture_mode(built_lib):
    from psvo_amd.graph import GraphedStep
    from psvo_amd.optim import FlatParams
    FLAGS, model, smc, obs, noise = TP._setup(*PLAIN_512, seed=24)
    nz = Hh.noise_to_hip(noise, "cuda")
    flat = FlatParams(model)
    obs_c = obs.float().cuda()

    def local():
        flat.zero_grad()
        z, _ = smc.get_log_ZSMC(obs_c, None, noise=nz)
        z.backward()
        return z.detach()
    with Hh.tuning(DET, 1):
        step = GraphedStep(local)
        assert step.deterministic
        step()
        torch.cuda.synchronize()
    with Hh.tuning(DET, 0), pytest.raises(RuntimeError, match="capture the step again"):
        step()
    with Hh.tuning(DET, 0), torch_deterministic():
        step()                  # (torch's flag turns the mode on as well)
        torch.cuda.synchronize()
