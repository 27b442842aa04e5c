"""Every reverse-pass route that a psvo_set_tuning switch (include/psvo_hip.h) or the workspace can select, against the fp64
oracle: the header promises the same results to rounding under every value, and a route no test takes is untested code.

The fp64 oracle's ELBO and autograd gradients are computed once per case (teacher-forced indices, as test_filter_gradients);
then one HIP forward + reverse pass runs per setting, each checked with the bars of tests/test_gpu_parity.py (ELBO rel 1e-4,
every gradient 2e-3 of its tensor's largest entry).  Each pass runs under torch.profiler and asserts that the kernel family the
setting is meant to select is the one that ran: a variant test that silently takes the default route proves nothing.

Routes of psvo_filter_backward (filter_bwd.hip: launch_filter_bwd) in the bootstrap wiring with resampling, one hidden layer:
  PSVO_TUNE_FILTER_BWD = 1 (default): the affine scan (fbs_*) without an upstream gradient (AESMC / SVO) or at N > 256;
                         2: the scan wherever it applies;  0: never the scan.
  Otherwise: four lanes per particle (filter_bwd_lpp_kernel) at N <= 128, H <= 32, Dx <= 3; else filter_bwd_kernel<.., 256|512>.
psvo_filter_backward_cov: the scan (fcs_*) in the bootstrap wiring with resampling unless the switch is 0, else
filter_cov_bwd_kernel.  The scan keeps a ring of D1 = 16 / 12 / 8 prefetched steps (Dx = 2 / 3 / 4) at N <= 64 and N in
(128, 256], D1 / 2 otherwise: the T = 40 cases below wrap every ring at least twice."""
import contextlib
import re

import pytest
import torch

from oracle import psvo_oracle as O
from psvo_amd import _lib
from tests import helpers as Hh
from tests import test_gpu_parity as TP
from tests.test_gpu_large import LARGE, _hip_noise, _teacher

pytestmark = pytest.mark.gpu

SCAN, LPP, PERSISTENT = "fbs_scan_kernel", "filter_bwd_lpp_kernel", "filter_bwd_kernel"
COV_SCAN, COV_PERSISTENT = "fcs_scan_kernel", "filter_cov_bwd_kernel"
FILTER_FAMILIES = (SCAN, LPP, PERSISTENT)
COV_FAMILIES = (COV_SCAN, COV_PERSISTENT)
V1, V2 = "bsim_bwd_kernel", "bsim_bwd2_kernel"


def _ids(c):
    if isinstance(c, tuple):
        return "-".join(map(str, c))
    if isinstance(c, dict):
        return ",".join("%s=%s" % kv for kv in c.items())
    return str(c)


def filter_route(case, setting, aligned=True):
    """the reverse-filter kernel family psvo_filter_backward launches for `case` (one hidden layer, no covariance heads)"""
    obj, B, T, N, M, Dx, Dy, H, boot, two_q = case
    resample = obj != "IWAE"
    upstream = obj in ("PSVO", "PSVOwR")
    if setting and boot and resample and aligned and (not upstream or N > 256 or setting == 2):
        return SCAN
    if H % 16 == 0 and H <= 32 and Dx <= 3 and N <= 128:
        return LPP
    return PERSISTENT


def cov_route(case, setting):
    obj, boot = case[0], case[8]
    return COV_SCAN if setting and boot and obj != "IWAE" else COV_PERSISTENT


def _family(names, family):
    """kernels of `names` that belong to `family` (name as a whole word: filter_bwd_kernel is not filter_cov_bwd_kernel)"""
    return [n for n in names if re.search(r"(^|[^A-Za-z0-9_])%s\b" % family, n)]


def assert_route(names, want, families):
    assert _family(names, want), "%s did not run; device kernels: %s" % (want, sorted(names))
    for other in families:
        if other != want:
            assert not _family(names, other), "%s ran besides %s: %s" % (other, want, _family(names, other))


class OracleOnce(object):
    """fp64 oracle ELBO and gradients of one case, computed once; hip() runs and checks one HIP pass per setting"""

    def __init__(self, case, seed, fhn=False, per_step_bound=None, **extra):
        self.obj = obj = case[0]
        B, T = case[1], case[2]
        self.FLAGS, self.model, self.smc, obs, noise = TP._setup(*case, seed=seed, **extra)
        if fhn:
            _, obs = O.fhn_synthetic(B, T, seed=3)            # an FHN trajectory, as in the headline workloads
        self.obs = obs
        _, ref0 = Hh.run_oracle(self.model, self.FLAGS, obj, obs, noise)
        teacher = _teacher(ref0, obj)
        self.z_ref, self.P = TP._oracle_grads(self.model, self.FLAGS, obj, obs, noise, teacher)
        if per_step_bound is not None:
            # a random model can run away over a long sequence, and then a relative tolerance compares nothing
            per_step = abs(float(self.z_ref)) / (B * T)
            assert per_step < per_step_bound, "the model ran away: |ELBO| / (B T) = %.3g" % per_step
        self.nz = _hip_noise(noise, teacher)

    def hip_pass(self):
        self.model.zero_grad()
        z, _ = self.smc.get_log_ZSMC(self.obs.float().cuda(), None, noise=self.nz)
        z.backward()
        torch.cuda.synchronize()
        return z

    def hip(self, settings=(), route=None, families=FILTER_FAMILIES, names_check=None, check=True):
        """one HIP forward + reverse pass under the psvo_set_tuning `settings` ((key, value) pairs); `route`: the kernel
        family that must have run (and no other of `families`); `names_check(names)`: any further assertion on the kernels.
        Returns the set of kernel names."""
        with contextlib.ExitStack() as st:
            for key, value in settings:
                st.enter_context(Hh.tuning(key, value))
            z, names = Hh.kernel_names(self.hip_pass)
        if route is not None:
            assert_route(names, route, families)
        if names_check is not None:
            names_check(names)
        if check:
            assert abs(float(z.detach()) - float(self.z_ref)) <= 1e-4 * abs(float(self.z_ref)), (float(z), float(self.z_ref))
            TP._check_grads(self.model, self.P)
        return names

    def grads(self):
        """{name: gradient} of the last HIP pass"""
        return {name: (torch.zeros_like(ref) if p.grad is None else p.grad.detach().double().cpu())
                for name, p, ref in TP._pairs(self.model, self.P)}

    def spread(self, g, g0):
        """largest |g - g0| of any tensor, in units of that tensor's largest oracle entry"""
        out = 0.0
        for name, _, ref in TP._pairs(self.model, self.P):
            scale = max(float(ref.grad.abs().max()) if ref.grad is not None else 0.0, 1e-6)
            out = max(out, float((g[name] - g0[name]).abs().max()) / scale)
        return out


ROUTE_RTOL = 3e-5    # routes against each other (fp32 against fp32; measured spread <= 4e-6 over FILTER_BWD_CASES)


# ---------------------------------------------------------------------------------------------
# B1: psvo_filter_backward under PSVO_TUNE_FILTER_BWD = 0 / 1 / 2
# ---------------------------------------------------------------------------------------------
BOOT_RESAMPLE = [c for c in TP.CASES if c[8] and c[0] != "IWAE"]
# T = 40 puts every scan bucket past its ring depth (N <= 64: 16 / 12 / 8 steps, 64 < N <= 128: 8 / 6 / 4, 128 < N <= 256:
# 16 / 12 / 8, N > 256: 8 / 6 / 4); N not a multiple of 64; without (AESMC) and with (PSVO) an upstream gradient
RING = [(obj, 2, 40, n, 4, dx, 1, 32, True, True) for obj in ("AESMC", "PSVO") for n in (40, 100, 200, 300) for dx in (2, 3, 4)]
# the short edge and lengths that are not a multiple of any ring depth (partial last window)
EDGES = [("AESMC", 2, 2, 64, 1, 2, 1, 32, True, True), ("PSVO", 2, 2, 300, 4, 4, 1, 32, True, True),
         ("AESMC", 2, 21, 64, 1, 3, 1, 32, True, True), ("PSVO", 2, 21, 100, 4, 4, 1, 32, True, True),
         ("SVO", 2, 23, 200, 1, 2, 1, 16, True, True), ("AESMC", 1, 37, 512, 1, 2, 1, 32, True, True)]
FILTER_BWD_CASES = BOOT_RESAMPLE + LARGE + RING + EDGES


@pytest.mark.parametrize("case", FILTER_BWD_CASES, ids=_ids)
def test_filter_backward_routes(built_lib, case):
    """every case under PSVO_TUNE_FILTER_BWD = 0, 1, 2 against one fp64 oracle run"""
    o = OracleOnce(case, seed=5)
    grads = []
    for setting in (0, 1, 2):
        o.hip([(_lib.PSVO_TUNE_FILTER_BWD, setting)], route=filter_route(case, setting))
        grads.append(o.grads())
    # the routes against each other: both are fp32 and differ in summation order only, so they agree far inside the oracle's
    # bar (which also carries fp32-against-fp64 rounding); a coefficient 1e-3 off at one step of the scan shows here
    spread = max(o.spread(g, grads[0]) for g in grads[1:])
    print("route spread %.3g of each tensor's largest oracle entry" % spread)
    assert spread <= ROUTE_RTOL, spread
    if case[0] == "PSVOwR":
        o.smc.check_exchange()


def test_filter_backward_misaligned_workspace(built_lib, monkeypatch):
    """A workspace that is not 16-byte aligned cannot hold the scan's float4 records: psvo_filter_backward must then run the
    persistent kernel (and not the scan on a null record pointer).  Only the psvo_filter_ws_floats-sized buffer comes back one
    float off its block; gradients against the oracle, the route from the profiler."""
    from psvo_amd import ops
    case = ("AESMC", 3, 9, 64, 1, 2, 1, 32, True, True)
    o = OracleOnce(case, seed=5)
    B, T, N, Dx, Dy = case[1], case[2], case[3], case[5], case[6]
    n_ws = _lib.load().psvo_filter_ws_floats(B, T, N, Dx, Dy)
    orig, seen = ops._empty, []

    def empty(*shape, **kw):
        if len(shape) == 1 and shape[0] == n_ws:
            seen.append(shape)
            buf = orig(n_ws + 1, **kw)
            return buf[1:]
        return orig(*shape, **kw)
    monkeypatch.setattr(ops, "_empty", empty)
    o.hip(route=filter_route(case, 1, aligned=False))
    assert seen, "the reverse filter's workspace was not allocated through ops._empty"
    assert filter_route(case, 1) == SCAN                     # (aligned, the same case takes the scan)
    monkeypatch.setattr(ops, "_empty", orig)
    o.hip(route=SCAN)


# ---------------------------------------------------------------------------------------------
# B2: psvo_filter_backward_cov under PSVO_TUNE_FILTER_BWD = 0 / 1
# ---------------------------------------------------------------------------------------------
COV_BOOT_RESAMPLE = [(c, e) for c, e in TP.COV_CASES if c[8] and c[0] != "IWAE"]


@pytest.mark.parametrize("case,extra", COV_BOOT_RESAMPLE, ids=_ids)
def test_cov_filter_backward_routes(built_lib, case, extra):
    """state-dependent scales: the bootstrap-and-resampling branch of filter_cov_bwd_kernel (switch 0) beside the scan"""
    o = OracleOnce(case, seed=7, **extra)
    for setting in (0, 1):
        o.hip([(_lib.PSVO_TUNE_FILTER_BWD, setting)], route=cov_route(case, setting), families=COV_FAMILIES)


@pytest.mark.parametrize("obj", ["PSVO", "PSVOwR", "SVO"])
def test_cov_filter_backward_persistent_long_sequence(built_lib, obj):
    """test_state_dependent_scales_long_sequence's T = 120 cases through filter_cov_bwd_kernel (switch 0)"""
    case = (obj, 2, 120, 24, 4, 2, 1, 32, True, True)
    o = OracleOnce(case, seed=13, **TP._COV)
    o.hip([(_lib.PSVO_TUNE_FILTER_BWD, 0)], route=COV_PERSISTENT, families=COV_FAMILIES)


# ---------------------------------------------------------------------------------------------
# B3: the other switches
# ---------------------------------------------------------------------------------------------
def _bsim_bwd_hs(names):
    """HS (last template argument) of every bsim_bwd_kernel instantiation that ran"""
    out = set()
    for n in _family(names, V1):
        m = re.search(r"%s<([^>]*)>" % V1, n)
        assert m, "cannot read the template arguments of %s" % n
        out.add(int(m.group(1).split(",")[-1]))
    return out


L2_CASES = [(c, e) for c, e in TP.DEPTH_CASES if c[0] == "PSVO"]


@pytest.mark.parametrize("case,extra", L2_CASES, ids=_ids)
def test_two_layer_split_chains(built_lib, case, extra):
    """PSVO_TUNE_L2_SPLIT = 0 / 1: the two-layer backward simulation with a chain on M or on 2 M lanes (HS = 2 where Dx = 2,
    2 M <= 64 and the problem is small, bsim_bwd_impl.h: bsim_geometry), forward and reverse kernels"""
    obj, B, T, N, M, Dx = case[:6]
    o = OracleOnce(case, seed=7, **extra)
    for split in (0, 1):
        hs = 2 if split and Dx <= 2 and 2 * M <= 64 else 1
        o.hip([(_lib.PSVO_TUNE_L2_SPLIT, split)],
              names_check=lambda names, hs=hs: _check_eq(_bsim_bwd_hs(names), {hs}, "HS of bsim_bwd_kernel"))


def _check_eq(got, want, what):
    assert got == want, "%s: %s, expected %s" % (what, got, want)


def _rows_bwd_rb(names):
    out = set()
    for n in _family(names, "rows_mlp_bwd_kernel"):
        m = re.search(r"rows_mlp_bwd_kernel<([^>]*)>", n)
        assert m, "cannot read the template arguments of %s" % n
        out.add(int(m.group(1).split(",")[-1]))
    return out


@pytest.mark.parametrize("case", [("PSVO", 2, 7, 16, 4, 2, 1, 32, True, True),       # 14 rows per hoisted MLP
                                  ("PSVO", 8, 160, 16, 4, 2, 1, 32, True, True)],   # 1280 rows
                         ids=_ids)
def test_rows_backward_block(built_lib, case):
    """PSVO_TUNE_ROWS_BWD = 16 / 64 rows per workgroup of psvo_rows_mlp_backward (the hoisted MLPs over T x B rows), below and
    above the automatic switch at 1024 rows"""
    o = OracleOnce(case, seed=9)
    for rb in (16, 64):
        o.hip([(_lib.PSVO_TUNE_ROWS_BWD, rb)], names_check=lambda names, rb=rb: _check_eq(_rows_bwd_rb(names), {rb}, "RB"))


@pytest.mark.parametrize("case", [("PSVO", 2, 9, 128, 16, 2, 1, 32, True, True), ("PSVO", 1, 6, 200, 8, 3, 1, 32, True, True)],
                         ids=_ids)
def test_bsim_backward_skew(built_lib, case):
    """PSVO_TUNE_SKEW = 50 / 100: start-up phase offsets between co-resident workgroups of the v2 reverse backward simulation"""
    o = OracleOnce(case, seed=17)
    for skew in (50, 100):
        o.hip([(_lib.PSVO_TUNE_SKEW, skew)], route=V2, families=(V1, V2))


# ---------------------------------------------------------------------------------------------
# B4: the BASELINE sequence lengths (C3: T = 400, Dx = 3; C5: T = 1000, Dx = 4), every gradient against the fp64 oracle
# ---------------------------------------------------------------------------------------------
RUNAWAY = 50.0      # bound on |ELBO| / (B T) asserted before any comparison (the seeds below give 3 - 4)


@pytest.mark.timeout(900)
def test_long_T_1000_dx4(built_lib):
    """PSVO, T = 1000, N = 64, M = 16, Dx = 4: C5's reverse backward simulation (v1 by default at Dx = 4) and v2 with its
    scratch spills, each with the persistent reverse filter (the default behind a backward simulation at N <= 256) and with
    the scan carrying the upstream gradient through its 8-step ring (125 wraps)"""
    case = ("PSVO", 1, 1000, 64, 16, 4, 1, 32, True, True)
    o = OracleOnce(case, seed=1, fhn=True, per_step_bound=RUNAWAY)
    for variant, want in ((-1, V1), (1, V2)):
        for fb in (1, 2):
            names = o.hip([(_lib.PSVO_TUNE_BSIM_BWD, variant), (_lib.PSVO_TUNE_FILTER_BWD, fb)],
                          route=filter_route(case, fb))
            assert_route(names, want, (V1, V2))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", [("PSVO", 1, 400, 128, 16, 3, 1, 32, True, True),
                                  ("PSVOwR", 1, 400, 128, 16, 2, 1, 32, True, True)], ids=_ids)
def test_long_T_400(built_lib, case):
    """C3's shape (PSVO, T = 400, Dx = 3: v2 with its accumulators in LDS, filter_bwd_lpp_kernel at Dx = 3) and the PSVOwR
    cluster ring over 400 steps"""
    o = OracleOnce(case, seed=1, fhn=True, per_step_bound=RUNAWAY)
    o.hip(route=filter_route(case, 1))
    if case[0] == "PSVOwR":
        o.smc.check_exchange()


@pytest.mark.timeout(900)
def test_long_T_1000_aesmc_n512(built_lib):
    """AESMC, T = 1000, N = 512, Dx = 4: C5's scan instantiation (fbs_scan_kernel<4, 4, 2, 4>) and, under switch 0,
    filter_bwd_kernel<4, 1, 32, 512> with its float atomics"""
    case = ("AESMC", 1, 1000, 512, 1, 4, 1, 32, True, True)
    o = OracleOnce(case, seed=1, fhn=True, per_step_bound=RUNAWAY)
    for fb in (1, 0):
        o.hip([(_lib.PSVO_TUNE_FILTER_BWD, fb)], route=filter_route(case, fb))
