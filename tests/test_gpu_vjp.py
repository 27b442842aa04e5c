"""Every reverse route under non-uniform upstream gradients: the vector-Jacobian product of each autograd node against fp64
autograd of the oracle (tests/vjp_reference.py holds the cotangents, the surrogate, the cases and the comparison).

The ELBO hands the filter-only reverse kernels d lse[t, b] = 1 / B, the PSVOwR reverse kernels d lseW[t, b] = 1 / B and the PSVO
ones a positive softmax over the chains; under those a read of d lse[b], [0], [t], [b T + t] or [(t - 1) B + b] is exactly right, and
so is a cross-sequence fold that pairs sequence b's cotangent with another sequence's rows.  Here every cotangent is signed,
N(0, 1) times 1 + b, or one-hot at (t0, B - 1); B = 3 and T = 5 make t B + b, b T + t and b differ.  Indices (and, on the adaptive
routes, mixed resampling decisions) are teacher-forced; routes are chosen with helpers.tuning only.

The test id names the route: groups (a) plain reverse filter with d lse, (b) with d lse + d Fm + d logW, (c) state-dependent
scales, (d) adaptive, (e) the wide-observation kernels in their Gaussian and count forms, (f) the reverse backward simulations
with the reverse filter behind them, (g) PSVOwR, (h) one-hot cotangents, (i) the input-driven filter (FLAGS.Di), whose input rows
W1[Dx:] and d v per sequence are compared besides, (j) the same under adaptive resampling, (k) PSVO on wide observations
(FLAGS.BSim_wide_obs): the static reverse backward simulation with the _ext reverse filter behind it.  140 cases, 6.3 s on
one MI355X (113 cases in 5.8 s before groups (i)-(k)).  Rule: error <= 2e-3 x the reference tensor's largest
entry + 1e-6, else <= K32 x the fp32 oracle's own error on that tensor; each case prints its worst error / largest entry and
which clause decided (profiles/vjp_cotangents.md records them).
"""
import pytest
import torch

from tests import vjp_reference as V
from tests.test_gpu_parity import _pairs

pytestmark = pytest.mark.gpu

# the kernel a route must launch (a word of the kernel's name, from torch.profiler), where the case is there for a kernel
# that the default dispatch would not pick: a case that silently takes another route proves nothing
KERNEL_OF = {
    "fbs_scan_1_1": "fbs_scan_kernel", "fbs_scan_1_2": "fbs_scan_kernel", "fbs_scan_4_1": "fbs_scan_kernel",
    "fbs_scan_4_2": "fbs_scan_kernel", "fbs_scan_ext": "fbs_scan_kernel", "fbs_scan_ext_default": "fbs_scan_kernel",
    "filter_bwd_lpp": "filter_bwd_lpp_kernel", "filter_bwd_lpp_ext": "filter_bwd_lpp_kernel",
    "filter_bwd_persistent": "filter_bwd_kernel", "filter_bwd_persistent_atomics": "filter_bwd_kernel",
    "filter_bwd_persistent_deterministic": "filter_bwd_kernel", "filter_bwd_persistent_ext": "filter_bwd_kernel",
    "filter_cov_bwd_nonbootstrap": "filter_cov_bwd_kernel", "filter_cov_bwd_persistent": "filter_cov_bwd_kernel",
    "filter_cov_bwd_persistent_deterministic": "filter_cov_bwd_kernel",
    "filter_cov_bwd_nonbootstrap_deterministic": "filter_cov_bwd_kernel", "fcs_scan": "fcs_scan_kernel",
    "filter_bwd_lpp_ad": "filter_bwd_lpp_ad_kernel", "filter_bwd_ad_persistent": "filter_bwd_ad_kernel",
    "filter_wobs_input": ("filter_bwd_wobs_in_kernel", "mlp_wgrad_rowbias_kernel"),
    "filter_wobs_input_adaptive": "filter_bwd_wobs_inad_kernel",
    "bsim_wobs_static": ("bsim_wobs_bwd_kernel", "filter_bwd_wobs_kernel"),
}


def _run(case):
    from tests import helpers as Hh
    from tests.test_gpu_variants import _family
    p = V.setup(case, "cuda")
    cots = V.cotangents_of(case)
    P, teacher, ref_outs = V.oracle_vjp(p, cots)                          # fp64, free-running: its draws become the teacher
    want = KERNEL_OF.get(case.route)
    if want is not None and case.hot is None:
        (outs, dv), names = Hh.kernel_names(lambda: V.product_vjp(p, cots, teacher))
        for kernel in (want,) if isinstance(want, str) else want:
            assert _family(names, kernel), "%s did not run; device kernels: %s" % (kernel, sorted(names))
    else:
        outs, dv = V.product_vjp(p, cots, teacher)
    for k in cots:                  # the forward values the cotangents weigh, at the suite's tolerances
        atol = 2e-4 if k in ("Fm", "Fs") else 2e-3 if k == "score" else 5e-4
        assert torch.allclose(outs[k].double().cpu(), ref_outs[k], atol=atol, rtol=1e-5), k
    fp32 = []                       # the fp32 oracle under the same surrogate, run once and only when a tensor needs it

    def yardstick():
        if not fp32:
            fp32.append(V.oracle_vjp(p, cots, torch.float32, teacher)[0])
        return fp32[0]
    report = V.compare(p, P, yardstick)
    if case.family in V.INPUT:      # the input rows W1[Dx:] on their own and d v per sequence, exact zeros held to ATOL alone
        V.compare_inputs(p, P, dv, yardstick)
    if p.e_never is not None:       # the never-observed output keeps exactly zero gradient under the random cotangent too
        seen = 0
        for name, par, ref in _pairs(p.model, P):
            if name in ("g.Wmu", "g.bmu", "g.sigma") and par.grad is not None:
                g = par.grad.detach().cpu()
                col = g[p.e_never] if g.dim() == 1 else g[:, p.e_never]
                assert bool((col == 0.0).all()), (name, col)
                seen += 1
        assert seen >= 2
    return report


def _ids(c):
    return c.id


@pytest.mark.parametrize("case", V.A_CASES, ids=_ids)
def test_a_plain_filter_dlse(built_lib, case):
    _run(case)


@pytest.mark.parametrize("case", V.B_CASES, ids=_ids)
def test_b_plain_filter_all_cotangents(built_lib, case):
    _run(case)


@pytest.mark.parametrize("case", V.C_CASES, ids=_ids)
def test_c_state_dependent_scales(built_lib, case):
    _run(case)


@pytest.mark.parametrize("case", V.D_CASES, ids=_ids)
def test_d_adaptive_filter(built_lib, case):
    _run(case)


@pytest.mark.parametrize("case", V.E_CASES, ids=_ids)
def test_e_wide_observation_kernels(built_lib, case):
    _run(case)


@pytest.mark.parametrize("case", V.F_CASES, ids=_ids)
def test_f_backward_simulation(built_lib, case):
    _run(case)


@pytest.mark.parametrize("case", V.G_CASES, ids=_ids)
def test_g_psvowr(built_lib, case):
    from psvo_amd import _lib
    blocks = _lib.load().psvo_bsimwr_blocks(V.B, case.N, case.M)
    want = {"psvowr_bwd_one_member": 1, "psvowr_bwd_cluster2": 2, "psvowr_bwd_cluster4": 4}.get(case.route)
    assert want is None or blocks == want, (blocks, want)
    _run(case)


@pytest.mark.parametrize("case", V.I_CASES, ids=_ids)
def test_i_input_driven_filter(built_lib, case):
    _run(case)


@pytest.mark.parametrize("case", V.J_CASES, ids=_ids)
def test_j_input_driven_adaptive_filter(built_lib, case):
    _run(case)


@pytest.mark.parametrize("case", V.K_CASES, ids=_ids)
def test_k_wide_backward_simulation(built_lib, case):
    _run(case)


@pytest.mark.parametrize("case", V.H_CASES, ids=_ids)
def test_h_one_hot(built_lib, case):
    _run(case)
