"""tests/vjp_reference.py on the CPU: the oracle side of the vector-Jacobian tests against what is already trusted, and the CPU
pre-check of every case of tests/test_gpu_vjp.py (no GPU is touched).

  * a constant cotangent 1 / B (PSVO: softmax(score) / B) makes the surrogate's gradients those of the ELBO, which
    tests/test_gpu_parity.py::_oracle_grads differentiates directly: equal to 1e-12 of each tensor's largest entry; on the input
    families the trusted side is exo_reference.grads / exo_adaptive_reference.grads, d v included, which ties the adapter
    (vjp_reference.InputOracle) to them;
  * a one-hot c_lse at (t0, b0) gives the fp64 autograd gradient of logsumexp(log_Ws, 1)[t0, b0] taken directly; its d v is zero
    outside sequence b0 and from step t0 on;
  * on every case the fp32 oracle's own gradients (the yardstick of the second clause) are finite and stay inside the first
    clause on at least three quarters of the tensors, so the model seed is fit for fp32 and a failure on the GPU is the kernel's.
"""
import math

import pytest
import torch

from tests import exo_adaptive_reference as XA
from tests import exo_reference as ER
from tests import vjp_reference as V
from tests.test_gpu_parity import _oracle_grads, _pairs

ELBO_CASES = [V.Case("elbo", "SVO", 17, 2, 1), V.Case("elbo", "AESMC", 17, 3, 2, boot=False),
              V.Case("elbo", "IWAE", 17, 2, 1, two_q=False), V.Case("elbo", "PSVOwR", 8, 2, 1, cots=("lseW",)),
              V.Case("elbo", "PSVO", 17, 2, 1, cots=("score",)),
              V.Case("elbo", "SVO", 17, 3, 2, family="input", boot=False, flags=dict(Di=2)),
              V.Case("elbo", "AESMC", 17, 2, 1, family="input_adaptive", flags=dict(Di=3)),
              V.Case("elbo", "PSVO", 17, 2, 3, family="wide", cots=("score",), flags=dict(BSim_wide_obs=True))]


def _close(model, P, P_ref, rel):
    for name, err, scale in V.grad_rows(model, P, P_ref):
        assert err <= rel * scale, (name, err, scale)


def test_cotangents_are_signed_seeded_and_scaled_per_sequence():
    shapes = {"lse": (V.T, V.B), "Fm": (V.T, V.B, 2, 40), "score": (V.B, 4000)}
    a, b = V.cotangents(shapes, 3), V.cotangents(shapes, 3)
    other = V.cotangents(shapes, 4)
    for k, s in shapes.items():
        assert a[k].dtype == torch.float32 and tuple(a[k].shape) == s and torch.equal(a[k], b[k]) and not torch.equal(a[k], other[k])
        assert bool((a[k] < 0).any()) and bool((a[k] > 0).any())
    # N(0, 1) times 1 + b along the sequence axis: the root mean square per sequence, 4000 draws each
    rms = a["score"].double().pow(2).mean(1).sqrt()
    for b_ in range(V.B):
        assert abs(float(rms[b_]) / (1.0 + b_) - 1.0) < 5.0 / math.sqrt(2 * 4000), (b_, float(rms[b_]))
    h = V.one_hot((V.T, V.B), (1, 2))
    assert h.dtype == torch.float32 and float(h.sum()) == 1.0 and float(h[1, 2]) == 1.0


def test_forced_decisions_and_mask():
    rs = V.forced_decisions()
    assert tuple(rs.shape) == (V.T, V.B)
    for b in range(V.B):            # every sequence both keeps and resamples
        assert 0 < int(rs[:, b].sum()) < V.T
    assert sum(1 for t in range(V.T) if 0 < int(rs[t].sum()) < V.B) >= V.T - 1
    for Dy in (1, 2, 3, 10):
        miss, t_all, e_never = V.mask(Dy, 5)
        assert bool(miss[:, t_all].all()) and bool(miss[V.B - 1, V.T - 2:].all()) and (e_never is None) == (Dy == 1)
        assert e_never is None or bool(miss[:, :, e_never].all())
        assert not bool(miss.all(-1)[:V.B - 1, [t for t in range(V.T) if t != t_all]].all())


def test_every_route_of_the_issue_is_a_case():
    routes = {c.route for c in V.CASES}
    for r in ("fbs_scan_1_1", "fbs_scan_1_2", "fbs_scan_4_1", "fbs_scan_4_2", "filter_bwd_lpp", "filter_bwd_persistent",
              "filter_bwd_persistent_atomics", "filter_bwd_persistent_deterministic", "filter_bwd_nonbootstrap", "filter_bwd_no_q2",
              "filter_bwd_iwae", "filter_bwd_two_layers", "fbs_scan_ext", "filter_cov_bwd_persistent", "fcs_scan",
              "filter_bwd_lpp_ad", "filter_bwd_ad_persistent", "filter_wobs_static", "filter_wobs_adaptive", "filter_wobs_missing",
              "filter_wobs_missing_adaptive", "filter_wobs_missing_ext", "bsim_bwd_default", "bsim_bwd_two_layers", "bsim_cov",
              "bsim_cov_ws_deterministic", "bsim_wobs_missing", "psvowr_bwd_one_member", "psvowr_bwd_cluster2",
              "psvowr_bwd_cluster4", "bsimwr_cov", "bsimwr_cov_ws_deterministic", "filter_wobs_input",
              "filter_wobs_input_adaptive", "bsim_wobs_static") + tuple("bsim_bwd_variant%d" % v for v in range(5)):
        assert r in routes, r
    for fam in ("wide", "wide_adaptive", "missing", "missing_adaptive", "missing_bsim"):     # Gaussian and count form each
        assert {c.emission for c in V.E_CASES if c.family == fam} >= {V.GAUSS, V.COUNT}, fam
    for fam, group in (("input", V.I_CASES), ("input_adaptive", V.J_CASES)):     # ... and so do the input families
        assert {c.family for c in group} == {fam} and {c.emission for c in group} == {V.GAUSS, V.COUNT}, fam
        assert all(c.flags["Di"] >= 1 for c in group) and any(c.flags["Di"] == c.H for c in group), fam
        assert {f for c in group for f in V.H_CASES if f.route == c.route and f.family == fam}, fam
    assert any(c.flags.get("missing_obs") for c in V.I_CASES)
    assert {(c.obj, c.family) for c in V.K_CASES} == {("PSVO", "wide")} and all(c.flags == dict(BSim_wide_obs=True) for c in V.K_CASES)
    assert {c.emission for c in V.K_CASES} == {V.GAUSS, V.UNIT, V.COUNT} and all(3 <= c.Dy <= 32 for c in V.K_CASES)
    assert any(set(c.cots) == {"score", "lse", "Fm", "logW"} for c in V.K_CASES)
    assert (len(V.I_CASES), len(V.J_CASES), len(V.K_CASES)) == (8, 5, 8)
    assert len(V.H_CASES) == 21 and {c.hot for c in V.H_CASES} == {(0, V.B - 1), (1, V.B - 1), (V.T - 1, V.B - 1)}
    assert 130 <= len(V.CASES) <= 150


@pytest.mark.parametrize("case", ELBO_CASES, ids=lambda c: c.id)
def test_constant_cotangent_gives_the_elbo_gradients(case):
    p = V.setup(case)
    with torch.no_grad():
        _, o, _, log = V.oracle_run(p)
        outs = V.oracle_outputs(o, log, case.family)
    teacher = V.teacher_of(log)
    (name,) = case.cots
    if name == "score":             # d [mean_b (logsumexp_n score - log N)] / d score = softmax_n(score) / B
        c = torch.softmax(outs["score"], 1) / V.B
    else:                           # d [mean_b sum_t lse] / d lse = 1 / B (PSVOwR: lseW, the - T log N is a constant)
        c = torch.full((V.T, V.B), 1.0 / V.B, dtype=torch.float64)
    P, _, _ = V.oracle_vjp(p, {name: c}, teacher=teacher)
    if case.family in V.INPUT:      # the references' own ELBO gradients, d v included: what ties the adapter to them
        if case.family == "input":
            _, P_elbo, dv = ER.grads(p.model, p.FLAGS, case.obj, p.obs, p.inputs, p.noise, teacher)
        else:
            _, P_elbo, dv = XA.grads(p.model, p.FLAGS, case.obj, p.obs, p.inputs, p.noise, {**teacher, "rs_f": p.forced}, ess_frac=V.TAU)
        assert float(dv.abs().max()) > 0 and float((P["inputs"].grad - dv).abs().max()) <= 1e-12 * float(dv.abs().max())
    else:
        _, P_elbo = _oracle_grads(p.model, p.FLAGS, case.obj, p.obs, p.noise, teacher)
    assert len(_pairs(p.model, P)) >= 17
    _close(p.model, P, P_elbo, 1e-12)


@pytest.mark.parametrize("case", [c for c in V.H_CASES if "lse" in c.cots], ids=lambda c: c.id)
def test_one_hot_cotangent_is_the_gradient_of_one_entry(case):
    p = V.setup(case)
    t0, b0 = case.hot
    P, teacher, _ = V.oracle_vjp(p, V.cotangents_of(case))
    P2, o, _, log = V.oracle_run(p, teacher=teacher)
    torch.logsumexp(log["log_Ws"], 1)[t0, b0].backward()
    _close(p.model, P, P2, 1e-12)
    assert any(s > 1e-6 for _, _, s in V.grad_rows(p.model, P, P2))
    if case.family in V.INPUT:      # d v of the one entry: nothing outside sequence b0, nothing from step t0 on (v[t] first
        dv = P["inputs"].grad       # meets the state at step t + 1), and what is left is autograd's own
        direct = torch.zeros_like(dv) if o.v.grad is None else o.v.grad
        assert float((dv - direct).abs().max()) <= 1e-12 * max(float(direct.abs().max()), 1e-6)
        keep = torch.zeros(V.B, V.T, dtype=torch.bool)
        keep[b0, :t0] = True
        assert bool((dv[~keep] == 0).all()) and (t0 == 0 or float(dv[b0, t0 - 1].abs().max()) > 0)


def _oracle_key(c):
    """what the oracle side of a case depends on (the tuning switches and the route's name do not enter)"""
    return (c.obj, c.N, c.Dx, c.Dy, c.family, c.cots, c.M, c.H, c.boot, c.two_q, c.emission, c.layers, c.seed, c.hot,
            tuple(sorted(c.flags.items())))


_UNIQUE = list({_oracle_key(c): c for c in V.CASES}.values())


@pytest.mark.parametrize("case", _UNIQUE, ids=lambda c: c.id)
def test_seed_is_fit_for_fp32(case):
    """the CPU pre-check of a case's model seed: the yardstick is finite, and fp32 arithmetic itself holds the first clause
    on at least three quarters of the tensors"""
    p = V.setup(case)
    cots = V.cotangents_of(case)
    P, teacher, outs = V.oracle_vjp(p, cots)
    for k in cots:
        assert tuple(outs[k].shape) == tuple(cots[k].shape) and bool(torch.isfinite(outs[k]).all()), k
    P32, _, _ = V.oracle_vjp(p, cots, torch.float32, teacher)
    rows = V.grad_rows(p.model, P32, P)
    if case.family in V.INPUT:      # the input rows and the d v blocks: in the share, and held to the GPU test's own assertions
        rows = rows + V.compare_inputs(p, P, None, lambda: P32, subject=P32)
    assert all(math.isfinite(e) and math.isfinite(s) for _, e, s in rows)
    assert any(s > 1e-6 for _, _, s in rows)
    assert V.fp32_share_over(rows) <= 0.25, [(n, e, s) for n, e, s in rows if not e <= V.RTOL * s + V.ATOL]
    if p.e_never is not None:       # the never-observed output has exactly zero gradient under a random cotangent too
        for name, _, ref in _pairs(p.model, P):
            if name in ("g.Wmu", "g.bmu", "g.sigma") and ref.grad is not None:
                col = ref.grad[p.e_never] if ref.grad.dim() == 1 else ref.grad[:, p.e_never]
                assert bool((col == 0.0).all()), name
