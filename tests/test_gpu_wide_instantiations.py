"""Every template instantiation of the wide-observation filters (six compilations), of the static wide backward simulation and
of the particle forecast, one small problem each (tests/wide_instantiations.py is the table; DESIGN.md section 8 says why a
sampled suite does not have to meet a bad instantiation).

Each test is one case and
  1. asserts, from the profiler's kernel names, that exactly the instantiation the table names ran -- every kernel of the swept
     families that ran is one the case names, and every one it names ran;
  2. (filters, backward simulation) compares the teacher-forced forward values and every parameter gradient with the family's
     fp64 reference, then runs free and holds every in-kernel draw to the reference's inverse-CDF rule on the replayed weights
     (EDGE_TOL); adaptive forms: the decisions and the effective sample size as their families check them;
  3. (forecast) judges the four outputs by tests/test_gpu_forecast.py::_judge with its K_TOL as it stands.
Tolerances are the families' own, imported or, where they are literals of the families' assertions, stated once in
wide_instantiations.VALUE_TOL: X / Xanc / Xs / bwX 2e-4, logW / lse / flp / glp / Omega 5e-4 (rtol 1e-5 each), ELBO 1e-4 relative,
gradients 2e-3 of a tensor's largest entry + 1e-6 or K32 times the fp32 reference's own error (computed only where the first
clause fails).  tests/test_wide_instantiations_host.py holds every case's reference, alone, to a quarter of the value tolerances.
The worst figures are printed before anything is asserted (profiles/wide_instantiations.md records them).  Nothing is cached
across tests."""
import pytest
import torch

from oracle import psvo_oracle as O
from tests import helpers as Hh
from tests import wide_instantiations as WI
from tests.test_gpu_forecast import _cuda, _judge
from tests.test_gpu_instantiations import K32
from tests.test_gpu_large import EDGE_TOL
from tests.test_gpu_parity import _pairs

pytestmark = pytest.mark.gpu

_ids = lambda c: c.id


# ---- 1. which kernels ran --------------------------------------------------------------------------------------------------------
def _assert_kernels(c, names):
    ran = WI.family(names)
    print("%s: ran %s" % (c.id, sorted(ran)))
    missing = [w for w in c.kernels if not any(WI.same_kernel(r, w) for r in ran)]
    assert not missing, "the case did not launch %s; of the swept families it launched %s" % (sorted(missing), sorted(ran))
    other = [r for r in ran if not any(WI.same_kernel(r, w) for w in c.kernels)]
    assert not other, "another instantiation ran: %s (the case names %s)" % (sorted(other), sorted(c.kernels))


# ---- 2. values, draws, decisions, gradients --------------------------------------------------------------------------------------
def _hip_noise(p, teacher):
    """the reference's noise and what is forced (idx_f, idx_b, rs_f in its layouts) in the kernels' layout"""
    nz = Hh.noise_to_hip({**p.noise, **{k: v for k, v in teacher.items() if k in ("idx_f", "idx_b")}}, "cuda")
    if "idx_f" in nz:
        nz.pop("u_f", None)
    if "sel_b" in nz:
        nz.pop("u_b", None)
    if teacher.get("rs_f") is not None:
        nz["rs_f"] = teacher["rs_f"].to(torch.int32).contiguous().cuda()
    return nz


def _launch(p, nz, v_c=None):
    kw = {} if p.v is None else {"inputs": p.v.float().cuda() if v_c is None else v_c}
    return p.smc.get_log_ZSMC(p.obs.float().cuda(), None, noise=nz, **kw)


def _hip_values(log):
    filt = log["filter"]
    out = {"X_prevs": Hh.part_to_ref(filt["X"]), "X_ancestors": Hh.part_to_ref(filt["Xanc"]), "log_Ws": Hh.w_to_ref(filt["logW"]),
           "lse": filt["lse"].double().cpu(), "Xs": log["Xs"].double().cpu()}
    if "bsim" in log:
        bs = log["bsim"]
        out.update({"bw_Xs": Hh.part_to_ref(bs["bwX"]), "f_log_probs": Hh.w_to_ref(bs["flp"]),
                    "g_log_probs": Hh.w_to_ref(bs["glp"]), "bw_log_Omegas": Hh.w_to_ref(bs["Omega"])})
    return {k: v.detach() for k, v in out.items()}


def _assert_values(tag, z, log, r):
    """allclose(atol, rtol 1e-5) on every compared quantity and the ELBO to 1e-4 relative; error / bound printed first"""
    want, got = WI.value_rows(r.log), _hip_values(log)
    assert set(want) <= set(got)
    share = {}
    for k, a in want.items():
        assert torch.isfinite(got[k]).all(), k
        share[k] = float(((got[k] - a).abs() / (WI.VALUE_TOL[k] + WI.RTOL * a.abs())).max())
    share["ELBO"] = abs(float(z) - float(r.z)) / (WI.ELBO_RTOL * abs(float(r.z)))
    worst = max(share, key=share.get)
    print("%s: value error / bound, worst %s %.3f; all %s" % (tag, worst, share[worst],
                                                            " ".join("%s %.3f" % kv for kv in sorted(share.items()))))
    assert abs(float(r.z)) >= 1.0
    assert share[worst] <= 1.0, share


def _draw_stats(draws):
    n = off = 0
    worst = 0.0
    for log_W, u, idx in draws:
        d = O.draw_distance(log_W, u, idx)
        n += d.numel()
        off += int((d > 0).sum())
        worst = max(worst, float(d.max()))
    return n, off, worst


def _ess_margin(c):
    if c.comp == "ad":
        from tests.test_gpu_wobs_adaptive import MARGIN
        return MARGIN
    if c.comp == "msad":
        from tests.test_gpu_missing_adaptive import MARGIN
        return MARGIN
    return None


def _assert_decisions(tag, c, filt, ref_log, forced):
    """the adaptive forms: rs_out is what was forced / what the rule says on the reference's ESS; ESS within the family's margin"""
    from tests import adaptive_reference as AR
    rs, ess = filt["rs"], filt["ess"]
    assert rs.dtype == torch.int32 and rs.shape == (c.T, c.B) and bool(((rs == 0) | (rs == 1)).all())
    assert torch.isfinite(ess).all() and float(ess.min()) >= 1.0 - 1e-3 and float(ess.max()) <= c.N * (1 + 1e-5)
    rs_hip = rs.cpu() != 0
    assert torch.equal(rs_hip, forced != 0), "decisions differ from the reference's"
    assert 0 < int(rs_hip.sum()) < c.T * c.B
    gap = float(((ess.double().cpu() - ref_log["ess"]).abs() / c.N).max())
    margin = _ess_margin(c)
    print("%s: resampled %d of %d; |ESS - ESS_ref| / N max %.3e (margin %s)" % (
        tag, int(rs_hip.sum()), c.T * c.B, gap, "%.3e" % margin if margin else "none: forced decisions"))
    if margin is not None:
        assert gap <= margin, "ESS off by %.3e N (margin %.3e N)" % (gap, margin)
        assert torch.equal(rs_hip, AR.decide(ref_log["ess"], c.tau, c.N))


def _assert_gradients(p, teacher, v_c):
    """every parameter tensor (the input rows W1[Dx:] on their own, and d v, on the input forms) against fp64 autograd of the
    reference: 2e-3 of the largest entry + 1e-6, or K32 times the fp32 reference's own error on that tensor"""
    c, model = p.case, p.model
    r = WI.evaluate(p, teacher=teacher, grad=True)

    def rows_of(P, dv, got):
        rows = {}
        if dv is not None:
            rows["inputs"] = (None if not got else v_c.grad.double().cpu(), dv.double())
        for name, q, ref in _pairs(model, P):
            g = torch.zeros_like(ref) if q.grad is None else q.grad.detach().double().cpu()
            want = (torch.zeros_like(ref) if ref.grad is None else ref.grad).double()
            rows[name] = (g, want)
            if c.Di and name in ("q1.W0", "f.W0"):       # the input rows must not hide behind a larger state block
                rows[name + "[Dx:]"] = (g[c.Dx:], want[c.Dx:])
        return rows
    rows = rows_of(r.P, r.dv, True)
    fig = {}
    for name, (g, want) in rows.items():
        assert torch.isfinite(g).all(), name
        fig[name] = (float((g - want).abs().max()), max(float(want.abs().max()), 1e-6))
    worst = max(fig, key=lambda n: fig[n][0] / fig[n][1])
    print("%s: worst gradient error / largest entry: %s %.3e (bound 2e-3)" % (c.id, worst, fig[worst][0] / fig[worst][1]))
    over = [n for n, (e, s) in fig.items() if e > 2e-3 * s + 1e-6]
    if over:
        r32 = WI.evaluate(p, torch.float32, teacher, grad=True)
        rows32 = rows_of(r32.P, r32.dv, False)
        err32 = {n: float((rows32[n][1] - rows[n][1]).abs().max()) for n in over}
        print("%s: over the first clause (tensor, error, largest entry, fp32 reference's own error): %s"
              % (c.id, [(n,) + fig[n] + (err32[n],) for n in over]))
        bad = [(n,) + fig[n] + (err32[n],) for n in over if fig[n][0] > K32 * err32[n]]
        assert not bad, "gradient mismatch (name, max abs err, own scale, fp32 reference's own err): %s" % bad
    names = set(fig)
    assert {"q1.W0", "q1.b0", "g.W0", "g.b0", "g.Wmu", "g.bmu"} <= names and ("g.sigma" in names) == (c.emission == WI.GAUSS)
    assert ("f.W0" in names) == (not c.boot) and ("q2.W0" in names) == c.two_q
    for n in names:          # no scale is compared as 0 == 0 (wide_instantiations.LIFT keeps every one off its floor)
        assert not n.endswith(".sigma") or fig[n][1] > 1e-6, n
    if c.Di:
        assert {"inputs", "q1.W0[Dx:]"} <= names and ("f.W0[Dx:]" in names) == (not c.boot)
        assert fig["inputs"][1] > 1e-6 and fig["q1.W0[Dx:]"][1] > 1e-6
    if c.group == "c":
        for prefix in ("q1_inv.", "BSim_q2.", "BSim_q_init."):
            assert any(n.startswith(prefix) for n in names), prefix
    if p.mask is not None and p.mask[2] is not None:          # a never-observed output keeps exactly zero gradient
        e = p.mask[2]
        for name, q, ref in _pairs(model, r.P):
            if name in ("g.Wmu", "g.bmu", "g.sigma"):
                g = q.grad.detach().cpu()
                col, rcol = (g[e], ref.grad[e]) if g.dim() == 1 else (g[:, e], ref.grad[:, e])
                assert bool((col == 0.0).all()) and bool((rcol == 0.0).all()), (name, col)


def _sweep(c):
    p = WI.problem(c, "cuda")
    adaptive = c.comp in WI.ADAPTIVE and c.group != "c"
    r64, teacher = WI.reference_teacher(p)

    # teacher-forced, forward and reverse, under the profiler
    p.model.zero_grad(set_to_none=True)
    v_c = None if p.v is None else p.v.float().cuda().requires_grad_(True)

    def step():
        z, log = _launch(p, _hip_noise(p, teacher), v_c)
        z.backward()
        return z.detach(), log
    (z, log), names = Hh.kernel_names(step)
    _assert_kernels(c, names)
    d = p.smc._desc(c.M)
    assert (d.Dx, d.H, d.N, d.Dy, d.M, d.emission) == (c.Dx, c.H, c.N, c.Dy, c.M, WI.EMISSION_CODE[c.emission])
    _assert_values(c.id + " forced", z, log, r64)
    if "idx_f" in teacher:
        assert torch.equal(log["filter"]["idx"].permute(0, 2, 1).cpu().long(), teacher["idx_f"])
    if c.group == "c":
        bs = log["bsim"]
        assert set(bs) == {"score", "bwX", "flp", "glp", "Omega", "sel"}
        assert torch.equal(bs["sel"].permute(0, 2, 1).cpu().long(), r64.log["idx_b"])
        ref = r64.log
        score_ref = (ref["f_log_probs"] + ref["g_log_probs"] - ref["bw_log_Omegas"]).sum(0).permute(1, 0)       # (B, N)
        e_score = float((bs["score"].detach().double().cpu() - score_ref).abs().max())
        print("%s: score max abs err %.3e" % (c.id, e_score))
        assert e_score <= 2e-3 + 1e-5 * float(score_ref.abs().max())
    if p.mask is not None:
        assert torch.equal(log["missing"].cpu(), torch.isnan(p.obs)) and torch.equal(log["missing"].cpu(), p.mask[0])
    if adaptive:
        _assert_decisions(c.id + " forced", c, log["filter"], r64.log, teacher["rs_f"])
        assert torch.equal(log["ess"], log["filter"]["ess"].t()) and torch.equal(log["resampled"], (log["filter"]["rs"] != 0).t())
    _assert_gradients(p, teacher, v_c)

    # free running: the kernels' own draws (and decisions), the reference replayed with them
    first = {"rs_f": teacher["rs_f"]} if c.comp == "inad" else {}
    with torch.no_grad():
        z, log = _launch(p, _hip_noise(p, first))
    torch.cuda.synchronize()
    filt = log["filter"]
    if r64.log.get("idx_f") is None:          # IWAE: no resampling, every particle its own ancestor
        n = torch.arange(c.N, dtype=torch.int32, device="cuda")
        assert torch.equal(filt["idx"], n.expand_as(filt["idx"]))
        _assert_values(c.id + " free", z, log, r64)
        return
    hip = {"idx_f": filt["idx"].permute(0, 2, 1).cpu().long()}
    if c.group == "c":
        hip["idx_b"] = log["bsim"]["sel"].permute(0, 2, 1).cpu().long()
    if adaptive:
        hip["rs_f"] = filt["rs"].cpu().long()
    rep = WI.evaluate(p, teacher=hip)
    draws, off, worst = _draw_stats(rep.draws)
    differ = int((hip["idx_f"] != r64.log["idx_f"]).sum()) + (int((hip["idx_b"] != r64.log["idx_b"]).sum()) if c.group == "c" else 0)
    print("%s free: draws %d, off their interval %d (worst edge distance %.3e), differing from the free reference %d"
          % (c.id, draws, off, worst, differ))
    assert draws > 0 and worst <= EDGE_TOL, "a draw that is not on a CDF edge"
    if adaptive:
        _assert_decisions(c.id + " free", c, filt, rep.log, r64.log["rs_f"])
    _assert_values(c.id + " free", z, log, rep)


@pytest.mark.parametrize("c", WI.GROUP_A, ids=_ids)
def test_every_wide_filter_instantiation(built_lib, c):
    _sweep(c)


@pytest.mark.parametrize("c", WI.GROUP_B, ids=_ids)
def test_the_lds_largest_corner(built_lib, c):
    """Dx 4, H 64, N 512, Dy 32 with its own f: the most dynamic LDS a wide filter can ask for, in every compilation"""
    _sweep(c)


@pytest.mark.parametrize("c", WI.GROUP_C, ids=_ids)
def test_every_static_wide_bsim_instantiation(built_lib, c):
    """(Dx, H, M, CNT) of bsim_wobs_fwd_kernel / bsim_wobs_bwd_kernel through PSVO, as
    tests/test_gpu_missing_bsim.py::test_every_instantiation sweeps the missing form; filter_bwd_wobs_kernel<.., EXT = true> runs
    behind them"""
    _sweep(c)


# ---- 3. the forecast -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", WI.GROUP_D, ids=_ids)
def test_every_forecast_instantiation(built_lib, f):
    from psvo_amd import ops
    from tests import forecast_reference as R
    c = WI.forecast_case(f)
    desc = ops.make_desc(f.B, f.T, f.N, 1, f.Dx, f.Dy, f.H, emission=f.emission)
    a = {k: _cuda(c[k]) for k in ("f", "g", "sig_f", "sig_g", "X", "logW", "obs", "eps")}
    kw = {"plain": {}, "missing": dict(missing=True), "input": dict(hb_f=None if f.form != "input" else c["hb_f"].cuda())}[f.form]

    def launch():
        return ops.particle_forecast(desc, f.K, a["f"], a["g"], a["sig_f"], a["sig_g"], a["X"], logW=a["logW"], obs=a["obs"],
                                     eps=a["eps"], **kw)
    out, names = Hh.kernel_names(launch)
    _assert_kernels(f, names)
    assert set(out) == set(R.KEYS) and out["lpd"].shape == (f.K + 1, f.T, f.B)
    assert out["ymean"].shape == out["yvar"].shape == (f.K + 1, f.T, f.B, f.Dy) and out["xmean"].shape == (f.K + 1, f.T, f.B, f.Dx)
    _judge(f.id, out, c)                                      # (figures first)
    lpd = out["lpd"].cpu()
    assert bool((lpd[~R.valid_mask(f.T, f.K)] == 0).all())    # exactly 0 where t + k >= T
    assert bool((lpd[~c["valid"]] == 0).all())                # ... and, missing forms, on target rows with nothing observed
    assert bool(c["valid"].any()) and f.gaps == bool(torch.isnan(c["obs"]).any())
    assert (out["yvar"] > 0).all()
