"""The CPU half of the wide-family instantiation sweep (tests/wide_instantiations.py is the table,
tests/test_gpu_wide_instantiations.py the GPU half).

  * The ledger: the kernel symbols of the built library that belong to the swept families are exactly the kernels the table
    promises to launch.  An instantiation added without a sweep case, or a dispatch line removed while its case stays, fails here
    and is named.
  * The reference alone: on every sweep case with a model behind it the family's reference, evaluated in fp32 on the CPU with the
    fp64 run's indices (and decisions), stays within a quarter of each value tolerance the GPU test applies, so that three
    quarters of each bound are the kernel's (another sum order, v_exp_f32).  A case that fails is given another seed or calmer
    output layers in wide_instantiations.MOVED, never a wider tolerance.
  * Adaptive forms: the fp64 reference's free-running decisions hold a kept and a resampled step, no closer to the threshold than
    100 x the GPU's ESS margin, and the fp32 reference's ESS stays within the family's recorded ESS_GAP32 figure, which that
    margin is built on.  (Input + adaptive: the family forces a fixed mixed pattern; the pattern holds both.)
  * Missing forms: every case holds a step with nothing observed and, where a row has more than one entry, a partly observed row.
"""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest
import torch

from tests import wide_instantiations as WI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ids = lambda c: c.id


def library_kernels(lib):
    """the demangled names of the device functions of every gfx950 code object in `lib`, from the symbol tables alone"""
    spec = importlib.util.spec_from_file_location("exec_restore_check", os.path.join(ROOT, "tools", "exec_restore_check.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        for co in chk.code_objects(lib, tmp):
            out = subprocess.run([chk.LLVM + "/llvm-objdump", "--syms", "--demangle", co], check=True, capture_output=True,
                                 text=True).stdout
            for line in out.splitlines():
                m = re.match(r"^[0-9a-f]+\s+\S+\s+F\s+\.text\s+[0-9a-f]+\s+(?:\.\w+\s+)?(.*)$", line)
                if m:
                    names.add(m.group(1))
    return names


def test_ledger(built_lib):
    names = library_kernels(built_lib)
    assert len(names) > 1000, "expected the whole kernel set, found %d" % len(names)
    lib, table = WI.family(names), WI.promised()
    count = lambda s, word: sum(1 for k in s if word in k[0])
    print("ledger: library / table -- wide filters %d / %d, static bsim %d / %d, missing bsim %d / %d, forecast %d / %d" % (
        count(lib, "filter_"), count(table, "filter_"), count(lib, "wbs::"), count(table, "wbs::"),
        count(lib, "wbs_ms::"), count(table, "wbs_ms::"), count(lib, "forecast"), count(table, "forecast")))
    assert not lib - table, "kernels of the library that no sweep case launches: %s" % sorted(lib - table)
    assert not table - lib, "kernels the table promises that the library does not hold: %s" % sorted(table - lib)
    assert all(WI.FAMILY.match(k[0]) for k in table)


def test_norm_reads_both_spellings():
    a = WI.norm("void psvo::wobs::filter_bwd_wobs_msad_kernel<3, 16, false, true>(psvo::wobs::BwdArgsAd)")
    assert a == ("filter_bwd_wobs_msad_kernel", (3, 16, 0, 1))
    assert WI.norm("psvo::wobs::filter_bwd_wobs_msad_kernel<3,16,(bool)0,(bool)1>") == a
    b = WI.norm("void psvo::forecast_kernel<3, 64, 0, true, false>(std::conditional<false, psvo::ForecastArgsIn, "
                "psvo::ForecastArgs>::type)")
    assert b == ("forecast_kernel", (3, 64, 0, 1, 0))
    assert WI.norm("void psvo::wbs_ms::bsim_wobs_fwd_kernel<2, 16, 4, true>(psvo::wbs_ms::FwdArgs)") == \
        ("wbs_ms::bsim_wobs_fwd_kernel", (2, 16, 4, 1))
    assert WI.norm("psvo_memset_kernel(float*)") is None
    assert WI.same_kernel(("bsim_wobs_fwd_kernel", (2, 16, 4, 1)), ("wbs::bsim_wobs_fwd_kernel", (2, 16, 4, 1)))
    assert not WI.same_kernel(("wbs_ms::bsim_wobs_fwd_kernel", (2, 16, 4, 1)), ("wbs::bsim_wobs_fwd_kernel", (2, 16, 4, 1)))


def test_table_shape():
    """the products the sweep is made of, and readable, distinct ids"""
    assert (len(WI.GROUP_A), len(WI.GROUP_B), len(WI.GROUP_C), len(WI.GROUP_D)) == (108, 12, 72, 81)
    assert len({c.id for c in WI.ALL}) == len(WI.ALL)
    for c in WI.GROUP_A:
        assert c.B == 2 and c.T == (6 if c.comp in WI.ADAPTIVE else 4)
        assert c.Dy >= (1 if c.comp in WI.MISSING_LINES else 3) and (c.obj != "IWAE" or c.comp not in WI.ADAPTIVE)
    for c in WI.GROUP_B:
        assert (c.Dx, c.H, c.N, c.Dy, c.B, c.T, c.boot, c.two_q) == (4, 64, 512, 32, 1, 4, False, True)
    for comp in WI.COMPILATIONS:          # every compilation meets both wirings, three waves and every objective it takes
        mine = [c for c in WI.GROUP_A if c.comp == comp]
        assert {c.boot for c in mine} == {c.two_q for c in mine} == {True, False} and any(c.N == 130 for c in mine)
        assert {c.obj for c in mine} == ({"AESMC", "SVO"} if comp in WI.ADAPTIVE else {"AESMC", "SVO", "IWAE"})
    for f in WI.GROUP_D:
        assert (f.T, f.B, f.K, f.Tv) == (3, 2, 2, 4 if f.form == "input" else 3)
    for form in ("plain", "missing", "input"):
        mine = [f for f in WI.GROUP_D if f.form == form]
        assert {f.N for f in mine} == {16, 70} and {f.weights for f in mine} == {"none", "finite", "masked"}
        assert {f.Dy for f in mine} == {1, 2, 3, 10, 32}


@pytest.mark.parametrize("c", WI.FILTER_CASES, ids=_ids)
def test_reference_alone(c):
    p = WI.problem(c, "cpu")
    r64, teacher = WI.reference_teacher(p)
    r32 = WI.evaluate(p, torch.float32, teacher)
    v64, v32 = WI.value_rows(r64.log), WI.value_rows(r32.log)
    assert set(v64) == set(v32) and {"X_prevs", "X_ancestors", "Xs", "log_Ws", "lse"} <= set(v64)
    assert (c.group == "c") == ("bw_Xs" in v64)
    share = {}
    for k, a in v64.items():
        assert torch.isfinite(a).all(), k
        share[k] = float(((v32[k].double() - a).abs() / (WI.VALUE_TOL[k] + WI.RTOL * a.abs())).max())
    z64, z32 = float(r64.z), float(r32.z)
    share["ELBO"] = abs(z32 - z64) / (WI.ELBO_RTOL * abs(z64))
    worst = max(share, key=share.get)
    print("%s: fp32 reference / tolerance, worst %s %.3f (ELBO %.4f)" % (c.id, worst, share[worst], z64))
    assert abs(z64) >= 1.0                        # (the relative tolerance has something to stand on)
    assert share[worst] <= 0.25, share

    # no scale sits on its floor: every d sigma the kernels produce is compared with a gradient that is alive
    for name in WI.SCALES:
        dist = getattr(p.model, name, None)
        if dist is not None and getattr(dist, "sigma_con", None) is not None:
            raw = torch.nn.functional.softplus(dist.sigma_con.detach())
            assert bool((raw > float(dist.sigma_min)).all()), (name, raw, dist.sigma_min)
    assert not any(k.endswith("_sigma_min") for k in c.knobs), c.knobs

    if c.comp in WI.MASKED and c.group != "c":
        miss, t_all, e_never = p.mask
        assert torch.equal(torch.isnan(p.obs), miss)
        assert bool(miss[:, t_all].all())
        n_obs = (~miss).sum(-1)
        assert (c.Dy == 1) or bool(((n_obs > 0) & (n_obs < c.Dy)).any())
        assert bool((n_obs > 0).any())
    elif c.group != "c":
        assert not bool(torch.isnan(p.obs).any())

    if c.comp in ("ad", "msad") and c.group != "c":
        from tests import missing_adaptive_reference as MA
        from tests import wobs_adaptive_reference as WR
        gap32 = WR.ESS_GAP32_WIDE if c.comp == "ad" else MA.ESS_GAP32_MISSING
        rs, ess = r64.log["rs_f"], r64.log["ess"]
        print("%s: resampled %d of %d; closest ESS / N to the threshold %.3e; fp32 ESS gap %.3e N" % (
            c.id, int(rs.sum()), rs.numel(), float((ess / c.N - c.tau).abs().min()),
            float((r32.log["ess"].double() - ess).abs().max()) / c.N))
        assert 0 < int(rs.sum()) < rs.numel()
        assert float((ess / c.N - c.tau).abs().min()) > 100 * 4 * gap32
        assert float((r32.log["ess"].double() - ess).abs().max()) / c.N <= gap32
        assert torch.equal(r32.log["rs_f"], rs)
    if c.comp == "inad":
        rs = r64.log["rs_f"]
        assert torch.equal(rs.long(), WI.forced_pattern(c)) and 0 < int(rs.sum()) < rs.numel()
        for b in range(c.B):
            assert 0 < int(rs[:, b].sum()) < c.T
