"""The table of the wide-family instantiation sweep (tests/test_gpu_wide_instantiations.py on the GPU,
tests/test_wide_instantiations_host.py on the CPU): one small problem per template instantiation of

  a. the wide-observation filters: filter_wobs_impl.h in its six compilations (static, adaptive, missing, missing + adaptive,
     input, input + adaptive), (Dx, H, CNT) each, forward and reverse;
  b. the same six at the shape that needs the most LDS (Dx 4, H 64, N 512, Dy 32, own f), Gaussian and count;
  c. the static wide backward simulation (bsim_wobs.hip: (Dx, H, M, CNT), forward and reverse), through PSVO, with the
     EXT = true reverse forms of the static filter behind it;
  d. the particle forecast (forecast.hip: (Dx, H, EMIS) in its plain, missing and input forms), launched directly.

For every case the table names the device kernels the case must launch, as (base name, template arguments as ints).  norm() turns
a demangled symbol of the library and a torch.profiler kernel name into that pair, so the CPU ledger (table == library) and the
GPU name assertion (table == what ran) speak the same language.  The two backward-simulation units are the same text compiled in
two namespaces (psvo::wbs, psvo::wbs_ms); that namespace is the only one norm() keeps, as a prefix of the base name.

Everything a case computes goes through a reference module the project already has; problem() / evaluate() only pick the
family's own setup and objective for a case.  No GPU is needed to import this file.  A helper, not a test.
"""
import collections
import itertools
import re

import torch

DXS, HS, MS = (2, 3, 4), (16, 32, 64), (4, 8, 16, 32)
COMPILATIONS = ("st", "ad", "ms", "msad", "in", "inad")
SUFFIX = {"st": "", "ad": "_ad", "ms": "_ms", "msad": "_msad", "in": "_in", "inad": "_inad"}
ADAPTIVE = ("ad", "msad", "inad")
MISSING_LINES = ("ms", "msad", "in", "inad")          # the compilations with PSVO_MS = 1: every 1 <= Dy <= 32
MASKED = ("ms", "msad")                               # ... of which these two get NaN entries from the family's mask
INPUT = ("in", "inad")
GAUSS, POISSON, COUNT = "gaussian", "poisson", "count"
EMISSION_FLAGS = {GAUSS: {}, POISSON: dict(poisson_emission=True), COUNT: dict(count_emission=True)}
EMISSION_CODE = {GAUSS: 0, POISSON: 1, COUNT: 2}

# what the sweep is about: a device kernel of one of these families that runs in a case must be one the case names
FAMILY = re.compile(r"^(filter_(fwd|bwd)_wobs(_ad|_ms|_msad|_in|_inad)?_kernel|(wbs|wbs_ms)::bsim_wobs_(fwd|bwd)_kernel|"
                    r"bsim_wobs_(fwd|bwd)_kernel|forecast_kernel)$")
KEPT_NAMESPACES = ("wbs", "wbs_ms")


# ---- kernel names --------------------------------------------------------------------------------------------------------------
def _int(tok):
    tok = re.sub(r"^\([^)]*\)", "", tok)              # (bool)1, (int)4
    if tok in ("true", "false"):
        return int(tok == "true")
    try:
        return int(tok)
    except ValueError:
        return tok


def norm(name):
    """a demangled kernel symbol / a profiler kernel name -> (base name, template arguments as ints), or None when the name has
    no template arguments.  Return type, namespaces (but wbs / wbs_ms), parameter list and whitespace are dropped."""
    s = re.sub(r"\s+", "", name)
    if s.startswith("void"):
        s = s[4:]
    m = re.search(r"[<(]", s)
    if not m or s[m.start()] != "<":
        return None
    parts = s[:m.start()].split("::")
    base = parts[-1]
    if len(parts) > 1 and parts[-2] in KEPT_NAMESPACES:
        base = parts[-2] + "::" + base
    depth, args, tok = 0, [], ""
    for ch in s[m.start():]:
        if ch in "<(":
            depth += 1
            if depth == 1:
                continue
        elif ch in ">)":
            depth -= 1
            if depth == 0:
                args.append(tok)
                break
        if ch == "," and depth == 1:
            args.append(tok)
            tok = ""
        else:
            tok += ch
    return base, tuple(_int(t) for t in args)


def family(names):
    """the normalised names of `names` that belong to the swept families"""
    out = set()
    for n in names:
        k = norm(n)
        if k is not None and FAMILY.match(k[0]):
            out.add(k)
    return out


def same_kernel(ran, want):
    """a name that ran against a name of the table; a profiler that drops namespaces cannot tell the two backward-simulation
    units apart, so a bare bsim_wobs_* name stands for either"""
    return ran == want or (ran[1] == want[1] and "::" not in ran[0] and want[0].split("::")[-1] == ran[0])


def filter_kernels(comp, Dx, H, cnt, ext=False):
    s = SUFFIX[comp]
    return {("filter_fwd_wobs%s_kernel" % s, (Dx, H, int(cnt))), ("filter_bwd_wobs%s_kernel" % s, (Dx, H, int(ext), int(cnt)))}


# ---- the cases -----------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id group comp k Dx H cnt M obj B T N Dy boot two_q emission Di seed knobs tau kernels")
Forecast = collections.namedtuple("Forecast", "id k Dx H emission form T B K N Dy weights Tv gaps kernels")

# Adaptive defaults: the families' `calm` (wobs_adaptive_reference._W: calmer output layers) and WIDE SCALES, without which every
# step of a random model collapses onto a few particles and no decision is ever "keep".  The families widen the scales with the
# floors q2_sigma_min / g_sigma_min; a floored scale has no gradient (clamp), so under those knobs d sig_q2 and d sig_g of an
# instantiation are compared as 0 == 0 -- the planted defect of profiles/wide_instantiations.md (one output's term dropped from
# d sig_g in one instantiation) passed that way.  Here the raw scale parameters are shifted up instead (`*_sigma_shift`, added to
# sigma_con behind the setup: softplus(raw + 3) is about 3.5 .. 5), so the scales are as wide and their gradients are alive;
# tests/test_wide_instantiations_host.py asserts that no scale of any case sits on its floor.
_ADAPTIVE_KNOBS = {GAUSS: dict(calm=0.5, q2_sigma_shift=3.0, g_sigma_shift=3.0),
                   POISSON: dict(calm=0.5, q2_sigma_shift=3.0),
                   COUNT: dict(calm=0.5, q2_sigma_shift=3.0)}
_CORNER_KNOBS = {GAUSS: dict(calm=0.25, q2_sigma_shift=3.0, g_sigma_shift=7.0), COUNT: dict(calm=0.25, q2_sigma_shift=3.0)}
# helpers.perturb_ draws the raw scales from [0.5, 2): softplus of the lower ones is below the flags' default floor *_sigma_min = 1,
# and a floored component has no gradient either.  Every raw scale of a sweep case is lifted by LIFT, which puts the smallest
# at softplus(1.0) = 1.31, so that every component of every d sigma is compared with a gradient that is alive.
LIFT = 0.5
SCALES = ("q0_dist", "q1_dist", "q2_dist", "g_dist", "f_dist", "Bsim_q_init_dist", "q1_inv_dist", "BSim_q2_dist")
SHIFTS = {"q2_sigma_shift": "q2_dist", "g_sigma_shift": "g_dist", "f_sigma_shift": "f_dist", "q1_sigma_shift": "q1_dist"}

# Cases whose seed, knobs or threshold were moved off the rotation, and why (profiles/wide_instantiations.md repeats the list).
# Every entry was chosen on the CPU with the reference alone (tests/test_wide_instantiations_host.py holds the conditions):
#   "mixed":  with the rotation's seed the fp64 reference, free running, resampled at every step (or kept every step), or came
#             closer to its threshold than 100 x the GPU's ESS margin;
#   "ess32":  with the rotation's seed the fp32 reference's ESS left its fp64 self by more than the family's recorded
#             ESS_GAP32 figure, which the GPU's ESS margin is built on.
# No case had to be moved for the value tolerances: with the rotation's seeds the fp32 reference stays within a quarter of each.
MOVED = {
    "ad-2-32-cnt": dict(seed=6, why="mixed"),
    "ad-2-64": dict(seed=3, tau=0.25, why="mixed"),
    "ad-2-64-cnt": dict(seed=3, tau=0.25, why="mixed"),
    "ad-3-16-cnt": dict(seed=8, why="mixed"),
    "ad-3-32": dict(seed=3, why="mixed"),
    "ad-3-32-cnt": dict(seed=4, tau=0.25, why="mixed"),
    "ad-3-64-cnt": dict(seed=3, tau=0.25, why="mixed"),
    "ad-4-16": dict(seed=3, tau=0.25, why="mixed"),
    "ad-4-16-cnt": dict(seed=3, tau=0.25, knobs=dict(calm=0.25), why="mixed"),
    "ad-4-64": dict(seed=3, tau=0.25, why="mixed"),
    "ad-4-64-cnt": dict(seed=4, why="mixed"),
    "msad-2-16": dict(seed=3, why="mixed"),
    "msad-3-64": dict(seed=6, why="ess32"),
    "msad-4-16-cnt": dict(seed=6, why="mixed"),
    "msad-4-32": dict(seed=3, why="ess32"),
    "msad-4-32-cnt": dict(seed=4, why="mixed"),
    "msad-4-64": dict(seed=4, why="mixed"),
    "corner-ad": dict(seed=5, why="mixed"),
    "corner-ad-cnt": dict(seed=13, why="mixed"),
    "corner-msad": dict(seed=11, why="mixed"),
}


def _a_case(k, comp, Dx, H, cnt, corner=False):
    adaptive, lines = comp in ADAPTIVE, comp in MISSING_LINES
    if corner:
        B, T, N, Dy, boot, two_q, obj = 1, 4, 512, 32, False, True, "AESMC"
        emission = COUNT if cnt else GAUSS
        seed, tau = 3, (0.5 if comp == "inad" else 0.25)          # (input + adaptive: the family's fixed threshold)
        knobs = dict(_CORNER_KNOBS[emission]) if adaptive else {}
        cid = "corner-%s%s" % (comp, "-cnt" if cnt else "")
    else:
        B, T = 2, (6 if adaptive else 4)
        N = 130 if k % 5 == 4 else (20, 36, 12)[k % 3]
        Dy = (1, 2, 3, 10, 32)[k % 5] if lines else (3, 10, 17, 32)[(k // 2) % 4]
        boot, two_q = k % 3 != 1, k % 4 != 3
        obj = ("AESMC", "SVO")[(k // 3) % 2] if adaptive else ("AESMC", "SVO", "IWAE")[(k // 2) % 3]
        emission = COUNT if cnt else (GAUSS, POISSON)[(k // 2) % 2]
        seed, tau = 3 + k % 5, 0.5
        knobs = dict(_ADAPTIVE_KNOBS[emission]) if adaptive else {}
        cid = "%s-%d-%d%s" % (comp, Dx, H, "-cnt" if cnt else "")
    Di = (1, 2, 3)[k % 3] if comp in INPUT else 0
    moved = MOVED.get(cid, {})
    seed, tau = moved.get("seed", seed), moved.get("tau", tau)
    knobs.update(moved.get("knobs", {}))
    return Case(cid, "b" if corner else "a", comp, k, Dx, H, cnt, 1, obj, B, T, N, Dy, boot, two_q, emission, Di, seed, knobs, tau,
                frozenset(filter_kernels(comp, Dx, H, cnt)))


def _c_case(k, Dx, H, M, cnt):
    """tests/test_gpu_missing_bsim.py::test_every_instantiation's shapes, Dy >= 3"""
    cid = "bsim-%d-%d-%d%s" % (Dx, H, M, "-cnt" if cnt else "")
    emission = COUNT if cnt else (GAUSS, POISSON)[(k // 2) % 2]
    kernels = {("wbs::bsim_wobs_fwd_kernel", (Dx, H, M, int(cnt))), ("wbs::bsim_wobs_bwd_kernel", (Dx, H, M, int(cnt)))}
    kernels |= filter_kernels("st", Dx, H, cnt, ext=True)
    moved = MOVED.get(cid, {})
    return Case(cid, "c", "st", k, Dx, H, cnt, M, "PSVO", 2, 6, (20, 36, 12)[k % 3], (3, 10, 17, 32)[(k // 2 + k // 8) % 4],
                k % 3 != 1, True, emission, 0, moved.get("seed", 5), dict(moved.get("knobs", {})), 0.0, frozenset(kernels))


def _d_case(k, Dx, H, emission, form):
    ms, inp = int(form != "plain"), int(form == "input")
    T = 3
    return Forecast("fc-%d-%d-e%d-%s" % (Dx, H, emission, form), k, Dx, H, emission, form, T, 2, 2, (16, 70)[k % 2],
                    (1, 2, 3, 10, 32)[k % 5], ("none", "finite", "masked")[(k // 3 + k // 9) % 3], T + 1 if inp else T,
                    form == "missing" or (inp and (k // 3) % 2 == 1), frozenset({("forecast_kernel", (Dx, H, emission, ms, inp))}))


def _build():
    a = [_a_case(k, comp, Dx, H, cnt)
         for k, (comp, Dx, H, cnt) in enumerate(itertools.product(COMPILATIONS, DXS, HS, (False, True)))]
    b = [_a_case(k, comp, 4, 64, cnt, corner=True) for k, (comp, cnt) in enumerate(itertools.product(COMPILATIONS, (False, True)))]
    c = [_c_case(k, *combo) for k, combo in enumerate(itertools.product(DXS, HS, MS, (False, True)))]
    d = [_d_case(k, *combo) for k, combo in enumerate(itertools.product(DXS, HS, (0, 1, 2), ("plain", "missing", "input")))]
    return a, b, c, d


GROUP_A, GROUP_B, GROUP_C, GROUP_D = _build()
FILTER_CASES = GROUP_A + GROUP_B + GROUP_C          # everything with a model behind it (values and gradients)
ALL = FILTER_CASES + GROUP_D


def missing_form_kernels():
    """the kernels tests/test_gpu_missing_bsim.py::test_every_instantiation sweeps: the missing form of the backward simulation
    and the EXT = true reverse form of the missing filter, claimed through that sweep's own table"""
    from tests.test_gpu_missing_bsim import EVERY
    out = set()
    for Dx, H, M, cnt in EVERY:
        out |= {("wbs_ms::bsim_wobs_fwd_kernel", (Dx, H, M, int(cnt))), ("wbs_ms::bsim_wobs_bwd_kernel", (Dx, H, M, int(cnt))),
                ("filter_bwd_wobs_ms_kernel", (Dx, H, 1, int(cnt)))}
    return out


def promised():
    """every kernel some case of this table (or of the missing backward simulation's own sweep) must launch"""
    out = set(missing_form_kernels())
    for c in ALL:
        out |= c.kernels
    return out


# ---- a case's problem and its reference ----------------------------------------------------------------------------------------
Problem = collections.namedtuple("Problem", "case FLAGS model smc obs noise v mask")


def _calm(model, calm):
    """adaptive_reference.setup's `calm` for the setups that do not have it: the output layers scaled down"""
    if calm != 1.0:
        with torch.no_grad():
            for name, p in model.named_parameters():
                if name.endswith("mu_kernel"):
                    p.mul_(calm)


def _tuple10(c):
    return (c.obj, c.B, c.T, c.N, c.M, c.Dx, c.Dy, c.H, c.boot, c.two_q)


def _adaptive_tuple(c):
    flags = dict({k: v for k, v in c.knobs.items() if k not in SHIFTS}, **EMISSION_FLAGS[c.emission])
    return (c.obj, c.B, c.T, c.N, c.Dx, c.Dy, str(c.H), c.boot, c.two_q, flags, c.seed, c.tau)


def problem(c, device="cpu"):
    """the family's own setup for a case: Problem(case, FLAGS, model, smc, obs (B,T,Dy) fp64, noise, v (B,T,Di) fp64 or None,
    (miss, t_all, e_never) or None)"""
    from tests import count_reference as CR
    knobs = {k: v for k, v in c.knobs.items() if k not in SHIFTS}
    calm = knobs.pop("calm", 1.0) if c.comp not in ("ad", "msad") or c.group == "c" else 1.0
    extra = dict(knobs, **EMISSION_FLAGS[c.emission])
    v = mask = None
    if c.group == "c":
        from tests import test_gpu_wobs_bsim as TB
        FLAGS, model, smc, obs, noise = TB._wide(_tuple10(c), dict(extra, device=device), c.seed)
        if c.cnt:
            obs = CR.counts(c.B, c.T, c.Dy, 100 + c.seed)
    elif c.comp == "st":
        from tests.test_gpu_parity import _setup
        FLAGS, model, smc, obs, noise = _setup(*_tuple10(c), seed=c.seed, device=device, **extra)
        assert smc.wide_obs
        if c.cnt:
            obs = CR.counts(c.B, c.T, c.Dy, 100 + c.seed)
    elif c.comp == "ad":
        from tests import wobs_adaptive_reference as WR
        FLAGS, model, smc, obs, noise = WR.setup(_adaptive_tuple(c), device)
        assert smc.wide_obs and smc.resample_ess == c.tau
    elif c.comp == "ms":
        from tests import missing_reference as MR
        from tests import test_gpu_missing as TM
        extra.pop("count_emission", None)
        FLAGS, model, smc, obs, noise, _ = TM._missing((_tuple10(c), c.cnt), c.seed, device=device, **extra)
        mask = MR.mask(c.B, c.T, c.Dy, c.seed)
    elif c.comp == "msad":
        from tests import missing_adaptive_reference as MA
        FLAGS, model, smc, obs, noise, mask = MA.setup(_adaptive_tuple(c), device)
        assert smc.missing_obs and smc.resample_ess == c.tau
    else:
        from tests import test_gpu_exo as TE
        extra.pop("count_emission", None)
        if c.cnt and c.Dy <= 2:          # (the count emission at a plain width exists in the missing-observation route only)
            extra["missing_obs"] = True
        if c.comp == "inad":
            from tests import exo_adaptive_reference as XA
            assert c.tau == XA.TAU
            extra.update(resample_ess=c.tau, resample_ess_inputs=True)
            if extra.get("missing_obs"):
                extra["resample_ess_missing_obs"] = True
        FLAGS, model, smc, obs, v, noise = TE.exo_setup((_tuple10(c), c.Di, "count" if c.cnt else ""), c.seed, device=device,
                                                        **extra)
    _calm(model, calm)
    with torch.no_grad():
        lifted = set()
        for name in SCALES:          # every scale off its floor (see LIFT); f_dist is q1_dist under bootstrap
            dist = getattr(model, name, None)
            if dist is not None and getattr(dist, "sigma_con", None) is not None and id(dist.sigma_con) not in lifted:
                lifted.add(id(dist.sigma_con))
                dist.sigma_con.add_(LIFT)
        for k, name in SHIFTS.items():
            if c.knobs.get(k) and getattr(model, name, None) is not None:          # (no q2 without two_q)
                getattr(model, name).sigma_con.add_(float(c.knobs[k]))
    return Problem(c, FLAGS, model, smc, obs, noise, v, mask)


def _objective(p, P):
    from oracle import psvo_oracle as O
    from tests import count_reference as CR
    from tests import helpers as Hh
    c = p.case
    if c.group == "c" or c.comp == "st":
        return CR.objective(P, p.FLAGS, c.obj) if c.cnt else O.OBJECTIVES[c.obj](P, Hh.oracle_flags(p.FLAGS, c.obj))
    if c.comp == "ad":
        from tests import wobs_adaptive_reference as WR
        return WR.objective(P, p.FLAGS, _adaptive_tuple(c))
    if c.comp == "ms":
        from tests import missing_reference as MR
        return MR.objective(P, p.FLAGS, c.obj)
    if c.comp == "msad":
        from tests import missing_adaptive_reference as MA
        return MA.objective(P, p.FLAGS, _adaptive_tuple(c))
    from tests import exo_reference as ER
    return ER.objective(P, p.FLAGS, c.obj)


Result = collections.namedtuple("Result", "z log P dv draws")


def evaluate(p, dtype=torch.float64, teacher=None, grad=False):
    """the family's reference on a problem, in `dtype`, with `teacher` (idx_f / idx_b / rs_f in the reference's layouts) forced:
    Result(ELBO, the reference's log, its parameters (with .grad under grad=True), d ELBO / d v or None, the draws it made as
    (logits, uniform, index) for oracle.draw_distance)"""
    from tests import missing_reference as MR
    c = p.case
    P = p.model.export_reference_layout(dtype)
    if grad:
        MR.require_grad(P)
    o = _objective(p, P)
    o.draw_log = []
    nz = MR._cast({**p.noise, **(teacher or {})}, dtype)
    obs = p.obs.to(dtype).cpu()
    v = None if p.v is None else p.v.to(dtype).cpu().clone().requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        if c.comp == "in" and c.group != "c":
            from tests import exo_reference as ER
            z, log = ER.smc(o, obs, v, nz)
        elif c.comp == "inad":
            from tests import exo_adaptive_reference as XA
            z, log = XA.smc(o, obs, v, nz, c.tau)
        else:
            z, log = o.get_log_ZSMC(obs, nz)
        if grad:
            z.backward()
    return Result(z.detach(), log, P, None if (v is None or not grad) else v.grad, o.draw_log)


def forced_pattern(c):
    """input + adaptive: the family's fixed mixed pattern of decisions (exo_adaptive_reference.forced), (T, B) int64"""
    from tests import exo_adaptive_reference as XA
    return XA.forced(c.T, c.B).long()


def reference_teacher(p):
    """the fp64 reference run once, free (input + adaptive: under the family's forced pattern), and what the kernels are then
    forced with: (Result, teacher).  Adaptive forms: the decisions rs_f are part of the teacher."""
    c = p.case
    first = {"rs_f": forced_pattern(c)} if c.comp == "inad" else None
    r = evaluate(p, teacher=first)
    teacher = {}
    if r.log.get("idx_f") is not None:
        teacher["idx_f"] = r.log["idx_f"]
    if c.group == "c":
        teacher["idx_b"] = r.log["idx_b"]
    if c.comp in ADAPTIVE and c.group != "c":
        teacher["rs_f"] = r.log["rs_f"].long()
    return r, teacher


# value tolerances of the families (atol; rtol 1e-5 each), by the reference's key
VALUE_TOL = {"X_prevs": 2e-4, "X_ancestors": 2e-4, "Xs": 2e-4, "log_Ws": 5e-4, "lse": 5e-4,
             "bw_Xs": 2e-4, "f_log_probs": 5e-4, "g_log_probs": 5e-4, "bw_log_Omegas": 5e-4}
RTOL, ELBO_RTOL = 1e-5, 1e-4


def value_rows(log):
    """the compared quantities of a reference log: {key: fp64 tensor}"""
    out = {k: log[k].double() for k in VALUE_TOL if k in log and log[k] is not None}
    out["lse"] = torch.logsumexp(log["log_Ws"].double(), 1)
    return out


# ---- forecast systems ----------------------------------------------------------------------------------------------------------
def forecast_case(f):
    """the system of a forecast case with both references: forecast_reference.system, under the missing form with
    missing_reference.mask knocked out of obs, under the input form with exo_forecast_reference's bias rows; c["valid"] is the
    (K+1, T[, B]) mask of the scored entries"""
    from tests import exo_forecast_reference as XR
    from tests import forecast_reference as R
    from tests import missing_reference as MR
    shape = (f.T, f.B, f.Dx, f.Dy, f.H, f.N, f.K, f.emission)
    c = dict(R.system(*shape, weights=f.weights, noisy=True))
    c["shape"] = shape
    if f.gaps:
        c["obs"] = MR.knock_out(c["obs"], MR.mask(f.B, f.T, f.Dy, 3)[0].permute(1, 0, 2).contiguous())
    if f.form == "plain":
        c["ref64"], c["ref32"] = R.run(c, torch.float64), R.run(c, torch.float32)
        c["valid"] = R.valid_mask(f.T, f.K)
    elif f.form == "missing":
        from tests import test_gpu_forecast_missing as FM
        c["ref64"], c["ref32"] = FM._forecast(c, torch.float64), FM._forecast(c, torch.float32)
        c["valid"] = XR.scored(c["obs"], f.T, f.K)
    else:
        c["Tv"], c["hb_f"] = f.Tv, XR.hb_rows(f.Tv, f.B, f.H)
        c["ref64"], c["ref32"] = XR.run(c, torch.float64), XR.run(c, torch.float32)
        c["valid"] = XR.scored(c["obs"], f.T, f.K)
    return c
