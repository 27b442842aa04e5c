"""Vector-Jacobian products of every reverse route against fp64 autograd of the oracle, under cotangents that are NOT the ELBO's.

The ELBO hands most reverse kernels a constant upstream gradient (1 / B at every (t, b) of lse and lseW; a positive softmax over
the chains for score), under which a kernel that reads the cotangent of another step or another sequence is exactly right.  Here
the product runs forward as always, the returned ELBO is ignored and .backward() is called on a weighted sum of the autograd node's
own differentiable outputs,

    filter nodes   sum c_lse lse  (+ sum c_Fm Fm + sum c_logW logW (+ sum c_Fs Fs) where the node accepts them)
    PSVO           sum c score,  c (B, N)
    PSVOwR         sum c lseW,   c (T, B)

with c signed, N(0, 1) times a per-sequence scale 1 + b, drawn in fp64 from a seeded generator and cast once to fp32; the oracle
gets that fp32 value cast back, so both sides use the same numbers.  The oracle side forms the same sum in fp64 on the
graph-attached log its get_log_ZSMC returns: lse = logsumexp(log_Ws, 1), logW = log_Ws, Fm (Fs) = f.mean (mean_and_sigma) of
X_prevs, score = sum_t (f_log_probs + g_log_probs - bw_log_Omegas), lseW = logsumexp(bw_log_W, 1).  The oracle objects are the
features' own (tests/adaptive_reference.py, wobs_adaptive_reference.py, missing_reference.py, missing_adaptive_reference.py,
missing_bsim_reference.py, count_reference.py, exo_reference.py, exo_adaptive_reference.py; O.OBJECTIVES for the plain,
state-dependent-scale and wide PSVO routes), and so are the masks, the count data, the exogenous inputs and the layout of the
forced resampling decisions.

The input families (FLAGS.Di: "input", "input_adaptive") have one more leaf on both sides, the input v (B, T, Di): the product
gets it as an fp32 leaf, the references through InputOracle.  Besides the parameters (compare) their input rows W1[Dx:] are
compared on their own and d v per sequence, each d v[b] at its own scale under the same two clauses, and wherever the reference
has d v[b, t] exactly zero the bound is ATOL alone (input_rows, compare_inputs): these are the only routes that turn a
cotangent into rows d hb[t, b, :], and a row written to another step or sequence lands where the reference has none.

Comparison (compare): over test_gpu_parity._pairs, a missing gradient counting as zero, under the suite's rule for gradients --
error <= 2e-3 x the reference tensor's largest entry + 1e-6 -- or else the K32 clause of tests/test_gpu_instantiations.py: error
<= K32 x the fp32 ORACLE's own error on that tensor under the same surrogate (computed only when the first clause fails).  Signed
cotangents make sums cancel, so the second clause binds more often than under the ELBO; it is measured against the reference's
arithmetic, never against the kernel.  A model seed is fit for a case when the fp32 oracle itself stays inside the first clause
on at least three quarters of the tensors (fp32_share_over; tests/test_vjp_host.py holds every case to it on the CPU).

140 cases in groups (a)-(k) (CASES below; tests/test_gpu_vjp.py runs them in 6.3 s on one MI355X).  A helper, not a test; only
tests and tools import it.
"""
import contextlib

import torch

from oracle import psvo_oracle as O
from tests import adaptive_reference as AR
from tests import count_reference as CR
from tests import exo_adaptive_reference as XA
from tests import exo_reference as ER
from tests import helpers as Hh
from tests import missing_adaptive_reference as MA
from tests import missing_bsim_reference as MB
from tests import missing_reference as MR
from tests import wobs_adaptive_reference as WR
from tests.test_gpu_instantiations import K32
from tests.test_gpu_parity import _pairs

B, T = 3, 5             # t*B + b, b*T + t and b all differ; the last sequence has offset 2; ordinary steps between the peeled ends
RTOL, ATOL = 2e-3, 1e-6  # the suite's rule for gradients (tests/test_gpu_parity.py::_grad_mismatches)
TAU = 0.5               # FLAGS.resample_ess of the adaptive routes (the decisions themselves are forced)

GAUSS, UNIT, COUNT = "gaussian", "unitnormal", "count"
# the autograd node a family's filter runs through and the outputs it leaves differentiable (psvo_amd/autograd.py)
FILTER_NODE = {
    "plain": ("FilterFunction", {"lse", "Fm", "logW"}),
    "cov": ("FilterCovFunction", {"lse", "Fm", "Fs", "logW"}),
    "wide": ("FilterWobsFunction", {"lse", "Fm", "logW"}),
    "adaptive": ("FilterAdaptiveFunction", {"lse"}),
    "wide_adaptive": ("FilterWobsAdaptiveFunction", {"lse"}),
    "missing": ("FilterWobsMissingFunction", {"lse"}),
    "missing_adaptive": ("FilterWobsMissingAdaptiveFunction", {"lse"}),
    "missing_bsim": ("FilterWobsMissingBsimFunction", {"lse", "Fm", "logW"}),
    "input": ("FilterWobsInputFunction", {"lse"}),
    "input_adaptive": ("FilterWobsInputAdaptiveFunction", {"lse"}),
}
BSIM_NODE = {
    ("PSVO", "plain"): ("BsimFunction", "score"), ("PSVO", "cov"): ("BsimCovFunction", "score"),
    ("PSVO", "missing_bsim"): ("BsimWobsMissingFunction", "score"), ("PSVO", "wide"): ("BsimWobsFunction", "score"),
    ("PSVOwR", "plain"): ("BsimWRFunction", "lseW"), ("PSVOwR", "cov"): ("BsimWRCovFunction", "lseW"),
}
ADAPTIVE = ("adaptive", "wide_adaptive", "missing_adaptive", "input_adaptive")
MISSING = ("missing", "missing_adaptive", "missing_bsim")
INPUT = ("input", "input_adaptive")     # FLAGS.Di > 0 (Case.flags carries Di): the exogenous input is a leaf on both sides


class Case(object):
    """one vector-Jacobian case: `route` names the kernel or entry point it is there for (it is the test id), `family` the
    host wiring (a key of FILTER_NODE), `cots` the outputs that get a cotangent, `tune` the psvo_set_tuning switches as
    (name of the key in psvo_amd._lib, value), `hot` (t0, b0) of a one-hot c_lse / c_lseW instead of the random draw"""

    def __init__(self, route, obj, N, Dx=2, Dy=1, family="plain", cots=("lse",), M=4, H=32, boot=True, two_q=True, tune=(),
                 emission=GAUSS, layers=1, seed=5, hot=None, flags=None):
        self.route, self.obj, self.N, self.Dx, self.Dy, self.family, self.cots = route, obj, N, Dx, Dy, family, tuple(cots)
        self.M, self.H, self.boot, self.two_q, self.tune, self.emission = M, H, boot, two_q, tuple(tune), emission
        self.layers, self.seed, self.hot, self.flags = layers, seed, hot, dict(flags or {})

    @property
    def id(self):
        parts = [self.route, self.obj, "N%d" % self.N, "Dx%d" % self.Dx, "Dy%d" % self.Dy, "+".join(self.cots)]
        if self.flags.get("Di"):
            parts.append("Di%d" % self.flags["Di"])
        if self.emission != GAUSS:
            parts.append(self.emission)
        if self.flags.get("missing_obs"):
            parts.append("missing")
        if self.hot is not None:
            parts.append("onehot_t%d_b%d" % self.hot)
        return "-".join(parts)

    def one_hot_at(self, t0, b0=B - 1):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.hot, c.cots = (t0, b0), (self.cots[0],)
        return c


def cotangents(shape_dict, seed):
    """{name: shape} -> {name: fp32 cotangent}: signed N(0, 1) in fp64 from a seeded generator, times 1 + b along the sequence
    axis (axis 0 of score (B, N), axis 1 of everything else) so that the sequences are told apart in the sum over b, cast once"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(shape_dict):
        shape = tuple(shape_dict[name])
        axis = 0 if name == "score" else 1
        c = torch.randn(*shape, generator=g, dtype=torch.float64)
        scale = 1.0 + torch.arange(shape[axis], dtype=torch.float64)
        c = c * scale.view([-1 if i == axis else 1 for i in range(len(shape))])
        out[name] = c.to(torch.float32)
    return out


def one_hot(shape, index):
    """fp32 cotangent that is 1 at `index` and 0 elsewhere"""
    c = torch.zeros(*shape, dtype=torch.float32)
    c[tuple(index)] = 1.0
    return c


def shapes_of(case):
    s = {"lse": (T, B), "Fm": (T, B, case.Dx, case.N), "Fs": (T, B, case.Dx, case.N), "logW": (T, B, case.N),
         "score": (B, case.N), "lseW": (T, B)}
    return {k: s[k] for k in case.cots}


def cotangents_of(case):
    if case.hot is not None:
        (name,) = case.cots
        return {name: one_hot((T, B), case.hot)}
    return cotangents(shapes_of(case), 4000 + case.seed)


def forced_decisions():
    """(T, B) int64, non-zero = resample: mixed along both axes (every sequence keeps at some steps and resamples at others, and
    at every step but the last some sequence keeps while another resamples), so that the !rs_here chain through d lnw runs"""
    t, b = torch.arange(T)[:, None], torch.arange(B)[None, :]
    rs = ((t + b) % 2 == 0).long()
    assert 0 < int(rs.sum()) < T * B and bool((rs.sum(0) > 0).all()) and bool((rs.sum(0) < T).all())
    return rs


def mask(Dy, seed):
    """missing_reference.mask, whose ragged tail exists at B = 2 only, with that tail on the last sequence of B = 3"""
    miss, t_all, e_never = MR.mask(B, T, Dy, seed)
    miss[B - 1, T - 2:, :] = True
    assert t_all < T - 2 and bool(miss[:, t_all].all()) and not bool(miss[0, 0].all())
    return miss, t_all, e_never


class Problem(object):
    pass


class InputOracle(object):
    """exo_reference.smc (ess_frac None) or exo_adaptive_reference.smc on the objective `o` and the inputs `v` (B, T, Di), in the
    get_log_ZSMC(obs, noise) shape oracle_run expects.  Every run holds v as a fresh leaf of the run's dtype in .v, so that
    .v.grad is d v once the surrogate has been differentiated."""

    def __init__(self, o, v, ess_frac=None):
        self.o, self.f, self.ess_frac, self._v, self.v = o, o.f, ess_frac, v, None

    def get_log_ZSMC(self, obs, noise):
        self.v = self._v.to(obs.dtype).cpu().clone().requires_grad_(True)
        if self.ess_frac is None:
            return ER.smc(self.o, obs, self.v, noise)
        return XA.smc(self.o, obs, self.v, noise, self.ess_frac)


def setup(case, device="cpu"):
    """tests/test_gpu_parity.py::_setup for `case` on `device` (same seeding), with the family's flags, data and reference"""
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.IWAE import IWAE
    from psvo_amd.SMC.PSVO import PSVO
    from psvo_amd.SMC.PSVOwR import PSVOwR
    from psvo_amd.SMC.SVO import SVO
    cls = {"SVO": SVO, "PSVO": PSVO, "AESMC": AESMC, "IWAE": IWAE, "PSVOwR": PSVOwR}[case.obj]
    fam, seed = case.family, case.seed
    hs = ",".join([str(case.H)] * case.layers)
    one = str(case.H)
    kw = dict(Dx=case.Dx, Dy=case.Dy, n_particles=case.N, n_particles_for_BSim_proposal=case.M, batch_size=B, time=T,
              q0_layers=one, q1_layers=hs, q2_layers=one, f_layers=hs, g_layers=hs, y_smoother_Dhs="8", X0_smoother_Dhs="8",
              use_bootstrap=case.boot, use_2_q=case.two_q)
    if fam == "cov":
        kw.update(output_cov=True, diag_cov=True)
    if fam in ADAPTIVE:
        kw.update(resample_ess=TAU)
    if fam == "wide_adaptive":
        kw.update(resample_ess_wide_obs=True)
    if fam in MISSING:
        kw.update(missing_obs=True)
    if fam == "missing_adaptive":
        kw.update(resample_ess_missing_obs=True)
    if fam == "missing_bsim":
        kw.update(BSim_missing_obs=True)
    if fam == "input_adaptive":
        kw.update(resample_ess_inputs=True)
    if case.emission == COUNT:
        kw.update(count_emission=True)
    if case.emission == UNIT:
        kw.update(poisson_emission=True)
    kw.update(case.flags)
    p = Problem()
    p.case = case
    p.FLAGS = FLAGS = Hh.make_flags(case.obj, **kw)
    torch.manual_seed(seed)
    p.model = Hh.perturb_(SSM(FLAGS)).to(device)
    p.smc = cls(p.model, FLAGS)
    g = torch.Generator().manual_seed(100 + seed)
    p.obs = torch.randn(B, T, case.Dy, generator=g, dtype=torch.float64) * 1.5
    if case.emission == COUNT:
        p.obs = CR.counts(B, T, case.Dy, 100 + seed).double()
    p.noise = O.make_noise(Hh.oracle_flags(FLAGS, case.obj), B, T, seed=1234 + seed)
    p.e_never = None
    if fam in MISSING or FLAGS.missing_obs:
        miss, _, p.e_never = mask(case.Dy, seed)
        p.obs = MR.knock_out(p.obs, miss)
    p.forced = forced_decisions() if fam in ADAPTIVE else None
    p.inputs = ER.inputs(B, T, FLAGS.Di, seed) if fam in INPUT else None
    # the tuple the adaptive references read their emission from: (objective, .., flags at [9], ..)
    pseudo = (case.obj, B, T, case.N, case.Dx, case.Dy, hs, case.boot, case.two_q,
              {"count_emission": True} if case.emission == COUNT else {}, seed, TAU)
    if fam == "adaptive":
        p.objective = lambda P: AR.objective(P, FLAGS, case.obj)
    elif fam == "wide_adaptive":
        p.objective = lambda P: WR.objective(P, FLAGS, pseudo)
    elif fam == "missing":
        p.objective = lambda P: MR.objective(P, FLAGS, case.obj)
    elif fam == "missing_adaptive":
        p.objective = lambda P: MA.objective(P, FLAGS, pseudo)
    elif fam == "missing_bsim":
        p.objective = lambda P: MB.objective(P, FLAGS, case.obj)
    elif fam in INPUT:
        p.objective = lambda P: InputOracle(ER.objective(P, FLAGS, case.obj), p.inputs, TAU if fam in ADAPTIVE else None)
    elif case.emission == COUNT:
        p.objective = lambda P: CR.objective(P, FLAGS, case.obj)
    else:
        p.objective = lambda P: O.OBJECTIVES[case.obj](P, Hh.oracle_flags(FLAGS, case.obj))
    return p


def _cast(nz, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in nz.items()}


def teacher_of(log):
    """the indices an oracle run drew, to be forced on the kernels and on the fp32 oracle"""
    return {k: log[k] for k in ("idx_f", "idx_b", "idx_r") if log.get(k) is not None}


def oracle_outputs(o, log, family):
    """the oracle's differentiable outputs in the product's layouts, still attached to the graph"""
    out = {"lse": torch.logsumexp(log["log_Ws"], 1), "logW": log["log_Ws"].permute(0, 2, 1)}
    if family == "cov":
        Fm, Fs = o.f.mean_and_sigma(log["X_prevs"])
        out["Fs"] = Fs.permute(0, 2, 3, 1)
    else:
        Fm = o.f.mean(log["X_prevs"])
    out["Fm"] = Fm.permute(0, 2, 3, 1)                                   # (T, N, B, Dx) -> (T, B, Dx, N)
    if "bw_log_Omegas" in log:
        out["score"] = (log["f_log_probs"] + log["g_log_probs"] - log["bw_log_Omegas"]).sum(0).permute(1, 0)
    if "bw_log_W" in log:
        out["lseW"] = torch.logsumexp(log["bw_log_W"], 1)
    return out


def oracle_run(p, dtype=torch.float64, teacher=None):
    """the reference of p in `dtype` under autograd: (P with leaves, oracle object, z, log)"""
    P = MR.require_grad(p.model.export_reference_layout(dtype))
    o = p.objective(P)
    nz = {**p.noise, **(teacher or {})}
    if p.forced is not None:
        nz["rs_f"] = p.forced
    z, log = o.get_log_ZSMC(p.obs.to(dtype).cpu(), _cast(nz, dtype))
    return P, o, z, log


def oracle_vjp(p, cots, dtype=torch.float64, teacher=None):
    """gradients of sum_k <cots[k], output k> in P's .grad; returns (P, teacher of this run, the outputs detached).  On the
    input families P["inputs"] is the run's input leaf (B, T, Di), its .grad d v"""
    P, o, _, log = oracle_run(p, dtype, teacher)
    outs = oracle_outputs(o, log, p.case.family)
    loss = sum((c.to(dtype) * outs[k]).sum() for k, c in cots.items())
    loss.backward()
    if p.inputs is not None:
        P["inputs"] = o.v
    return P, teacher_of(log), {k: v.detach() for k, v in outs.items()}


def hip_noise(p, teacher):
    nz = Hh.noise_to_hip({**p.noise, **teacher}, "cuda")
    for u, idx in (("u_f", "idx_f"), ("u_b", "sel_b"), ("u_r", "anc_r")):
        if idx in nz:
            nz.pop(u, None)
    if p.forced is not None:
        nz["rs_f"] = p.forced.to(torch.int32).contiguous().cuda()
    return nz


def differentiable_outputs(log, case):
    """{name: output} of the autograd nodes of a product run, after asserting that each node is the family's and leaves
    differentiable exactly the outputs expected of it -- a node that silently drops a cotangent is noticed here"""
    filt = log["filter"]
    node, want = FILTER_NODE[case.family]
    assert type(filt["lse"].grad_fn).__name__ == node + "Backward", (type(filt["lse"].grad_fn).__name__, node)
    got = {k for k, v in filt.items() if torch.is_tensor(v) and v.requires_grad}
    assert got == want, "differentiable outputs of %s: %s, expected %s" % (node, sorted(got), sorted(want))
    outs = {k: filt[k] for k in want}
    if "bsim" in log:
        bnode, key = BSIM_NODE[(case.obj, case.family)]
        bs = log["bsim"]
        assert type(bs[key].grad_fn).__name__ == bnode + "Backward", (type(bs[key].grad_fn).__name__, bnode)
        got = {k for k, v in bs.items() if torch.is_tensor(v) and v.requires_grad}
        assert got == {key}, "differentiable outputs of %s: %s" % (bnode, sorted(got))
        outs[key] = bs[key]
    return outs


def product_vjp(p, cots, teacher):
    """the product's forward pass (model on the GPU) and .backward() on the surrogate, under the case's tuning switches;
    the gradients are left in the model's .grad; returns (the node outputs, detached; d v (B, T, Di) of the fp32 input leaf on
    the input families, else None)"""
    from psvo_amd import _lib
    nz = hip_noise(p, teacher)
    p.model.zero_grad()
    v = None if p.inputs is None else p.inputs.float().cuda().requires_grad_(True)
    with contextlib.ExitStack() as st:
        for key, value in p.case.tune:
            st.enter_context(Hh.tuning(getattr(_lib, key), value))
        _, log = p.smc.get_log_ZSMC(p.obs.float().cuda(), None, noise=nz, **({} if v is None else {"inputs": v}))
        outs = differentiable_outputs(log, p.case)
        assert set(cots) <= set(outs), (sorted(cots), sorted(outs))
        loss = sum((c.cuda() * outs[k]).sum() for k, c in cots.items())
        loss.backward()
        torch.cuda.synchronize()
    if p.case.obj == "PSVOwR" and p.case.family == "plain":
        p.smc.check_exchange()
    return {k: o.detach() for k, o in outs.items()}, (None if v is None else v.grad)


def grad_rows(model, P, P_ref):
    """(name, max abs difference of P's gradient from P_ref's, largest entry of P_ref's) per trainable tensor; `model` only
    orders the tensors.  P may be the model itself (its .grad) or an oracle layout (fp32)."""
    rows = []
    other = None if P is model else _pairs(model, P)
    for i, (name, par, ref) in enumerate(_pairs(model, P_ref)):
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        src = par if other is None else other[i][2]
        g = torch.zeros_like(ref) if src.grad is None else src.grad.detach().double().cpu().reshape(ref.shape)
        rows.append((name, float((g - r).abs().max()), max(float(r.abs().max()), 1e-6)))
    return rows


def input_rows(p, P, P_ref, dv=None):
    """the rows an input family adds to grad_rows, same triples: the input rows W1[Dx:] of q1 (and of f, where it is its own
    network) on their own, so that they do not hide behind the state block, and d v -- `dv` (B, T, Di) where P is the model, else
    P["inputs"].grad -- per sequence, "inputs[b]" at the scale of the reference's d v[b].  The (t, b) rows that the reference has
    exactly zero (the last step always: nothing reads v[:, T - 1]; under a one-hot cotangent whatever the entry does not depend
    on) are taken out of their sequence and form one row of scale 0, whose first-clause bound is therefore ATOL alone."""
    Dx = p.case.Dx
    grad = lambda t: None if t is None or t.grad is None else t.grad.detach().double().cpu()
    other = None if P is p.model else {n: t for n, _, t in _pairs(p.model, P)}
    rows = []
    for name, par, ref in _pairs(p.model, P_ref):
        if name in ("q1.W0", "f.W0"):
            r, g = grad(ref), grad(par if other is None else other[name])
            r = torch.zeros_like(ref) if r is None else r
            g = torch.zeros_like(ref) if g is None else g.reshape(ref.shape)
            rows.append((name + "[Dx:]", float((g[Dx:] - r[Dx:]).abs().max()), max(float(r[Dx:].abs().max()), 1e-6)))
    ref = grad(P_ref["inputs"])
    ref = torch.zeros_like(P_ref["inputs"]) if ref is None else ref
    got = grad(P["inputs"]) if other is not None else (None if dv is None else dv.detach().double().cpu())
    d = ((torch.zeros_like(ref) if got is None else got) - ref).abs()
    zero = (ref == 0).all(-1)                                            # (B, T)
    assert bool(zero[:, T - 1].all())
    for b in range(B):
        if not bool(zero[b].all()):
            rows.append(("inputs[%d]" % b, float(d[b][~zero[b]].max()), float(ref[b].abs().max())))
    rows.append(("inputs[where the reference is exactly 0]", float(d[zero].max()), 0.0))
    return rows


def compare_inputs(p, P, dv, yardstick, subject=None):
    """compare() for input_rows: the product's (p.model's .grad and `dv`; or the oracle layout `subject`) against the fp64
    oracle's P under the same two clauses, the fp32 oracle's own error on the same block being the yardstick of the second;
    the block the reference has exactly zero is held to ATOL alone.  Under the random cotangent the reference's d v must be
    non-zero on every sequence, and so must its input rows."""
    rows = input_rows(p, p.model if subject is None else subject, P, dv)
    if p.case.hot is None:
        assert {n for n, _, _ in rows} >= {"inputs[%d]" % b for b in range(B)}, rows
        assert all(s > 1e-6 for n, _, s in rows if n.endswith("[Dx:]")), rows
    assert ("f.W0[Dx:]" in {n for n, _, _ in rows}) == (not p.case.boot) and rows[0][0] == "q1.W0[Dx:]"
    over = [r for r in rows if not r[1] <= RTOL * r[2] + ATOL]
    second = []
    if over:
        err32 = {n: e for n, e, _ in input_rows(p, yardstick(), P)}
        second = [(n, e, s, err32[n]) for n, e, s in over]
    bad = [r for r in second if r[2] == 0.0 or not r[1] <= K32 * r[3]]
    worst = max((r for r in rows if r[2] > 0.0), key=lambda r: r[1] / r[2])
    print("VJP %s, input rows and d v: worst error / largest entry %.3e (%s); error where the reference is exactly 0 %.3e; "
          "%d of %d blocks on the fp32 yardstick%s" % (
              p.case.id, worst[1] / worst[2], worst[0], rows[-1][1], len(over), len(rows),
              "".join("; %s err %.3e fp32-oracle err %.3e" % (n, e, e32) for n, e, _, e32 in second)))
    assert not bad, "input-gradient mismatch (name, max abs err, largest entry, fp32 oracle's own err): %s" % bad
    return rows


def fp32_share_over(rows32):
    """share of the tensors on which the fp32 oracle's own error is outside the first clause: the seed's fitness for a case"""
    return sum(1 for _, e, s in rows32 if not e <= RTOL * s + ATOL) / float(len(rows32))


def compare(p, P, yardstick):
    """the product's gradients (p.model's .grad) against the fp64 oracle's (P): first clause, else K32 x the fp32 oracle's own
    error from `yardstick()` -> P32, called only when a tensor needs it.  Prints the worst error / largest entry and returns
    the report {worst: (name, ratio), clause: 1 | 2, second: [(name, err, scale, err32)], tensors: n}; AssertionError naming
    every tensor that fails both clauses."""
    rows = grad_rows(p.model, p.model, P)
    worst = max(rows, key=lambda r: r[1] / r[2])
    report = {"worst": (worst[0], worst[1] / worst[2]), "clause": 1, "second": [], "tensors": len(rows)}
    over = [r for r in rows if not r[1] <= RTOL * r[2] + ATOL]
    bad = []
    if over:
        err32 = {n: e for n, e, _ in grad_rows(p.model, yardstick(), P)}
        report["clause"] = 2
        report["second"] = [(n, e, s, err32[n]) for n, e, s in over]
        bad = [r for r in report["second"] if not r[1] <= K32 * r[3]]
    print("VJP %s: worst error / largest entry %.3e (%s); clause %d; %d of %d tensors on the fp32 yardstick%s" % (
        p.case.id, report["worst"][1], report["worst"][0], report["clause"], len(over), len(rows),
        "".join("; %s err %.3e fp32-oracle err %.3e" % (n, e, e32) for n, e, _, e32 in report["second"])))
    assert not bad, "gradient mismatch (name, max abs err, largest entry, fp32 oracle's own err): %s" % bad
    return report


# ---- the cases -------------------------------------------------------------------------------------------------------------
FB0, FB2, DET = ("PSVO_TUNE_FILTER_BWD", 0), ("PSVO_TUNE_FILTER_BWD", 2), ("PSVO_TUNE_DETERMINISTIC", 1)
ALL3, ALL4 = ("lse", "Fm", "logW"), ("lse", "Fm", "Fs", "logW")
L2 = dict(layers=2)

# (a) the plain reverse filter, d lse only
A_CASES = [
    Case("fbs_scan_1_1", "AESMC", 16, 2, 1),
    Case("fbs_scan_1_2", "SVO", 100, 3, 2),
    Case("fbs_scan_4_1", "AESMC", 200, 4, 1),
    Case("fbs_scan_4_2", "SVO", 300, 2, 2),
    Case("filter_bwd_lpp", "AESMC", 17, 2, 1, tune=[FB0]),
    Case("filter_bwd_lpp", "SVO", 128, 3, 2, tune=[FB0]),
    Case("filter_bwd_persistent", "AESMC", 130, 2, 1, tune=[FB0]),
    Case("filter_bwd_persistent_atomics", "AESMC", 300, 3, 2, tune=[FB0]),
    Case("filter_bwd_persistent_deterministic", "AESMC", 130, 2, 1, tune=[FB0, DET]),
    Case("filter_bwd_nonbootstrap", "AESMC", 17, 2, 1, boot=False),
    Case("filter_bwd_nonbootstrap", "SVO", 130, 3, 2, boot=False),
    Case("filter_bwd_no_q2", "AESMC", 17, 2, 1, two_q=False),
    Case("filter_bwd_iwae", "IWAE", 17, 3, 1),
    Case("filter_bwd_two_layers", "AESMC", 17, 4, 1, **L2),
    Case("filter_bwd_two_layers", "AESMC", 130, 2, 2, **L2),
]
# (b) the plain reverse filter, all three cotangents
B_CASES = [
    Case("filter_bwd_lpp_ext", "AESMC", 17, 2, 1, cots=ALL3, tune=[FB0]),
    Case("filter_bwd_persistent_ext", "AESMC", 130, 3, 2, cots=ALL3, tune=[FB0]),
    Case("fbs_scan_ext", "AESMC", 17, 2, 1, cots=ALL3, tune=[FB2]),
    Case("fbs_scan_ext", "SVO", 130, 3, 2, cots=ALL3, tune=[FB2]),
    Case("fbs_scan_ext_default", "AESMC", 300, 4, 1, cots=ALL3),
    Case("filter_bwd_nonbootstrap_ext", "AESMC", 17, 2, 2, cots=ALL3, boot=False),
]
# (c) state-dependent scales: filter_cov_bwd_kernel (no bootstrap; bootstrap under FILTER_BWD 0) and the fcs_* scan
C_CASES = [Case(route, "AESMC", N, Dx, Dy, family="cov", cots=cots, boot=boot, tune=tune)
           for route, boot, tune in (("filter_cov_bwd_nonbootstrap", False, ()), ("filter_cov_bwd_persistent", True, [FB0]),
                                     ("fcs_scan", True, ()))
           for N, Dx, Dy in ((16, 2, 1), (100, 3, 2))
           for cots in (("lse",), ALL4)] + [
    Case("filter_cov_bwd_persistent_deterministic", "AESMC", 100, 3, 2, family="cov", cots=ALL4, tune=[FB0, DET]),
    Case("filter_cov_bwd_nonbootstrap_deterministic", "AESMC", 100, 2, 1, family="cov", cots=ALL4, boot=False, tune=[DET]),
]
# (d) the adaptive filter, decisions forced and mixed
D_CASES = [
    Case("filter_bwd_lpp_ad", "AESMC", 17, 2, 1, family="adaptive"),
    Case("filter_bwd_ad_persistent", "AESMC", 130, 3, 2, family="adaptive"),
]
# (e) the wide-observation kernels, Gaussian and count form each
_WIDE_SHAPES = [(3, 16, 2), (10, 100, 3)]                    # (Dy, N, Dx)
_MISSING_SHAPES = _WIDE_SHAPES + [(1, 16, 2), (2, 100, 3)]
E_CASES = (
    [Case("filter_wobs_static", "AESMC", N, Dx, Dy, family="wide", cots=ALL3, emission=em)
     for em in (GAUSS, COUNT) for Dy, N, Dx in _WIDE_SHAPES + [(32, 300, 4)]]
    + [Case("filter_wobs_static", "AESMC", 16, 2, 3, family="wide", cots=ALL3, emission=UNIT)]
    + [Case("filter_wobs_adaptive", "AESMC", N, Dx, Dy, family="wide_adaptive", emission=em)
       for em in (GAUSS, COUNT) for Dy, N, Dx in _WIDE_SHAPES]
    + [Case("filter_wobs_missing", "AESMC", N, Dx, Dy, family="missing", emission=em)
       for em in (COUNT, GAUSS) for Dy, N, Dx in _MISSING_SHAPES]
    + [Case("filter_wobs_missing_adaptive", "AESMC", N, Dx, Dy, family="missing_adaptive", emission=em)
       for em in (GAUSS, COUNT) for Dy, N, Dx in _MISSING_SHAPES]
    + [Case("filter_wobs_missing_ext", "PSVO", N, Dx, Dy, family="missing_bsim", cots=ALL3, emission=em)
       for em in (GAUSS, COUNT) for Dy, N, Dx in _MISSING_SHAPES]
)
# (f) the reverse backward simulations, random signed d score (B, N); the reverse filter behind each gets d Fm / d logW / d lse
F_CASES = (
    [Case("bsim_bwd_variant%d" % v, "PSVO", 17, Dx, 1, cots=("score",), tune=[("PSVO_TUNE_BSIM_BWD", v)])
     for v in (0, 1, 2, 3, 4) for Dx in (2, 3, 4)]
    + [Case("bsim_bwd_default", "PSVO", 130, 2, 1, cots=("score",), M=16),
       Case("bsim_bwd_two_layers", "PSVO", 17, 2, 1, cots=("score",), **L2),
       Case("bsim_cov", "PSVO", 17, 2, 1, family="cov", cots=("score",)),
       Case("bsim_cov_ws_deterministic", "PSVO", 17, 3, 2, family="cov", cots=("score",), tune=[DET]),
       Case("bsim_wobs_missing", "PSVO", 40, 3, 10, family="missing_bsim", cots=("score",), emission=COUNT),
       Case("bsim_wobs_missing", "PSVO", 64, 2, 1, family="missing_bsim", cots=("score",))]
)
# (g) PSVOwR, random d lseW (T, B): the two smallest shapes of the PSVOwR members of test_gpu_parity.CASES -- clusters of two and
# of four workgroups per sequence (psvo_bsimwr_blocks) --, N = 6 for the one-member launch that neither of them is, and the
# smallest PSVOwR member of COV_CASES
G_CASES = [
    Case("psvowr_bwd_cluster2", "PSVOwR", 8, 2, 1, cots=("lseW",), M=4, H=16),
    Case("psvowr_bwd_cluster4", "PSVOwR", 20, 3, 1, cots=("lseW",), M=4, H=32, boot=False, two_q=False),
    Case("psvowr_bwd_one_member", "PSVOwR", 6, 2, 1, cots=("lseW",), M=4, H=16),
    Case("bsimwr_cov", "PSVOwR", 8, 2, 1, family="cov", cots=("lseW",), M=4, H=16),
    Case("bsimwr_cov_ws_deterministic", "PSVOwR", 8, 2, 1, family="cov", cots=("lseW",), M=4, H=16, tune=[DET]),
]
# (i) the input-driven filter (FLAGS.Di): the only route that turns a cotangent into rows d hb[t, b, :], which torch folds into
# d W1[Dx:] and d v.  (obj, N, Dx, Dy, H, Di, ...) as tests/exo_reference.CASES
_INPUT_SHAPES = [
    ("AESMC", 16, 2, 1, 16, 1, {}),                              # smallest everything
    ("AESMC", 16, 2, 1, 16, 16, {}),                             # Di = H: W1[Dx:] is square, no unit of d hb hides in the projection
    ("SVO", 16, 2, 3, 64, 2, dict(boot=False)),                  # one wave stages 2 H = 128 bias words; separate f (dhb_f)
    ("SVO", 40, 3, 2, 32, 3, dict(boot=False)),                  # partly filled wave
    ("SVO", 17, 2, 2, 24, 2, dict(boot=False)),                  # H = 24 at kernel width 32: padded columns of hb / d hb
    ("IWAE", 24, 4, 17, 64, 2, dict(two_q=False)),               # reverse step without an inner barrier
    ("AESMC", 100, 3, 10, 32, 2, dict(emission=COUNT)),
]


def _input_case(route, family, obj, N, Dx, Dy, H, Di, kw, **flags):
    return Case(route, obj, N, Dx, Dy, family=family, H=H, flags=dict(Di=Di, **flags), **kw)


I_CASES = [_input_case("filter_wobs_input", "input", *s) for s in _INPUT_SHAPES] + [
    _input_case("filter_wobs_input", "input", *_INPUT_SHAPES[3], missing_obs=True)]     # never-observed column stays exactly 0
# (j) the same under adaptive resampling, decisions forced and mixed: the !rs_here chain through d lnw besides
J_CASES = [_input_case("filter_wobs_input_adaptive", "input_adaptive", *_INPUT_SHAPES[i]) for i in (0, 1, 3, 4, 6)]
# (k) PSVO on wide observations (FLAGS.BSim_wide_obs, Dy 3..32): the static compilation of the reverse backward simulation and
# the _ext reverse filter behind it.  (N, Dx, Dy, M, H, ...) as tests/test_gpu_wobs_bsim.CASES
_WIDE_BSIM = dict(family="wide", cots=("score",), flags=dict(BSim_wide_obs=True))
K_CASES = [Case("bsim_wobs_static", "PSVO", N, Dx, Dy, M=M, H=H, **{**_WIDE_BSIM, **kw}) for N, Dx, Dy, M, H, kw in (
    (16, 2, 3, 4, 16, {}),
    (40, 3, 10, 8, 32, dict(boot=False)),
    (24, 3, 32, 32, 64, {}),
    (130, 4, 17, 4, 64, dict(boot=False)),
    (24, 2, 5, 8, 32, dict(two_q=False)),
    (16, 2, 10, 8, 32, dict(emission=UNIT)),
    (40, 3, 10, 8, 32, dict(emission=COUNT)),
    # the _ext reverse filter gets the backward simulation's gradients and a direct cotangent together
    (16, 2, 3, 4, 16, dict(cots=("score", "lse", "Fm", "logW"))),
)]
# (h) one-hot cotangents at (t0, B - 1), t0 in {0, 1, T - 1}: a single misplaced read moves the whole gradient
_FIRST_MISSING_COUNT = next(c for c in E_CASES if c.family == "missing" and c.emission == COUNT)
H_CASES = [c.one_hot_at(t0) for c in (A_CASES[0], C_CASES[0], D_CASES[0], _FIRST_MISSING_COUNT, G_CASES[0], I_CASES[0], J_CASES[0])
           for t0 in (0, 1, T - 1)]

CASES = A_CASES + B_CASES + C_CASES + D_CASES + E_CASES + F_CASES + G_CASES + I_CASES + J_CASES + K_CASES + H_CASES
assert len({c.id for c in CASES}) == len(CASES)
