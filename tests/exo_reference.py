"""fp64 reference of exogenous inputs (FLAGS.Di; psvo_filter_forward_wobs_input): a stand-alone restatement of the filter loop,
since the oracle has no transformation that changes with time.  Everything that does not see the input is the oracle's own, taken
through tests/missing_reference.objective (the emission that leaves NaN entries out, the zero-filled proposal inputs, q0, q2, the
encoders, resample_X and sample_from_2_dist); what is restated here is

  * InputMVN: the distribution of q1 / f with a first layer W1 (Dx + Di, H) on concat[x, v],
        MLP(x; v) = relu(x W1[:Dx] + (b1 + v W1[Dx:])) W2 + b2            (form "hoisted": b1 + v W1[Dx:] rounded ONCE, as the kernels)
                  = relu(concat[x, v] W1 + b1) W2 + b2                    (form "concat": the definition)
    A plain tensor as its input (the X0 feature at t = 0) means a zero input;
  * smc(): OracleSVO.SMC line for line, with the feed of step t >= 1 being (X_anc, v_{t-1}): x_t ~ f(. | x_{t-1}, v_{t-1}).

inputs(): the seeded standard normals the tests use, different at every step and sequence.  A helper, not a test.
"""
import math

import torch

from oracle import psvo_oracle as O
from tests import helpers as Hh
from tests import missing_reference as MR

SCALE = 1.0          # input scale of the GPU cases (tests/test_exo_host.py asserts the separation condition at this scale)


CASES = [
    # ((objective, B, T, N, M, Dx, Dy, H, bootstrap, two_q), Di)
    (("AESMC", 2, 5, 16, 1, 2, 1, 16, True, True), 1),         # smallest everything, Dy = 1
    (("SVO", 2, 5, 16, 1, 2, 3, 64, False, True), 2),          # one wave of 64 lanes staging 2 * 64 bias words
    (("SVO", 2, 6, 40, 1, 3, 2, 32, False, True), 3),          # separate f, partly filled wave
    (("IWAE", 2, 5, 24, 1, 4, 17, 64, True, False), 2),        # no resampling: the reverse step without an inner barrier
    (("AESMC", 1, 4, 512, 1, 4, 32, 32, False, True), 4),      # eight waves, every limit
    (("SVO", 1, 60, 32, 1, 3, 10, 32, True, True), 1),         # both halves of the row buffer many times
]
# (case, Di, variant): every case plainly, case 3 again under --missing_obs with MR.mask, case 2 again under --count_emission
RUNS = [(c, d, "") for c, d in CASES] + [(CASES[2][0], CASES[2][1], "missing"), (CASES[1][0], CASES[1][1], "count")]
run_id = lambda r: "-".join(map(str, r[0])) + "-Di%d" % r[1] + ("-" + r[2] if r[2] else "")


def run_flags(run, **extra):
    """the flags of a run, as tests/test_gpu_parity._setup builds them"""
    (obj, B, T, N, M, Dx, Dy, H, bootstrap, two_q), Di, variant = run
    hs = str(H)
    kw = dict(Dx=Dx, Dy=Dy, n_particles=N, n_particles_for_BSim_proposal=M, batch_size=B, time=T,
              q0_layers=hs, q1_layers=hs, q2_layers=hs, f_layers=hs, g_layers=hs,
              y_smoother_Dhs="8", X0_smoother_Dhs="8", use_bootstrap=bootstrap, use_2_q=two_q, Di=Di)
    if variant == "missing":
        kw["missing_obs"] = True
    if variant == "count":
        kw["count_emission"] = True
    kw.update(extra)
    return Hh.make_flags(obj, **kw)


def observations(run, seed, obs=None):
    """the observations of a run: _setup's seeded normals (or `obs`, when the caller has them), counts under the count variant,
    knocked out by MR.mask under the missing variant"""
    from tests.count_reference import counts
    (_, B, T, _, _, _, Dy, _, _, _), _, variant = run
    if obs is None:
        obs = torch.randn(B, T, Dy, generator=torch.Generator().manual_seed(100 + seed), dtype=torch.float64) * 1.5
    if variant == "count":
        obs = counts(B, T, Dy, 100 + seed)
    if variant == "missing":
        obs = MR.knock_out(obs, MR.mask(B, T, Dy, seed)[0])
    return obs


def cpu_setup(run, seed):
    """the model, data and draws of a GPU run, on the host: (FLAGS, model, obs, v, noise), seeded as tests/test_gpu_parity._setup"""
    from psvo_amd.model import SSM
    (obj, B, T, _, _, _, _, _, _, _), Di, _ = run
    FLAGS = run_flags(run)
    torch.manual_seed(seed)
    model = Hh.perturb_(SSM(FLAGS))
    noise = O.make_noise(Hh.oracle_flags(FLAGS, obj), B, T, seed=1234 + seed)
    return FLAGS, model, observations(run, seed), inputs(B, T, Di, seed), noise


def inputs(B, T, Di, seed, scale=SCALE):
    g = torch.Generator().manual_seed(9000 + seed)
    return torch.randn(B, T, Di, generator=g, dtype=torch.float64) * scale


class InputMVN:
    """OracleMVN (state-independent scale) whose transformation takes (x, v); x alone means v = 0"""

    def __init__(self, p, Dx, form="hoisted"):
        assert len(p["layers"]) == 1 and p.get("sigma") is None and form in ("hoisted", "concat")
        self.p, self.Dx, self.form = p, Dx, form

    def mean(self, Input):
        x, v = Input if isinstance(Input, tuple) else (Input, None)
        W1, b1 = self.p["layers"][0]
        Dx = self.Dx
        if v is None:
            v = x.new_zeros(x.shape[:-1] + (W1.shape[0] - Dx,))
        if self.form == "concat":
            v = v.expand(x.shape[:-1] + (v.shape[-1],))
            h = torch.relu(torch.cat([x, v], dim=-1) @ W1 + b1)
        else:
            h = torch.relu(x @ W1[:Dx] + (b1 + v @ W1[Dx:]))
        W, b = self.p["mu"]
        return h @ W + b

    def mean_and_sigma(self, Input):
        return self.mean(Input), O.get_sigma(self.p)

    def sigma(self, Input=None):
        return O.get_sigma(self.p)

    def log_prob(self, Input, output):
        mu, s = self.mean_and_sigma(Input)
        return O.diag_log_prob(output, mu, s)

    def sample_and_log_prob(self, Input, eps):
        mu, s = self.mean_and_sigma(Input)
        x = mu + s * eps
        return x, O.diag_log_prob(x, mu, s)


def objective(P, FLAGS, obj, form="hoisted"):
    """missing_reference.objective with q1 / f taking the input"""
    Dx = FLAGS.Dx
    first = lambda p: {**p, "layers": [(p["layers"][0][0][:Dx], p["layers"][0][1])]}
    # (the oracle's own constructor only wraps the parameter dicts; its q1 / f are replaced below)
    o = MR.objective({**P, "q1": first(P["q1"]), **({"f": first(P["f"])} if "f" in P else {})}, FLAGS, obj)
    o.q1 = InputMVN(P["q1"], Dx, form)
    o.f = o.q1 if o.use_bootstrap else InputMVN(P["f"], Dx, form)
    return o


def smc(o, obs, v, noise):
    """OracleSVO.SMC (oracle/psvo_oracle.py) with input-driven q1 / f; v (B,T,Di)"""
    B, T, _ = obs.shape
    N = o.n_particles
    q0, q1, f = o.q0, o.q1, o.f
    eps, u, idx_tf = noise["eps_f"], noise.get("u_f"), noise.get("idx_f")
    logN = math.log(float(N))
    preprocessed_X0, preprocessed_obs = o.preprocess_obs(obs)

    def step(t, feed):
        d1 = q0 if t == 0 else q1
        if o.use_2_q:
            X_t, q_lp, f_lp = o.sample_from_2_dist(d1, o.q2, feed, preprocessed_obs[t], eps[t])
        else:
            X_t, q_lp = d1.sample_and_log_prob(feed, eps[t])
        if not (o.use_bootstrap and o.use_2_q):
            f_lp = f.log_prob(feed, X_t)
        g_lp = o.g.log_prob(X_t, obs[:, t])
        return X_t, f_lp + g_lp - q_lp

    Xs, X_ancs, log_Ws, idxs = [], [], [], []
    X_anc, log_norm_W = None, None
    for t in range(T):
        X_t, log_alpha = step(t, preprocessed_X0 if t == 0 else (X_anc, v[:, t - 1]))
        log_W = log_alpha - logN if t == 0 else log_alpha + log_norm_W
        X_anc, idx = o.resample_X(X_t, log_W, u=None if u is None else u[t], idx=None if idx_tf is None else idx_tf[t],
                                  sample_size=N, resample_particles=o.resample_particles)
        log_norm_W = log_W - O.logsumexp(log_W, 0)
        if o.resample_particles:
            log_norm_W = torch.full_like(log_W, -logN)
        Xs.append(X_t); X_ancs.append(X_anc); log_Ws.append(log_W); idxs.append(idx)
    idx_f = None if idxs[0] is None else torch.stack(idxs)
    X_prevs, X_ancestors, log_Ws = torch.stack(Xs), torch.stack(X_ancs), torch.stack(log_Ws)
    z = O.logsumexp(log_Ws, 1).sum(0).mean()
    return z, {"Xs": X_ancestors.permute(2, 0, 1, 3), "X_prevs": X_prevs, "X_ancestors": X_ancestors, "log_Ws": log_Ws,
               "idx_f": idx_f}


def run(model, FLAGS, obj, obs, v, noise, teacher=None, dtype=torch.float64, form="hoisted", P=None):
    o = objective(model.export_reference_layout(dtype) if P is None else P, FLAGS, obj, form)
    with torch.no_grad():
        return smc(o, obs.to(dtype).cpu(), v.to(dtype).cpu(), MR._cast({**noise, **(teacher or {})}, dtype))


def grads(model, FLAGS, obj, obs, v, noise, teacher, dtype=torch.float64):
    """ELBO, the reference's parameters with .grad, and d ELBO / d v"""
    P = MR.require_grad(model.export_reference_layout(dtype))
    v = v.to(dtype).cpu().clone().requires_grad_(True)
    z, _ = smc(objective(P, FLAGS, obj), obs.to(dtype).cpu(), v, MR._cast({**noise, **teacher}, dtype))
    z.backward()
    return z.detach(), P, v.grad


def replay_with_hip_indices(model, FLAGS, obj, obs, v, noise, log):
    """missing_reference.replay_with_hip_indices on this reference"""
    o = objective(model.export_reference_layout(torch.float64), FLAGS, obj)
    o.draw_log = []
    nz = dict(noise)
    nz.update(Hh.hip_indices(log, obj))
    with torch.no_grad():
        z, ref = smc(o, obs.double().cpu(), v.double().cpu(), nz)
    draws = off = 0
    worst = 0.0
    for log_W, u, idx in o.draw_log:
        d = O.draw_distance(log_W, u, idx)
        draws += d.numel()
        off += int((d > 0).sum())
        worst = max(worst, float(d.max()))
    return z, ref, {"draws": draws, "off": off, "worst": worst}
