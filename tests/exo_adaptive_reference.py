"""fp64 reference of adaptive resampling under exogenous inputs (FLAGS.Di with FLAGS.resample_ess and FLAGS.resample_ess_inputs;
psvo_filter_forward_wobs_input_adaptive): tests/exo_reference.py's filter loop with the decision of tests/adaptive_reference.py,
and nothing new.  The objective, its input-driven q1 / f and the emission that leaves NaN entries out are exo_reference's; the
effective sample size and the rule are adaptive_reference's (ess_of, decide).  Per step: the multinomial draw is made and returned
whatever the decision; step t + 1 starts from the drawn ancestors with weight -log N where the sequence resampled, else from the
particles themselves with the normalised weight logW_t - lse_t, and in both cases meets v_t.  noise["rs_f"] (T, B), non-zero =
resample, forces the decisions; decisions and indices are constants of the reverse pass.  A helper, not a test.
"""
import math

import torch

from oracle import psvo_oracle as O
from tests import adaptive_reference as AR
from tests import exo_reference as ER
from tests import missing_reference as MR

TAU = AR.TAU
# the cases of exo_reference that resample at all (SVO / AESMC): the smallest shape, ONE wave staging 2 H = 128 bias words, the
# partly filled wave with a separate f, eight waves at every limit, and T = 60 for both halves of the row buffer many times
RUNS = [(c, d, "") for c, d in ER.CASES if c[0] in ("SVO", "AESMC")]
run_id = ER.run_id


def forced(T, B, seed=11):
    """the fixed mixed pattern of the forced-decision tests, (T, B) int32: about half of the steps resample, and every sequence
    holds both a resampled and a kept step (tests/test_exo_adaptive_host.py asserts it)"""
    g = torch.Generator().manual_seed(seed)
    rs = (torch.rand(T, B, generator=g) < 0.5).to(torch.int32)
    rs[0, :], rs[1, :] = 1, 0
    return rs


def smc(o, obs, v, noise, ess_frac):
    """exo_reference.smc with adaptive_reference's decision; v (B,T,Di)"""
    B, T, _ = obs.shape
    N = o.n_particles
    q0, q1, f = o.q0, o.q1, o.f
    eps, u, idx_tf, rs_tf = noise["eps_f"], noise.get("u_f"), noise.get("idx_f"), noise.get("rs_f")
    logN = math.log(float(N))
    preprocessed_X0, preprocessed_obs = o.preprocess_obs(obs)

    def step(t, feed):          # (exo_reference.smc's step)
        d1 = q0 if t == 0 else q1
        if o.use_2_q:
            X_t, q_lp, f_lp = o.sample_from_2_dist(d1, o.q2, feed, preprocessed_obs[t], eps[t])
        else:
            X_t, q_lp = d1.sample_and_log_prob(feed, eps[t])
        if not (o.use_bootstrap and o.use_2_q):
            f_lp = f.log_prob(feed, X_t)
        g_lp = o.g.log_prob(X_t, obs[:, t])
        return X_t, f_lp + g_lp - q_lp

    Xs, X_ancs, log_Ws, idxs, rss, esss = [], [], [], [], [], []
    start, log_norm_W = None, None
    for t in range(T):
        X_t, log_alpha = step(t, preprocessed_X0 if t == 0 else (start, v[:, t - 1]))
        log_W = log_alpha - logN if t == 0 else log_alpha + log_norm_W
        X_anc, idx = o.resample_X(X_t, log_W, u=None if u is None else u[t], idx=None if idx_tf is None else idx_tf[t],
                                  sample_size=N, resample_particles=True)
        ess = AR.ess_of(log_W.detach())
        rs = AR.decide(ess, ess_frac, N) if rs_tf is None else (rs_tf[t] != 0)          # (B,)
        start = torch.where(rs[None, :, None], X_anc, X_t)
        log_norm_W = torch.where(rs[None, :], torch.full_like(log_W, -logN), log_W - O.logsumexp(log_W, 0))
        Xs.append(X_t); X_ancs.append(X_anc); log_Ws.append(log_W); idxs.append(idx); rss.append(rs); esss.append(ess)
    X_prevs, X_ancestors, log_Ws = torch.stack(Xs), torch.stack(X_ancs), torch.stack(log_Ws)
    z = O.logsumexp(log_Ws, 1).sum(0).mean()
    return z, {"Xs": X_ancestors.permute(2, 0, 1, 3), "X_prevs": X_prevs, "X_ancestors": X_ancestors, "log_Ws": log_Ws,
               "idx_f": torch.stack(idxs), "rs_f": torch.stack(rss), "ess": torch.stack(esss)}


def run(model, FLAGS, obj, obs, v, noise, teacher=None, dtype=torch.float64, ess_frac=TAU):
    o = ER.objective(model.export_reference_layout(dtype), FLAGS, obj)
    with torch.no_grad():
        return smc(o, obs.to(dtype).cpu(), v.to(dtype).cpu(), MR._cast({**noise, **(teacher or {})}, dtype), ess_frac)


def grads(model, FLAGS, obj, obs, v, noise, teacher, dtype=torch.float64, ess_frac=TAU):
    """ELBO, the reference's parameters with .grad, and d ELBO / d v"""
    P = MR.require_grad(model.export_reference_layout(dtype))
    v = v.to(dtype).cpu().clone().requires_grad_(True)
    z, _ = smc(ER.objective(P, FLAGS, obj), obs.to(dtype).cpu(), v, MR._cast({**noise, **teacher}, dtype), ess_frac)
    z.backward()
    return z.detach(), P, v.grad
