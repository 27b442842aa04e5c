"""fp64 reference of adaptive resampling (FLAGS.resample_ess; psvo_filter_forward_adaptive): the oracle's filter objectives with
SMC overridden by the one definition the kernels, the header and DESIGN.md share.  With w_n = exp(logW_t[n] - max) over the N
particles of a sequence,

    ESS_t = (sum w_n)^2 / sum w_n^2        (here: exp(2 lse(logW_t) - lse(2 logW_t))),
    the sequence resamples at step t  iff  not (ESS_t >= ess_frac * N)        (a NaN ESS resamples).

Every step makes the multinomial draw (noise["u_f"], or noise["idx_f"] teacher-forced) and returns the gathered particles as
X_ancestors; only what step t + 1 starts from depends on the decision -- the drawn ancestors with weight -log N, or the particles
themselves with the normalised weight logW_t - lse_t.  noise["rs_f"] (T, B), non-zero = resample, forces the decisions.  Decisions
and indices are constants of the reverse pass.

The class runs in the dtype of its parameters: fp64 is the reference, an fp32 CPU run the yardstick of what the arithmetic type
costs on a case.  run_oracle / oracle_grads / replay_with_hip mirror tests/helpers.py and tests/count_reference.py.  A helper, not
a test; only tests import it.
"""
import math

import torch

from oracle import psvo_oracle as O
from tests import helpers as Hh


TAU = 0.5          # the threshold of the free-running tests
# The largest |ESS_fp32 - ESS_fp64| / N of this reference over CASES, fp32 on the CPU with the fp64 run's draws and decisions
# (measured 7.71e-07, rounded up; tests/test_adaptive_host.py holds the measurement to it, profiles/adaptive_resampling.md records
# it).  The GPU tests allow 4 x this: the kernel's v_exp_f32 against libm.
ESS_GAP32 = 7.8e-07

# The cases of tests/test_gpu_adaptive.py: the smallest shapes that reach each kernel form.
# (objective, B, T, N, Dx, Dy, hidden layers, bootstrap, two_q, further flags, model seed)
# The further flags and the seed are chosen on the CPU (tests/test_adaptive_host.py checks it) so that the fp64 reference alone, free
# running at TAU, resamples at between 10 % and 90 % of each case's (step, sequence) pairs: `calm` scales the MLPs' output layers
# (see setup) and the *_sigma_min flags floor the scales; helpers.perturb_'s random model as it stands has every step of the wider
# cases collapse onto a few particles (ESS / N <= 0.3), and no decision would ever be "keep".
_WIDE = dict(calm=0.5, q2_sigma_min=4.0, g_sigma_min=4.0)
CASES = [
    ("AESMC", 2, 6, 16, 2, 1, "32", True, True, {}, 3),               # four lanes per particle (lpp), forward and reverse
    ("AESMC", 2, 6, 16, 2, 1, "32", False, True, {}, 3),              # ... the other three wirings
    ("AESMC", 2, 6, 16, 2, 1, "32", True, False, {}, 3),
    ("AESMC", 2, 6, 16, 2, 1, "32", False, False, dict(calm=0.5), 4),
    ("AESMC", 3, 7, 100, 4, 2, "64", True, True, _WIDE, 4),           # one lane per particle, <= 256 threads, padded lanes
    ("AESMC", 3, 7, 100, 4, 2, "64", True, True, dict(_WIDE, poisson_emission=True), 4),
    ("AESMC", 2, 6, 320, 3, 2, "32", True, True, _WIDE, 6),           # the 512-thread kernels (deterministic mode: DET form)
    ("AESMC", 2, 6, 16, 2, 1, "32,32", True, True, dict(calm=0.5), 4),    # two hidden layers, lpp
    ("AESMC", 2, 6, 192, 2, 1, "32,32", True, True, _WIDE, 4),        # two hidden layers, one lane per particle
    ("SVO", 2, 6, 16, 2, 1, "32", True, True, {}, 3),                 # the bi-LSTM encoder in front
]
case_id = lambda c: "-".join(str(v) for v in c[:9]) + ("-poisson" if c[9].get("poisson_emission") else "")


def setup(case, device="cpu", seed=None, **extra):
    """tests/test_gpu_parity.py::_setup for an adaptive case, on `device`: (FLAGS, model, smc, obs (B,T,Dy) fp64, noise in the
    reference's layout).  FLAGS.resample_ess = TAU unless `extra` says otherwise."""
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    from psvo_amd.SMC.SVO import SVO
    obj, B, T, N, Dx, Dy, hs, bootstrap, two_q, more, model_seed = case
    seed = model_seed if seed is None else seed
    kw = dict(Dx=Dx, Dy=Dy, n_particles=N, batch_size=B, time=T, q0_layers=hs, q1_layers=hs, q2_layers=hs, f_layers=hs,
              g_layers=hs, y_smoother_Dhs="8", X0_smoother_Dhs="8", use_bootstrap=bootstrap, use_2_q=two_q, resample_ess=TAU)
    kw.update(more)
    kw.update(extra)
    calm = kw.pop("calm", 1.0)
    FLAGS = Hh.make_flags(obj, **kw)
    torch.manual_seed(seed)
    model = Hh.perturb_(SSM(FLAGS))
    if calm != 1.0:
        # he_normal output layers send particles that differ by a scale or two to means that differ by ten: every step's weights
        # then collapse onto a few particles and no case would ever see a balanced step.  `calm` scales the output layers down.
        with torch.no_grad():
            for name, p in model.named_parameters():
                if name.endswith("mu_kernel"):
                    p.mul_(calm)
    model = model.to(device)
    smc = {"SVO": SVO, "AESMC": AESMC}[obj](model, FLAGS)
    g = torch.Generator().manual_seed(100 + seed)
    obs = torch.randn(B, T, Dy, generator=g, dtype=torch.float64) * 1.5
    noise = O.make_noise(Hh.oracle_flags(FLAGS, obj), B, T, seed=1234 + seed)
    return FLAGS, model, smc, obs, noise


def ess_of(log_W):
    """(N, B) log-weights -> (B,) effective sample size"""
    return torch.exp(2.0 * O.logsumexp(log_W, 0) - O.logsumexp(2.0 * log_W, 0))


def decide(ess, ess_frac, N):
    """the rule: (B,) bool, True = resample"""
    return ~(ess >= ess_frac * N)


class _Adaptive:
    """mixin over OracleSVO / OracleAESMC: SMC with the per-(step, sequence) decision"""
    ess_frac = 0.5

    def SMC(self, obs, noise):
        B, T, _ = obs.shape
        N = self.n_particles
        q0, q1, f = self.q0, self.q1, self.f
        eps, u, idx_tf, rs_tf = noise["eps_f"], noise.get("u_f"), noise.get("idx_f"), noise.get("rs_f")
        logN = math.log(float(N))

        preprocessed_X0, preprocessed_obs = self.preprocess_obs(obs)
        self.preprocessed_X0, self.preprocessed_obs = preprocessed_X0, preprocessed_obs

        def step(t, feed):          # (OracleSVO.SMC's step)
            d1 = q0 if t == 0 else q1
            if self.use_2_q:
                X_t, q_lp, f_lp = self.sample_from_2_dist(d1, self.q2, feed, preprocessed_obs[t], eps[t])
            else:
                X_t, q_lp = d1.sample_and_log_prob(feed, eps[t])
            if not (self.use_bootstrap and self.use_2_q):
                f_lp = f.log_prob(feed, X_t)
            g_lp = self.g.log_prob(X_t, obs[:, t])
            return X_t, f_lp + g_lp - q_lp

        Xs, X_ancs, log_Ws, idxs, rss, esss = [], [], [], [], [], []
        feed, log_norm_W = preprocessed_X0, None
        for t in range(T):
            X_t, log_alpha = step(t, feed)
            log_W = log_alpha - logN if t == 0 else log_alpha + log_norm_W
            X_anc, idx = self.resample_X(X_t, log_W, u=None if u is None else u[t],
                                         idx=None if idx_tf is None else idx_tf[t], sample_size=N)
            ess = ess_of(log_W.detach())
            rs = decide(ess, self.ess_frac, N) if rs_tf is None else (rs_tf[t] != 0)          # (B,)
            feed = torch.where(rs[None, :, None], X_anc, X_t)
            log_norm_W = torch.where(rs[None, :], torch.full_like(log_W, -logN), log_W - O.logsumexp(log_W, 0))
            Xs.append(X_t); X_ancs.append(X_anc); log_Ws.append(log_W); idxs.append(idx); rss.append(rs); esss.append(ess)
        self.idx_f, self.rs_f, self.ess = torch.stack(idxs), torch.stack(rss), torch.stack(esss)
        return torch.stack(Xs), torch.stack(X_ancs), torch.stack(log_Ws)

    def get_log_ZSMC(self, obs, noise):
        z, log = super().get_log_ZSMC(obs, noise)
        log["rs_f"], log["ess"] = self.rs_f, self.ess          # (T, B) bool, (T, B)
        return z, log


class AdaptiveSVO(_Adaptive, O.OracleSVO):
    pass


class AdaptiveAESMC(_Adaptive, O.OracleAESMC):
    pass


OBJECTIVES = {"SVO": AdaptiveSVO, "AESMC": AdaptiveAESMC}


def objective(P, FLAGS, obj, ess_frac=None):
    o = OBJECTIVES[obj](P, Hh.oracle_flags(FLAGS, obj))
    o.ess_frac = float(FLAGS.resample_ess if ess_frac is None else ess_frac)
    return o


def _cast(noise, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in noise.items()}


def run_oracle(model, FLAGS, obj, obs, noise, teacher=None, dtype=torch.float64, ess_frac=None):
    o = objective(model.export_reference_layout(dtype), FLAGS, obj, ess_frac)
    with torch.no_grad():
        z, log = o.get_log_ZSMC(obs.to(dtype).cpu(), _cast({**noise, **(teacher or {})}, dtype))
    return z, log


def hip_teacher(log):
    """what the HIP run drew and decided, in the reference's layouts: idx_f (T, N, B) int64, rs_f (T, B) int64"""
    return {"idx_f": log["filter"]["idx"].permute(0, 2, 1).cpu().long(), "rs_f": log["filter"]["rs"].cpu().long()}


def replay_with_hip(model, FLAGS, obj, obs, noise, log, dtype=torch.float64):
    """the reference with the HIP run's indices AND decisions teacher-forced: (z_ref, ref_log).  ref_log["ess"] is then the
    reference's ESS on the replayed weights, and decide(ref_log["ess"], tau, N) the rule's own decision there."""
    return run_oracle(model, FLAGS, obj, obs, noise, teacher=hip_teacher(log), dtype=dtype)


def oracle_grads(model, FLAGS, obj, obs, noise, teacher, dtype=torch.float64):
    """ELBO and the autograd gradients of the reference in `dtype` (tests/test_gpu_parity.py::_oracle_grads)"""
    P = model.export_reference_layout(dtype)

    def req(x):
        if torch.is_tensor(x):
            x.requires_grad_(True)
        elif isinstance(x, dict):
            [req(v) for v in x.values()]
        elif isinstance(x, (list, tuple)):
            [req(v) for v in x]
    req(P)
    o = objective(P, FLAGS, obj)
    z, _ = o.get_log_ZSMC(obs.to(dtype).cpu(), _cast({**noise, **teacher}, dtype))
    z.backward()
    return z.detach(), P
