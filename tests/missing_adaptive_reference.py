"""Cases and reference of adaptive resampling on missing observations (FLAGS.missing_obs with FLAGS.resample_ess and
FLAGS.resample_ess_missing_obs; psvo_filter_forward_wobs_missing_adaptive / psvo_filter_backward_wobs_missing_adaptive).

The fp64 reference is a composition of what exists and nothing else: tests/adaptive_reference.py's objective (its SMC does not
depend on Dy or on the emission), its emission wrapped in missing_reference.MissingEmission (around count_reference.CountEmission
for the count cases) and its preprocess_obs fed missing_reference.zero_filled(obs).  The mask is missing_reference.mask with the
case's seed.  A helper, not a test; only tests and tools import it.
"""
import torch

from tests import adaptive_reference as AR
from tests import count_reference as CR
from tests import missing_reference as MR
from tests.wobs_adaptive_reference import _W

# The largest |ESS_fp32 - ESS_fp64| / N of this reference over CASES, fp32 on the CPU with the fp64 run's draws and decisions
# (measured 1.79e-06 on the unit-normal-around-the-rate case, rounded up; tests/test_missing_adaptive_host.py holds the measurement
# to it, profiles/missing_adaptive.md records it).  The GPU tests allow 4 x this: the kernel's v_exp_f32 against libm.
ESS_GAP32_MISSING = 1.8e-06

# (objective, B, T, N, Dx, Dy, hidden layers, bootstrap, two_q, further flags, seed, threshold)
# The smallest shapes that reach each form of the kernels.  Flags, seed and threshold are chosen on the CPU with the fp64
# reference alone, free running, so that it resamples at between 10 % and 90 % of the (step, sequence) pairs and never comes
# closer to its threshold than 100 x the GPU's ESS tolerance (tests/test_missing_adaptive_host.py checks both).
CASES = [
    ("AESMC", 2, 6, 16, 2, 1, "16", True, True, dict(calm=0.5), 7, 0.5),                      # Dy = 1, one wave
    ("SVO", 2, 7, 40, 3, 2, "32", False, True, _W(0.5, g=4.0), 3, 0.5),                       # Dy = 2, encoder, own f
    ("AESMC", 2, 6, 16, 2, 3, "16", True, True, dict(calm=0.5), 5, 0.5),                      # the smallest wide Dy
    ("AESMC", 2, 7, 100, 3, 10, "32", False, True, _W(0.25, g=8.0), 4, 0.25),                 # padded lanes, own f
    ("AESMC", 2, 6, 130, 3, 17, "64", True, False, _W(0.5, g=4.0), 5, 0.5),                   # odd Dy, 3 waves, bootstrap, no q2
    ("AESMC", 1, 5, 512, 4, 32, "32", False, True, _W(0.25, g=8.0), 3, 0.25),                 # every limit
    ("AESMC", 2, 6, 40, 2, 10, "32", True, True, _W(0.5, count_emission=True), 4, 0.5),       # counts
    ("AESMC", 2, 6, 40, 2, 2, "32", True, True, _W(0.5, count_emission=True), 8, 0.5),        # counts at a plain width
    ("AESMC", 2, 6, 40, 2, 10, "32", True, True, _W(0.5, g=4.0, poisson_emission=True), 7, 0.5),
    ("SVO", 1, 40, 32, 3, 10, "32", True, True, _W(0.5, g=4.0), 5, 0.5),                      # a long sequence
]
GAP_CASE = 4        # bootstrap without q2: a step with nothing observed behind a resampled one has ESS = N


def case_id(c):
    tag = "-poisson" if c[9].get("poisson_emission") else "-count" if c[9].get("count_emission") else ""
    return "-".join(str(v) for v in c[:9]) + tag


def is_count(case):
    return bool(case[9].get("count_emission"))


def setup(case, device="cpu", knock=True, **extra):
    """AR.setup for a case with FLAGS.missing_obs, FLAGS.resample_ess = the case's threshold and FLAGS.resample_ess_missing_obs
    (unless `extra` says otherwise): (FLAGS, model, smc, obs (B,T,Dy) fp64 with NaN at the mask, noise, (miss, t_all, e_never)).
    Count cases get count observations.  knock=False: nothing is missing."""
    seed, tau = case[10], case[11]
    kw = dict(resample_ess=tau, missing_obs=True, resample_ess_missing_obs=True)
    kw.update(extra)
    FLAGS, model, smc, obs, noise = AR.setup(case[:11], device, **kw)
    B, T, Dy = case[1], case[2], case[5]
    if is_count(case):
        obs = CR.counts(B, T, Dy, 100 + seed).double()
    m = MR.mask(B, T, Dy, seed)
    if knock:
        obs = MR.knock_out(obs, m[0])
    return FLAGS, model, smc, obs, noise, m


def objective(P, FLAGS, case, ess_frac=None):
    o = AR.objective(P, FLAGS, case[0], ess_frac)
    o.g = MR.MissingEmission(CR.CountEmission(P["g"]) if is_count(case) else o.g)
    pre = o.preprocess_obs
    o.preprocess_obs = lambda obs: pre(MR.zero_filled(obs))
    return o


def run_oracle(model, FLAGS, case, obs, noise, teacher=None, dtype=torch.float64, ess_frac=None):
    o = objective(model.export_reference_layout(dtype), FLAGS, case, ess_frac)
    with torch.no_grad():
        z, log = o.get_log_ZSMC(obs.to(dtype).cpu(), AR._cast({**noise, **(teacher or {})}, dtype))
    return z, log


hip_teacher = AR.hip_teacher


def replay_with_hip(model, FLAGS, case, obs, noise, log, dtype=torch.float64):
    """the reference with the HIP run's indices AND decisions teacher-forced: (z_ref, ref_log)"""
    return run_oracle(model, FLAGS, case, obs, noise, teacher=hip_teacher(log), dtype=dtype)


def oracle_grads(model, FLAGS, case, obs, noise, teacher, dtype=torch.float64):
    """ELBO and the autograd gradients of the reference in `dtype`"""
    P = MR.require_grad(model.export_reference_layout(dtype))
    o = objective(P, FLAGS, case)
    z, _ = o.get_log_ZSMC(obs.to(dtype).cpu(), AR._cast({**noise, **teacher}, dtype))
    z.backward()
    return z.detach(), P
