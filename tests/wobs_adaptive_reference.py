"""Cases and reference of adaptive resampling on the wide-observation kernels (FLAGS.resample_ess with
FLAGS.resample_ess_wide_obs; psvo_filter_forward_wobs_adaptive / psvo_filter_backward_wobs_adaptive).

The reference is tests/adaptive_reference.py's, as it stands: its SMC does not depend on Dy.  For the count cases the
objective's emission is count_reference.CountEmission and the observations are count_reference.counts.  Seeding, `calm` and the
teacher / replay helpers are AR's.  A helper, not a test; only tests import it.
"""
import torch

from oracle import psvo_oracle as O
from tests import adaptive_reference as AR
from tests import count_reference as CR
from tests import helpers as Hh

# The largest |ESS_fp32 - ESS_fp64| / N of the reference over CASES, fp32 on the CPU with the fp64 run's draws and decisions
# (measured 7.0e-06 on the SVO / vind case, rounded up; tests/test_wobs_adaptive_host.py holds the measurement to it,
# profiles/wobs_adaptive.md records it).  The GPU tests allow 4 x this: the kernel's v_exp_f32 against libm.
ESS_GAP32_WIDE = 7.0e-06


def _W(calm, g=None, f=None, q1=None, **kw):
    d = dict(calm=calm, q2_sigma_min=4.0, **kw)
    if g is not None:
        d["g_sigma_min"] = g
    if f is not None:
        d["f_sigma_min"] = f
    if q1 is not None:
        d["q1_sigma_min"] = q1
    return d


# (objective, B, T, N, Dx, Dy, hidden layers, bootstrap, two_q, further flags, model seed, threshold)
# The smallest shapes that reach each form of the kernels.  Flags, thresholds and seeds are chosen on the CPU with the fp64
# reference alone, free running, so that it resamples at between 10 % and 90 % of the (step, sequence) pairs and never comes
# closer to its threshold than 100 x the GPU's ESS tolerance (tests/test_wobs_adaptive_host.py checks both).
CASES = [
    ("AESMC", 2, 6, 16, 2, 3, "16", True, True, dict(calm=0.5), 4, 0.5),                      # one wave, smallest Dy
    ("AESMC", 2, 7, 100, 3, 10, "32", False, True, _W(0.25, g=8.0), 3, 0.25),                 # Lorenz, padded lanes, own f
    ("SVO", 2, 8, 32, 2, 20, "32", True, True, _W(0.5, g=4.0), 6, 0.5),                       # vind, encoder
    ("AESMC", 2, 6, 130, 3, 17, "64", True, False, _W(0.5, g=4.0), 7, 0.5),                   # odd Dy, 3 waves, no q2
    ("AESMC", 2, 5, 300, 4, 5, "64", False, False, _W(0.25, g=8.0, f=3.0, q1=3.0), 3, 0.25),  # Dx 4, 5 waves
    ("AESMC", 2, 6, 40, 2, 10, "32", True, True, _W(0.5, g=4.0, poisson_emission=True), 3, 0.5),
    ("AESMC", 1, 5, 512, 4, 32, "32", False, True, _W(0.25, g=8.0), 3, 0.25),                 # every limit
    ("AESMC", 2, 6, 40, 2, 10, "32", True, True, _W(0.5, count_emission=True), 4, 0.5),
    ("SVO", 2, 6, 100, 3, 5, "32", False, True, _W(0.1, f=3.0, q1=3.0, count_emission=True), 6, 0.25),
]
ONE_WAVE, LORENZ, VIND, ODD, DX4, POISSON, LIMITS, COUNT, SVO_COUNT = range(9)


def case_id(c):
    tag = "-poisson" if c[9].get("poisson_emission") else "-count" if c[9].get("count_emission") else ""
    return "-".join(str(v) for v in c[:9]) + tag


def is_count(case):
    return bool(case[9].get("count_emission"))


def setup(case, device="cpu", seed=None, **extra):
    """AR.setup for a wide case: FLAGS.resample_ess = the case's threshold and FLAGS.resample_ess_wide_obs on, unless `extra` says
    otherwise; count cases get count observations"""
    tau = case[11]
    kw = dict(resample_ess=tau, resample_ess_wide_obs=True)
    kw.update(extra)
    FLAGS, model, smc, obs, noise = AR.setup(case[:11], device, seed=seed, **kw)
    if is_count(case):
        obs = CR.counts(case[1], case[2], case[5], 100 + (case[10] if seed is None else seed))
    return FLAGS, model, smc, obs, noise


def objective(P, FLAGS, case, ess_frac=None):
    o = AR.objective(P, FLAGS, case[0], ess_frac)
    if is_count(case):
        o.g = CR.CountEmission(P["g"])
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
    """ELBO and the autograd gradients of the reference in `dtype` (AR.oracle_grads with the case's emission)"""
    P = model.export_reference_layout(dtype)

    def req(x):
        if torch.is_tensor(x):
            x.requires_grad_(True)
        elif isinstance(x, dict):
            [req(v) for v in x.values()]
        elif isinstance(x, (list, tuple)):
            [req(v) for v in x]
    req(P)
    o = objective(P, FLAGS, case)
    z, _ = o.get_log_ZSMC(obs.to(dtype).cpu(), AR._cast({**noise, **teacher}, dtype))
    z.backward()
    return z.detach(), P


def static_objective(P, FLAGS, case, resample):
    """the unmodified oracle objective of the case (its own SMC): resampling at every step, or never"""
    fl = Hh.oracle_flags(FLAGS, case[0])
    if resample:
        o = O.OBJECTIVES[case[0]](P, fl)
    else:
        o = O.OracleIWAE(P, fl) if case[0] == "AESMC" else O.OracleSVO(P, fl, resample_particles=False)
    if is_count(case):
        o.g = CR.CountEmission(P["g"])
    return o
