"""fp32 missing-observation reference against its own fp64 values on the ten runs of tests/test_gpu_missing.py, on the CPU, with the
tests' own models (the _setup of tests/test_gpu_parity.py without .cuda()), masks (tests/missing_reference.mask) and seeds
(3: values, 5: gradients).  Prints one row per run and the maxima; profiles/missing_obs.md holds the table."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from oracle import psvo_oracle as O
from tests import count_reference as CR, helpers as Hh, missing_reference as MR
from tests.test_gpu_parity import _pairs
torch.set_num_threads(8)
CASES = [("AESMC", 2, 5, 16, 1, 2, 1, 16, True, True), ("SVO", 2, 6, 40, 1, 3, 2, 32, False, True),
         ("AESMC", 2, 5, 16, 1, 2, 3, 16, True, True), ("SVO", 2, 6, 40, 1, 3, 10, 32, False, True),
         ("IWAE", 2, 5, 24, 1, 4, 17, 64, True, False), ("AESMC", 1, 4, 512, 1, 4, 32, 32, False, True),
         ("SVO", 1, 60, 32, 1, 3, 10, 32, True, True)]
RUNS = [(c, False) for c in CASES] + [(CASES[2], True), (CASES[3], True), (CASES[5], True)]


def setup(case, count, seed):
    from psvo_amd.model import SSM
    obj, B, T, N, M, Dx, Dy, H, bootstrap, two_q = case
    hs = str(H)
    kw = dict(Dx=Dx, Dy=Dy, n_particles=N, n_particles_for_BSim_proposal=M, batch_size=B, time=T, q0_layers=hs, q1_layers=hs,
              q2_layers=hs, f_layers=hs, g_layers=hs, y_smoother_Dhs="8", X0_smoother_Dhs="8", use_bootstrap=bootstrap,
              use_2_q=two_q, missing_obs=True, count_emission=count)
    FLAGS = Hh.make_flags(obj, **kw)
    torch.manual_seed(seed)
    model = Hh.perturb_(SSM(FLAGS))
    g = torch.Generator().manual_seed(100 + seed)
    obs = torch.randn(B, T, Dy, generator=g, dtype=torch.float64) * 1.5
    if count:
        obs = CR.counts(B, T, Dy, 100 + seed)
    noise = O.make_noise(Hh.oracle_flags(FLAGS, obj), B, T, seed=1234 + seed)
    return FLAGS, model, MR.knock_out(obs, MR.mask(B, T, Dy, seed)[0]), noise


mx = {}
for case, count in RUNS:
    obj = case[0]
    FLAGS, model, obs, noise = setup(case, count, 3)
    z64, r64 = MR.run_oracle(model, FLAGS, obj, obs, noise)
    t = {"idx_f": r64["idx_f"]} if r64["idx_f"] is not None else {}
    z32, r32 = MR.run_oracle(model, FLAGS, obj, obs, noise, teacher=t, dtype=torch.float32)
    e = lambda k: float((r32[k].double() - r64[k]).abs().max())
    ratio = lambda a, b, atol: float(((a.double() - b).abs() / (atol + 1e-5 * b.abs())).max())
    l32, l64 = torch.logsumexp(r32["log_Ws"], 1), torch.logsumexp(r64["log_Ws"], 1)
    row = {"X": e("X_prevs"), "logW": e("log_Ws"), "lse": float((l32.double() - l64).abs().max()),
           "ELBOrel": abs(float(z32) - float(z64)) / abs(float(z64)), "ELBO": abs(float(z64)),
           "maxlogW": float(r64["log_Ws"].abs().max()), "observed": 1.0 - float(torch.isnan(obs).float().mean())}
    row["ratio"] = max(ratio(r32["X_prevs"], r64["X_prevs"], 2e-4), ratio(r32["log_Ws"], r64["log_Ws"], 5e-4),
                       ratio(l32, l64, 5e-4), ratio(r32["Xs"], r64["Xs"], 2e-4), row["ELBOrel"] / 1e-4)
    FLAGS, model, obs, noise = setup(case, count, 5)
    _, r0 = MR.run_oracle(model, FLAGS, obj, obs, noise)
    t = {"idx_f": r0["idx_f"]} if r0["idx_f"] is not None else {}
    z5, P = MR.oracle_grads(model, FLAGS, obj, obs, noise, t)
    _, P32 = MR.oracle_grads(model, FLAGS, obj, obs, noise, t, dtype=torch.float32)
    worst = 0.0
    for (name, _, ref), (_, _, ref32) in zip(_pairs(model, P), _pairs(model, P32)):
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        r32g = torch.zeros_like(ref) if ref32.grad is None else ref32.grad.double()
        worst = max(worst, float((r32g - r).abs().max()) / max(float(r.abs().max()), 1e-6))
    row["grad"] = worst
    row["ELBO5"] = abs(float(z5))
    print("-".join(map(str, case)) + ("-count" if count else ""), " ".join("%s %.2e" % kv for kv in row.items()), flush=True)
    for k, v in row.items():
        mx[k] = max(mx.get(k, 0.0), v) if k not in ("ELBO", "ELBO5", "observed") else min(mx.get(k, 1e30), v)
print("MAX (ELBO, ELBO5, observed: MIN)", " ".join("%s %.2e" % kv for kv in mx.items()))
