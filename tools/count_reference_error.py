"""fp32 count reference against its own fp64 values on the nine cases of tests/test_gpu_count.py, on the CPU, with the tests'
own models (the _setup of tests/test_gpu_parity.py without .cuda()) and seeds (3: values, 5: gradients)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from oracle import psvo_oracle as O
from tests import count_reference as CR, helpers as Hh
from tests.test_gpu_parity import _pairs
torch.set_num_threads(8)
CASES = [("AESMC", 2, 5, 16, 1, 2, 3, 16, True, True), ("SVO", 2, 6, 40, 1, 3, 10, 32, False, True),
         ("IWAE", 2, 5, 24, 1, 4, 17, 64, True, False), ("AESMC", 1, 4, 512, 1, 4, 32, 32, False, True),
         ("SVO", 1, 60, 32, 1, 3, 10, 32, True, True), ("PSVO", 2, 5, 16, 4, 2, 3, 16, True, True),
         ("PSVO", 2, 6, 40, 8, 3, 10, 32, False, True), ("PSVO", 1, 5, 24, 32, 3, 32, 64, True, True),
         ("PSVO", 2, 5, 130, 4, 4, 17, 64, False, True)]

def setup(obj, B, T, N, M, Dx, Dy, H, bootstrap, two_q, seed):
    from psvo_amd.model import SSM
    hs = str(H)
    kw = dict(Dx=Dx, Dy=Dy, n_particles=N, n_particles_for_BSim_proposal=M, batch_size=B, time=T, q0_layers=hs, q1_layers=hs,
              q2_layers=hs, f_layers=hs, g_layers=hs, y_smoother_Dhs="8", X0_smoother_Dhs="8", use_bootstrap=bootstrap,
              use_2_q=two_q, count_emission=True, BSim_wide_obs=(obj == "PSVO"))
    FLAGS = Hh.make_flags(obj, **kw)
    torch.manual_seed(seed)
    model = Hh.perturb_(SSM(FLAGS))
    noise = O.make_noise(Hh.oracle_flags(FLAGS, obj), B, T, seed=1234 + seed)
    return FLAGS, model, CR.counts(B, T, Dy, 100 + seed), noise

mx = {}
def upd(k, v):
    mx[k] = max(mx.get(k, 0.0), v)
for case in CASES:
    obj = case[0]
    FLAGS, model, obs, noise = setup(*case, seed=3)
    z64, r64 = CR.run_oracle(model, FLAGS, obj, obs, noise)
    t = {"idx_f": r64["idx_f"]} if r64["idx_f"] is not None else {}
    if obj == "PSVO":
        t["idx_b"] = r64["idx_b"]
    z32, r32 = CR.run_oracle(model, FLAGS, obj, obs, noise, teacher=t, dtype=torch.float32)
    e = lambda k: float((r32[k].double() - r64[k]).abs().max())
    ratio = lambda a, b, atol: float(((a.double() - b).abs() / (atol + 1e-5 * b.abs())).max())
    row = {"X": e("X_prevs"), "logW": e("log_Ws"),
           "lse": float((torch.logsumexp(r32["log_Ws"], 1).double() - torch.logsumexp(r64["log_Ws"], 1)).abs().max()),
           "ELBOrel": abs(float(z32) - float(z64)) / abs(float(z64)), "maxlogW": float(r64["log_Ws"].abs().max())}
    row["ratio"] = max(ratio(r32["X_prevs"], r64["X_prevs"], 2e-4), ratio(r32["log_Ws"], r64["log_Ws"], 5e-4),
                       ratio(torch.logsumexp(r32["log_Ws"], 1), torch.logsumexp(r64["log_Ws"], 1), 5e-4),
                       ratio(r32["Xs"], r64["Xs"], 2e-4), row["ELBOrel"] / 1e-4)
    if obj == "PSVO":
        row["ratio"] = max([row["ratio"], ratio(r32["bw_Xs"], r64["bw_Xs"], 2e-4)] +
                           [ratio(r32[k], r64[k], 5e-4) for k in ("f_log_probs", "g_log_probs", "bw_log_Omegas")])
        row.update({"bwX": e("bw_Xs"), "flp": e("f_log_probs"), "glp": e("g_log_probs"), "Omega": e("bw_log_Omegas")})
    # gradients, seed 5
    FLAGS, model, obs, noise = setup(*case, seed=5)
    _, r0 = CR.run_oracle(model, FLAGS, obj, obs, noise)
    t = {"idx_f": r0["idx_f"]} if r0["idx_f"] is not None else {}
    if obj == "PSVO":
        t["idx_b"] = r0["idx_b"]
    _, P = CR.oracle_grads(model, FLAGS, obj, obs, noise, t)
    _, P32 = CR.oracle_grads(model, FLAGS, obj, obs, noise, t, dtype=torch.float32)
    worst = 0.0
    for (name, _, ref), (_, _, ref32) in zip(_pairs(model, P), _pairs(model, P32)):
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        r32 = torch.zeros_like(ref) if ref32.grad is None else ref32.grad.double()
        worst = max(worst, float((r32 - r).abs().max()) / max(float(r.abs().max()), 1e-6))
    row["grad"] = worst
    print("-".join(map(str, case)), " ".join("%s %.2e" % kv for kv in row.items()), flush=True)
    for k, v in row.items():
        upd(k, v)
print("MAX", " ".join("%s %.2e" % kv for kv in mx.items()))
