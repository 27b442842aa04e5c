"""fp32 exogenous-input reference against its own fp64 values on the runs of tests/test_gpu_exo.py, on the CPU, with the tests' own
models, inputs and seeds (tests/exo_reference.cpu_setup; 3: values, 5: gradients).  Prints one row per run and the maxima;
profiles/exo_inputs.md holds the table.  table() returns the rows (tests/test_exo_host.py asserts them against a third of the
tolerances)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch

from tests import exo_reference as ER
from tests.test_gpu_parity import _pairs


def row_of(run):
    obj, Dx = run[0][0], run[0][5]
    FLAGS, model, obs, v, noise = ER.cpu_setup(run, 3)
    z64, r64 = ER.run(model, FLAGS, obj, obs, v, noise)
    t = {"idx_f": r64["idx_f"]} if r64["idx_f"] is not None else {}
    z32, r32 = ER.run(model, FLAGS, obj, obs, v, noise, teacher=t, dtype=torch.float32)
    e = lambda k: float((r32[k].double() - r64[k]).abs().max())
    ratio = lambda a, b, atol: float(((a.double() - b).abs() / (atol + 1e-5 * b.abs())).max())
    l32, l64 = torch.logsumexp(r32["log_Ws"], 1), torch.logsumexp(r64["log_Ws"], 1)
    row = {"run": ER.run_id(run), "X": e("X_prevs"), "logW": e("log_Ws"), "lse": float((l32.double() - l64).abs().max()),
           "elbo_rel": abs(float(z32) - float(z64)) / abs(float(z64)), "elbo_abs_min": abs(float(z64)),
           "max_logW": float(r64["log_Ws"].abs().max())}
    row["bound_share"] = max(ratio(r32["X_prevs"], r64["X_prevs"], 2e-4), ratio(r32["log_Ws"], r64["log_Ws"], 5e-4),
                             ratio(l32, l64, 5e-4), ratio(r32["Xs"], r64["Xs"], 2e-4))
    FLAGS, model, obs, v, noise = ER.cpu_setup(run, 5)
    _, r0 = ER.run(model, FLAGS, obj, obs, v, noise)
    t = {"idx_f": r0["idx_f"]} if r0["idx_f"] is not None else {}
    z5, P, dv = ER.grads(model, FLAGS, obj, obs, v, noise, t)
    _, P32, dv32 = ER.grads(model, FLAGS, obj, obs, v, noise, t, dtype=torch.float32)
    worst = float((dv32.double() - dv).abs().max()) / max(float(dv.abs().max()), 1e-6)
    for (name, _, ref), (_, _, ref32) in zip(_pairs(model, P), _pairs(model, P32)):
        r = torch.zeros_like(ref) if ref.grad is None else ref.grad
        g = torch.zeros_like(ref) if ref32.grad is None else ref32.grad.double()
        worst = max(worst, float((g - r).abs().max()) / max(float(r.abs().max()), 1e-6))
        if name in ("q1.W0", "f.W0"):       # (the input rows on their own scale)
            worst = max(worst, float((g[Dx:] - r[Dx:]).abs().max()) / max(float(r[Dx:].abs().max()), 1e-6))
    row["grad_rel"] = worst
    row["elbo_abs_min"] = min(row["elbo_abs_min"], abs(float(z5)))
    return row


def table():
    return [row_of(run) for run in ER.RUNS]


if __name__ == "__main__":
    torch.set_num_threads(8)
    keys = ("X", "logW", "lse", "elbo_rel", "bound_share", "grad_rel", "max_logW", "elbo_abs_min")
    rows = table()
    for r in rows:
        print(r["run"], " ".join("%s %.2e" % (k, r[k]) for k in keys), flush=True)
    print("MAX (elbo_abs_min: MIN)", " ".join("%s %.2e" % (k, (min if k == "elbo_abs_min" else max)(r[k] for r in rows)) for k in keys))
