"""Effect of the gradient guard on the notebook configuration: tests/notebook_curve.run_hip over seeds, once with the flags off
and once with clip_norm and skip_nonfinite_steps, same seeds, same epochs.

    python tools/adam_guard_effect.py --seeds 0-23 --epochs 20 --clip_norm 10 --out profiles/adam_guard_effect.json

Per run: whether it trained (the criterion of tests/test_gpu_notebook_curve.py: a finite held-out ELBO above -600 at the last
evaluation, and the run reached that evaluation), the steps clipped and skipped (from the trainer's own "gradient guard:" lines)
and the largest gradient norm.  The arm with the flags off has no guard to report a norm, so this probe takes it there itself:
psvo_grad_sumsq on the gradient in front of every plain step and a running maximum kept on the device (the update is
psvo_adam_step, untouched).  Needs a GPU."""
import argparse
import contextlib
import ctypes
import io
import json
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LINE = re.compile(r"gradient guard: last norm (\S+), largest norm (\S+); since the last evaluation (\d+) steps applied "
                  r"\((\d+) of them clipped\), (\d+) skipped")


def _seeds(spec):
    out = []
    for part in spec.split(","):
        lo, _, hi = part.partition("-")
        out += list(range(int(lo), int(hi or lo) + 1))
    return out


@contextlib.contextmanager
def observed_norms():
    """flags off: watch the norm of every gradient the plain optimizer takes; yields a dict filled in on exit"""
    import torch
    from psvo_amd import _lib, optim
    seen = {}
    real = optim.TFAdam.step

    def step(self, lr, world_size=1):
        lib = _lib.load()
        if "partial" not in seen:
            seen["partial"] = torch.zeros(lib.psvo_grad_norm_blocks(self.flat.numel), device="cuda", dtype=torch.float64)
            seen["max"] = torch.zeros((), device="cuda", dtype=torch.float64)
            seen["bad"] = torch.zeros((), device="cuda", dtype=torch.float64)
        _lib.check(lib.psvo_grad_sumsq(ctypes.c_void_p(self.flat.grad.data_ptr()), self.flat.numel,
                                       ctypes.c_void_p(seen["partial"].data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "psvo_grad_sumsq")
        norm = seen["partial"].sum().sqrt() / world_size
        ok = torch.isfinite(norm)
        seen["max"] = torch.where(ok, torch.maximum(seen["max"], norm), seen["max"])
        seen["bad"] = seen["bad"] + (~ok)
        return real(self, lr, world_size)
    optim.TFAdam.step = step
    out = {}
    try:
        yield out
    finally:
        optim.TFAdam.step = real
        if "max" in seen:
            out.update(max_norm=float(seen["max"]), nonfinite_steps=int(seen["bad"]))


def run(seed, epochs, **flags):
    from tests import notebook_curve as NC
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        rows = NC.run_hip(seed, epochs, quiet=False, **flags)
    guard = [LINE.search(l) for l in sink.getvalue().splitlines()]
    guard = [g.groups() for g in guard if g]
    last = rows["valid_log_ZSMC"][-1]
    done = rows["iter"][-1] == epochs
    out = {"seed": seed, "iters": rows["iter"], "valid_log_ZSMC": rows["valid_log_ZSMC"], "wall_s": rows["wall_s"],
           "trained": bool(done and math.isfinite(last) and last > -600.0)}
    if guard:
        out.update(applied=sum(int(g[2]) for g in guard), clipped=sum(int(g[3]) for g in guard),
                   skipped=sum(int(g[4]) for g in guard), max_norm=float(guard[-1][1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="0-23")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--clip_norm", type=float, default=10.0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("adam_guard_effect.py trains on the GPU: none is visible")
    res = {"epochs": a.epochs, "clip_norm": a.clip_norm, "off": [], "on": []}

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    for seed in _seeds(a.seeds):
        with observed_norms() as seen:
            off = run(seed, a.epochs)
        off.update(seen)
        on = run(seed, a.epochs, clip_norm=a.clip_norm, skip_nonfinite_steps=True)
        res["off"].append(off)
        res["on"].append(on)
        print(json.dumps({"seed": seed, "off": {k: off.get(k) for k in ("trained", "max_norm", "nonfinite_steps")},
                          "off_valid": off["valid_log_ZSMC"][-1],
                          "on": {k: on.get(k) for k in ("trained", "applied", "clipped", "skipped", "max_norm")},
                          "on_valid": on["valid_log_ZSMC"][-1]}), flush=True)
        dump()
    for arm in ("off", "on"):
        runs = res[arm]
        print("%s: %d of %d seeds trained" % (arm, sum(r["trained"] for r in runs), len(runs)))
    dump()


if __name__ == "__main__":
    main()
