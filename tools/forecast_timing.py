"""Time of one particle forecast (psvo_particle_forecast through SVO.particle_forecast) beside the k-step prediction chain of the
reference's metric (SVO.n_step_prediction: 2 (MSE_steps + 1) row-MLP launches issued from Python), device events.

    python tools/forecast_timing.py [--out profiles/forecast_timing.json] [--shape B T N Dx Dy] ... [--steps 30]

Per shape a model in the bootstrap wiring (H = 32, one hidden layer) and a random cloud in the kernels' layout, as an evaluation
hands it over (log["Xs"]).  The arms -- the forecast with transition noise (the draw of the K T B Dx N normals included: it is part
of the call), the forecast with injected noise, the noise-free forecast, and the prediction chain -- are timed alternately, round
after round (tools/ffbs_timing.measure): a window is BATCH back-to-back calls between two events, the figure the median over the
rounds of window / BATCH, reported with its minimum and maximum.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ffbs_timing as FT          # noqa: E402  (the measuring loop)

SHAPES = [(32, 200, 128, 2, 1), (16, 200, 64, 2, 1), (32, 200, 128, 3, 10)]      # the notebook configuration C*; AESMC C2; wide


def arms(B, T, N, Dx, Dy, K, H=32):
    import torch
    from psvo_amd.flags import Flags
    from psvo_amd.model import SSM
    from psvo_amd.SMC.AESMC import AESMC
    hs = str(H)
    FLAGS = Flags(PSVO=False, AESMC=True, Dx=Dx, Dy=Dy, n_particles=N, batch_size=B, time=T, q0_layers=hs, q1_layers=hs,
                  q2_layers=hs, f_layers=hs, g_layers=hs, MSE_steps=K, particle_forecast=True)
    torch.manual_seed(0)
    model = SSM(FLAGS).cuda()
    smc = AESMC(model, FLAGS)
    smc.generator = torch.Generator(device="cuda").manual_seed(1)
    g = torch.Generator().manual_seed(2)
    hidden = torch.randn(T, B, Dx, N, generator=g).cuda().permute(1, 0, 3, 2)
    obs = torch.randn(B, T, Dy, generator=g).cuda()
    eps = torch.randn(K, T, B, Dx, N, generator=g).cuda()
    quiet = AESMC(model, Flags(**{**FLAGS.as_dict(), "forecast_noise": False}))

    def under_no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    out = {"particle_forecast": under_no_grad(lambda: smc.particle_forecast(K, hidden, obs)),
           "particle_forecast_injected": under_no_grad(lambda: smc.particle_forecast(K, hidden, obs, noise={"eps_p": eps})),
           "particle_forecast_noisefree": under_no_grad(lambda: quiet.particle_forecast(K, hidden, obs)),
           "n_step_prediction": under_no_grad(lambda: smc.n_step_prediction(K, hidden, obs))}
    for fn in out.values():
        fn()
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, action="append", metavar=("B", "T", "N", "Dx", "Dy"))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("forecast_timing.py measures on the GPU: none is visible")
    res = {"device": torch.cuda.get_device_name(0), "rounds": FT.ROUNDS, "steps": a.steps, "shapes": {}}
    for B, T, N, Dx, Dy in (a.shape or SHAPES):
        fns = arms(B, T, N, Dx, Dy, a.steps)
        batch = 20
        r = FT.measure(fns, batch)
        res["shapes"]["B%d T%d N%d Dx%d Dy%d" % (B, T, N, Dx, Dy)] = dict(r, batch=batch)
        for k, v in r.items():
            print("B%-3d T%-4d N%-4d Dx%d Dy%-2d K%-3d %-28s median %8.4f ms  (min %8.4f, max %8.4f)"
                  % (B, T, N, Dx, Dy, a.steps, k, v["median_ms"], v["min_ms"], v["max_ms"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
