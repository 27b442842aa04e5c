"""Time of the MAP trajectory (psvo_map_path) beside the marginal smoother (psvo_ffbs_smooth) on the same particle system, device
events.

    python tools/map_path_timing.py [--out profiles/map_path_timing.json] [--shape T B N Dx Dy] ... [--calls K]

Per shape the particle system is the one of tools/ffbs_timing.py (a forward filter in the bootstrap wiring with two proposals,
H = 32, Dy = 1, random small weights); the emission network of the decoder is a random one of width H = 32 at the shape's own Dy
with random observations -- the kernels do not care that the filter scored other data.  Timed alternately, round after round:
    ffbs_smooth              the smoother (constant scale, uniforms, every output)
    map_path                 both launches and the backtrack (ops.map_path)
    map_path_no_backtrack    the same entry point with path = Xmap = NULL: both launches, no backtrack
    map_emission_T1          the entry point on the same T B (step, sequence) pairs declared as T = 1: the emission launch as it is,
                             and a recursion launch that only has step 0 to do (T B workgroups, a prior term and a maximum each)
A window is BATCH back-to-back launches between two events, the figure the median over the rounds of window / BATCH, reported
with its minimum and maximum.  The backtrack alone is map_path - map_path_no_backtrack; the recursion alone is bounded by
map_path_no_backtrack - map_emission_T1 from below.  For the per-kernel split run a kernel trace over `--calls K` (K plain calls of
map_path and ffbs_smooth per shape, nothing else) and read map_emission_kernel / map_viterbi_kernel / ffbs_kernel there.
Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ffbs_timing as FT          # noqa: E402  (the particle system and the measuring loop)

SHAPES = [(200, 64, 128, 2, 1), (200, 64, 512, 3, 10)]      # (T, B, N, Dx, Dy)
H = 32


def arms(T, B, N, Dx, Dy):
    import torch
    from psvo_amd import _lib, ops
    base, _, _ = FT.arms(B, T, N, Dx)
    f = base["filter_forward"]()
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).cuda()
    sig = (0.5 + torch.rand(Dx, generator=gen)).cuda()
    sig_g = (0.5 + torch.rand(Dy, generator=gen)).cuda()
    g = (rn(Dx, H, scale=0.3), rn(H, scale=0.1), rn(H, Dy, scale=0.3), rn(Dy, scale=0.1))
    obs, fm0, fsig0 = rn(T, B, Dy), f["X"][0].mean(-1).contiguous(), (1.0 + torch.rand(Dx, generator=gen)).cuda()
    up = torch.rand(T, B, N, generator=gen).cuda()
    desc_s = ops.make_desc(B, T, N, 1, Dx, 1, H)
    desc = ops.make_desc(B, T, N, 1, Dx, Dy, H)
    first = ops.map_path(desc, f, g, sig, sig_g, fm0, fsig0, obs)

    lib = _lib.load()
    gs = ops._mlp_struct(g, Dx, H, Dy, "g")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    delta, lmax, bp = torch.empty_like(first["delta"]), torch.empty_like(first["lmax"]), torch.empty_like(first["bp"])

    def raw(d, fm0_, obs_):
        _lib.check(lib.psvo_map_path(ctypes.byref(d), ctypes.byref(gs), P(sig), P(sig_g), P(fm0_), P(fsig0), P(obs_), P(f["X"]),
                                     P(f["Fm"]), P(delta), P(lmax), P(bp), None, None,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "psvo_map_path")
    desc1 = ops.make_desc(B * T, 1, N, 1, Dx, Dy, H)
    fm0_1 = fm0.repeat(T, 1).contiguous()                      # (T B, Dx): a prior mean for every pair
    raw(desc, fm0, obs)
    assert torch.equal(delta, first["delta"]) and torch.equal(bp, first["bp"])
    out = {"ffbs_smooth": lambda: ops.ffbs_smooth(desc_s, f, sig_f=sig, u=up),
           "map_path": lambda: ops.map_path(desc, f, g, sig, sig_g, fm0, fsig0, obs),
           "map_path_no_backtrack": lambda: raw(desc, fm0, obs),
           "map_emission_T1": lambda: raw(desc1, fm0_1, obs)}
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, action="append", metavar=("T", "B", "N", "Dx", "Dy"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=0, help="K plain calls of map_path and ffbs_smooth per shape and nothing else")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("map_path_timing.py measures on the GPU: none is visible")
    res = {"device": torch.cuda.get_device_name(0), "rounds": FT.ROUNDS, "shapes": {}}
    for T, B, N, Dx, Dy in (a.shape or SHAPES):
        fns = arms(T, B, N, Dx, Dy)
        if a.calls:
            for _ in range(a.calls):
                fns["map_path"]()
                fns["ffbs_smooth"]()
            torch.cuda.synchronize()
            continue
        batch = 20 if T * N <= 200 * 128 else 3
        r = FT.measure(fns, batch)
        res["shapes"]["T%d B%d N%d Dx%d Dy%d" % (T, B, N, Dx, Dy)] = dict(r, batch=batch)
        for k, v in r.items():
            print("T%-5d B%-3d N%-4d Dx%d Dy%-2d  %-22s median %8.4f ms  (min %8.4f, max %8.4f)  %7.1f ns per step"
                  % (T, B, N, Dx, Dy, k, v["median_ms"], v["min_ms"], v["max_ms"], v["median_ms"] * 1e6 / T), flush=True)
    if a.out and not a.calls:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
