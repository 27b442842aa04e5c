"""Reference restatement of the particle forecast (include/psvo_hip.h: psvo_particle_forecast) in plain torch, written from the
recursion in the header with injected noise.  It runs in the dtype of its inputs (fp64: the reference; fp32 on the CPU: the
yardstick that says what fp32 arithmetic costs at a given shape).  A helper, not a test.

Layouts are the library's: cloud (T, B, Dx, N), log-weights (T, B, N), observations (T, B, Dy), noise (K, T, B, Dx, N); outputs
(K+1, T, B, .).  MLPs are (W1 (Din,H), b1 (H), W2 (H,Dout), b2 (Dout)) tuples.
"""
import math

import torch

KEYS = ("ymean", "yvar", "xmean", "lpd")


def mlp(x, p):
    W1, b1, W2, b2 = p
    return torch.relu(x @ W1 + b1) @ W2 + b2


def emission_mean(r, emission):
    """MLP_g's output -> mean of the emission: itself (0), softplus + 1e-6 (1: unit-scale normal around it, 2: Poisson rate)"""
    return r if emission == 0 else torch.nn.functional.softplus(r) + 1e-6


def log_g(y, mu, sig_g, emission):
    """log g(y | x) given the emission mean mu (..., N, Dy) and y (..., 1, Dy)"""
    if emission == 2:
        return (y * torch.log(mu) - mu - torch.lgamma(y + 1.0)).sum(-1)
    z = (y - mu) / sig_g
    return -0.5 * (z * z).sum(-1) - torch.log(sig_g).sum() - 0.5 * mu.shape[-1] * math.log(2.0 * math.pi)


def forecast(X, f, g, sig_f, sig_g, K, emission=0, logW=None, obs=None, eps=None):
    """dict(ymean, yvar (K+1,T,B,Dy), xmean (K+1,T,B,Dx), lpd (K+1,T,B) or None without obs; 0 where t + k >= T)"""
    T, B, Dx, N = X.shape
    x = X.permute(0, 1, 3, 2)                                                   # (T, B, N, Dx)
    logw = torch.full((T, B, N), -math.log(N), dtype=X.dtype) if logW is None else torch.log_softmax(logW, -1)
    w = torch.exp(logw).unsqueeze(-1)
    out = {k: [] for k in KEYS}
    for k in range(K + 1):
        mu = emission_mean(mlp(x, g), emission)                                 # (T, B, N, Dy)
        ymean = (w * mu).sum(-2)
        v = sig_g * sig_g if emission == 0 else torch.ones_like(ymean) if emission == 1 else ymean
        out["ymean"].append(ymean)
        out["yvar"].append((w * mu * mu).sum(-2) - ymean * ymean + v)
        out["xmean"].append((w * x).sum(-2))
        if obs is not None:
            lpd = torch.zeros(T, B, dtype=X.dtype)
            if k < T:
                lg = log_g(obs[k:].unsqueeze(-2), mu[:T - k], sig_g, emission)  # origin t scores obs[t + k]
                lpd[:T - k] = torch.logsumexp(logw[:T - k] + lg, -1)
            out["lpd"].append(lpd)
        if k < K:
            x = mlp(x, f)
            if eps is not None:
                x = x + sig_f * eps[k].permute(0, 1, 3, 2)
    return {k: (torch.stack(v) if v else None) for k, v in out.items()}


def valid_mask(T, K):
    """(K+1, T) bool: the target of horizon k from origin t lies inside the data"""
    return (torch.arange(T)[None, :] + torch.arange(K + 1)[:, None]) < T


# ---- the inputs of the direct kernel tests (tests/test_gpu_forecast.py) ---------------------------------------------------------
# (T, B, Dx, Dy, H, N, K, emission), weights ("none": logW = NULL, "finite", "masked": every third particle and the last of weight
# zero), whether transition noise is injected
_TABLE = [
    ((5, 3, 2, 1, 32, 16, 3, 0), "finite", True),         # sub-wave
    ((4, 2, 3, 2, 16, 64, 6, 0), "masked", True),         # K > T; particles of weight zero
    ((1, 2, 4, 3, 64, 192, 2, 1), "none", True),          # three waves, T = 1
    ((6, 2, 3, 10, 32, 512, 4, 2), "finite", True),       # count emission, N = 512
    ((3, 1, 2, 32, 16, 1, 0, 0), "none", False),          # N = 1, K = 0, Dy = 32
    ((5, 3, 2, 1, 32, 16, 3, 0), "none", False),          # eps = NULL: noise-free propagation
]


def cases():
    """[(id, shape, weights, noisy)]; every system is built (and checked: finite fp64 lpd at the valid entries, yvar > 0) once"""
    out = []
    for shape, weights, noisy in _TABLE:
        case(shape, weights, noisy)
        out.append(("-".join(map(str, shape)) + "-" + weights + ("" if noisy else "-noisefree"), shape, weights, noisy))
    return out


def system(T, B, Dx, Dy, H, N, K, emission, weights="none", noisy=True, seed=11):
    """A model, a latent path per sequence simulated from it, observations emitted from that path, and at every origin a cloud
    scattered around the path: the observations are draws of the model the forecast scores them with.  fp32 values (what the
    kernel is given)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    f = (rn(Dx, H) / math.sqrt(Dx), 0.3 * rn(H), 0.6 * rn(H, Dx) / math.sqrt(H), 0.1 * rn(Dx))
    g = (rn(Dx, H) / math.sqrt(Dx), 0.3 * rn(H), rn(H, Dy) / math.sqrt(H), 0.3 * rn(Dy))
    sig_f = 0.1 + 0.2 * torch.rand(Dx, generator=gen, dtype=torch.float64)
    sig_g = torch.ones(Dy, dtype=torch.float64) if emission else 0.3 + 0.5 * torch.rand(Dy, generator=gen, dtype=torch.float64)
    z = [rn(B, Dx)]
    for _ in range(T - 1):
        z.append(mlp(z[-1], f) + sig_f * rn(B, Dx))
    z = torch.stack(z)                                                                  # (T, B, Dx)
    mu = emission_mean(mlp(z, g), emission)
    obs = torch.poisson(mu, generator=gen) if emission == 2 else mu + sig_g * rn(T, B, Dy)
    X = z.unsqueeze(-1) + 0.3 * rn(T, B, Dx, N)
    logW = None
    if weights != "none":
        logW = -3.0 + 1.5 * rn(T, B, N)
        if weights == "masked":
            logW[:, :, ::3] = float("-inf")
            logW[:, :, N - 1] = float("-inf")
    eps = rn(K, T, B, Dx, N) if (noisy and K > 0) else None
    c32 = lambda v: None if v is None else tuple(c32(u) for u in v) if isinstance(v, tuple) else v.float().contiguous()
    return dict(f=c32(f), g=c32(g), sig_f=c32(sig_f), sig_g=c32(sig_g), X=c32(X), logW=c32(logW), obs=c32(obs), eps=c32(eps),
                K=K, emission=emission)


_CACHE = {}


def _as(c, dtype):
    cv = lambda v: None if v is None else tuple(cv(u) for u in v) if isinstance(v, tuple) else v.to(dtype)
    return {k: cv(c[k]) for k in ("X", "f", "g", "sig_f", "sig_g", "logW", "obs", "eps")}


def run(c, dtype):
    """the restatement on the fp32 inputs of system(), computed in `dtype`"""
    a = _as(c, dtype)
    return forecast(a["X"], a["f"], a["g"], a["sig_f"], a["sig_g"], c["K"], c["emission"], logW=a["logW"], obs=a["obs"],
                    eps=a["eps"])


def case(shape, weights="none", noisy=True):
    """inputs (fp32, CPU) and both references of a case, computed once, shared and left unchanged"""
    key = (shape, weights, noisy)
    if key not in _CACHE:
        c = system(*shape, weights=weights, noisy=noisy)
        c["ref64"], c["ref32"] = run(c, torch.float64), run(c, torch.float32)
        T, K = shape[0], shape[6]
        ok = valid_mask(T, K)
        c["valid"] = ok
        assert torch.isfinite(c["ref64"]["lpd"][ok]).all(), key
        assert (c["ref64"]["lpd"][~ok] == 0).all(), key
        assert (c["ref64"]["yvar"] > 0).all() and (c["ref32"]["yvar"] > 0).all(), key
        _CACHE[key] = c
    return _CACHE[key]


def error(out, ref64, key, valid):
    """(max |out - ref64|, max |ref64|) of one output; lpd over the valid entries only (the others are exactly 0 by contract)"""
    o, r = out[key].double(), ref64[key]
    if key == "lpd":
        o, r = o[valid], r[valid]
    return float((o - r).abs().max()), float(r.abs().max())
