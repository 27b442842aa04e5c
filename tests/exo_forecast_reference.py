"""Reference restatement of the particle forecast under exogenous inputs (include/psvo_hip.h: psvo_particle_forecast_input) in
plain torch, written from the recursion in the header: tests/forecast_reference.py's forecast with the first-layer bias of the
transition replaced, per origin and horizon, by the row
    b1 + hb_f[t + k, b, :]      (b1 alone where t + k >= Tv),
and with the predictive log-density summed over the observed entries of the target row (NaN = not observed; the missing form is
the base of the input form).  It runs in the dtype of its inputs (fp64: the reference; fp32 on the CPU: the yardstick).  A helper,
not a test.

Layouts are the library's and forecast_reference's; hb_f is (Tv, B, H), Tv >= T.
"""
import math

import torch

from tests import forecast_reference as R
from tests import missing_reference as MR

KEYS = R.KEYS


def log_g_observed(y, mu, sig_g, emission):
    """log g over the observed entries of y (..., 1, Dy) given the emission mean mu (..., N, Dy): NaN = not observed, each Gaussian
    term with its own constant"""
    seen = ~torch.isnan(y)
    y0 = torch.where(seen, y, torch.zeros_like(y))
    if emission == 2:
        terms = y0 * torch.log(mu) - mu - torch.lgamma(y0 + 1.0)
    else:
        z = (y0 - mu) / sig_g
        terms = -0.5 * z * z - torch.log(sig_g) - 0.5 * math.log(2.0 * math.pi)
    return torch.where(seen, terms, torch.zeros_like(terms)).sum(-1)


def bias_rows(hb_f, b1, T, k):
    """(T, B, 1, H): the effective first-layer bias of the transition from horizon k to k + 1 at every origin t -- one add"""
    Tv = hb_f.shape[0]
    rows = torch.zeros(T, hb_f.shape[1], hb_f.shape[2], dtype=hb_f.dtype)
    n = max(0, min(T, Tv - k))              # origins t < n have t + k < Tv
    rows[:n] = hb_f[k:k + n]
    return (b1 + rows).unsqueeze(-2)


def forecast(X, f, g, sig_f, sig_g, K, hb_f, emission=0, logW=None, obs=None, eps=None):
    """dict(ymean, yvar (K+1,T,B,Dy), xmean (K+1,T,B,Dx), lpd (K+1,T,B) or None without obs; 0 where t + k >= T and where the
    target row has nothing observed)"""
    T, B, Dx, N = X.shape
    W1, b1, W2, b2 = f
    x = X.permute(0, 1, 3, 2)                                                   # (T, B, N, Dx)
    logw = torch.full((T, B, N), -math.log(N), dtype=X.dtype) if logW is None else torch.log_softmax(logW, -1)
    w = torch.exp(logw).unsqueeze(-1)
    out = {k: [] for k in KEYS}
    for k in range(K + 1):
        mu = R.emission_mean(R.mlp(x, g), emission)                             # (T, B, N, Dy)
        ymean = (w * mu).sum(-2)
        v = sig_g * sig_g if emission == 0 else torch.ones_like(ymean) if emission == 1 else ymean
        out["ymean"].append(ymean)
        out["yvar"].append((w * mu * mu).sum(-2) - ymean * ymean + v)
        out["xmean"].append((w * x).sum(-2))
        if obs is not None:
            lpd = torch.zeros(T, B, dtype=X.dtype)
            if k < T:
                lg = log_g_observed(obs[k:].unsqueeze(-2), mu[:T - k], sig_g, emission)     # origin t scores obs[t + k]
                any_seen = (~torch.isnan(obs[k:])).any(-1)
                lpd[:T - k] = torch.where(any_seen, torch.logsumexp(logw[:T - k] + lg, -1), torch.zeros(T - k, B, dtype=X.dtype))
            out["lpd"].append(lpd)
        if k < K:
            x = torch.relu(x @ W1 + bias_rows(hb_f, b1, T, k)) @ W2 + b2
            if eps is not None:
                x = x + sig_f * eps[k].permute(0, 1, 3, 2)
    return {k: (torch.stack(v) if v else None) for k, v in out.items()}


# ---- the inputs of the direct kernel tests (tests/test_gpu_exo_forecast.py) ------------------------------------------------------
# id -> ((T, B, Dx, Dy, H, N, K, emission), Tv, weights, whether transition noise is injected, whether obs carries NaN entries)
CASES = {
    "four-origins": ((5, 3, 2, 1, 32, 16, 3, 0), 5, "finite", True, False),       # TB = 15: a dead origin in the last workgroup
    "K-beyond-T": ((4, 2, 3, 2, 16, 64, 6, 0), 4, "masked", True, False),         # most rows past Tv, both halves reused
    "three-waves": ((1, 2, 4, 3, 64, 192, 2, 1), 3, "none", True, False),         # H = 64, every future row given
    "count-eight-waves": ((6, 2, 3, 10, 32, 512, 4, 2), 8, "finite", True, False),      # future inputs that end part-way
    "noise-free": ((5, 3, 2, 1, 32, 16, 3, 0), 5, "finite", False, False),        # eps = NULL
    "missing": ((6, 2, 3, 10, 32, 512, 4, 2), 8, "finite", True, True),           # NaN entries in obs
}
# the standard deviation of the seeded hb_f: the size of b1's own spread in forecast_reference.system (0.3) and more, so that
# the inputs move the forecast far beyond the tolerance (tests/test_exo_forecast_host.py asserts it)
HB_SCALE = 1.0
ULP = 2.0 ** -24
_CACHE = {}


def hb_rows(Tv, B, H, seed=23, scale=HB_SCALE):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(Tv, B, H, generator=g, dtype=torch.float64)).float().contiguous()


def run(c, dtype, hb_f=None):
    """the restatement on the fp32 inputs of a case, computed in `dtype` (hb_f: in place of the case's own rows)"""
    a = R._as(c, dtype)
    hb = (c["hb_f"] if hb_f is None else hb_f).to(dtype)
    return forecast(a["X"], a["f"], a["g"], a["sig_f"], a["sig_g"], c["K"], hb, c["emission"], logW=a["logW"], obs=a["obs"],
                    eps=a["eps"])


def scored(obs, T, K):
    """(K+1, T, B) bool: the target of horizon k from origin t lies inside the data and has an observed entry"""
    n_obs = (~torch.isnan(obs)).sum(-1)                                    # (T, B)
    tk = torch.arange(T)[None, :] + torch.arange(K + 1)[:, None]           # (K+1, T)
    return (n_obs[tk.clamp(max=T - 1)] * (tk < T)[:, :, None]) > 0


def case(name):
    """inputs (fp32, CPU) and both references of a case, computed once, shared and left unchanged"""
    if name not in _CACHE:
        shape, Tv, weights, noisy, gaps = CASES[name]
        T, B, Dx, Dy, H, N, K, emission = shape
        c = dict(R.system(*shape, weights=weights, noisy=noisy))
        if gaps:
            c["obs"] = MR.knock_out(c["obs"], MR.mask(B, T, Dy, 3)[0].permute(1, 0, 2).contiguous())
        c["shape"], c["Tv"], c["hb_f"] = shape, Tv, hb_rows(Tv, B, H)
        c["ref64"], c["ref32"] = run(c, torch.float64), run(c, torch.float32)
        c["valid"] = scored(c["obs"], T, K)
        assert bool(c["valid"].any())
        assert gaps == bool((~c["valid"] & R.valid_mask(T, K)[:, :, None]).any())        # (gaps: empty target rows inside the data)
        assert torch.isfinite(c["ref64"]["lpd"]).all() and bool((c["ref64"]["lpd"][~c["valid"]] == 0).all()), name
        assert (c["ref64"]["yvar"] > 0).all() and (c["ref32"]["yvar"] > 0).all(), name
        _CACHE[name] = c
    return _CACHE[name]


def error(out, ref64, key, valid):
    """(max |out - ref64|, max |ref64|) of one output; lpd over the scored entries only (the others are exactly 0 by contract)"""
    o, r = out[key].double(), ref64[key]
    if key == "lpd":
        o, r = o[valid], r[valid]
    return float((o - r).abs().max()), float(r.abs().max())


def bound(c, key, k_tol):
    """the project's rule for one output of a case: K_TOL err_32 + 8 2^-24 max|ref_64|"""
    err_32, biggest = error(c["ref32"], c["ref64"], key, c["valid"])
    return k_tol * err_32 + 8 * ULP * biggest
