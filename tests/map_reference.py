"""Reference restatement of the MAP trajectory (include/psvo_hip.h: psvo_map_path) in plain torch, written from the recursion in
the header on top of tests/ffbs_reference.log_transition.  It runs in the dtype of its inputs (fp64: the reference; fp32 on the
CPU: the yardstick that says what fp32 arithmetic costs at a given shape).  Beside it: a brute-force maximiser over all N^T
paths for tiny systems, the fp64 joint log-density of a given path, the one-step check of a set of backpointers against the
delta they were computed from, and the case table of tests/test_gpu_map_path.py.  A helper, not a test.

Layouts are the library's: particles (T, B, Dx, N), observations (T, B, Dy), delta and bp (T, B, N), lmax and path (T, B).
"""
import itertools
import math

import torch

from tests.ffbs_reference import log_transition

ULP = 2.0 ** -24


def emission_terms(X, obs, g, sig_g, emission):
    """G (T, B, N): the emission log-density of every particle over the OBSERVED entries of its step (NaN = not observed), terms
    added in the order e = 0 .. Dy - 1, each Gaussian term with its own constant; exactly 0 where nothing is observed.
    g = (W1 (Dx,H), b1 (H), W2 (H,Dy), b2 (Dy)), relu; emission 0: normal around the output with scale sig_g, 1: normal around
    softplus + 1e-6 (the caller passes ones as sig_g), 2: Poisson with rate softplus + 1e-6 (sig_g is not read)."""
    W1, b1, W2, b2 = (w.to(X.dtype) for w in g)
    h = torch.relu(X.transpose(2, 3) @ W1 + b1)                          # (T, B, N, H)
    r = h @ W2 + b2                                                      # (T, B, N, Dy)
    mean = lambda v: torch.where(v > 20, v, torch.log1p(torch.exp(torch.clamp(v, max=20.0)))) + 1e-6
    acc = torch.zeros(X.shape[0], X.shape[1], X.shape[3], dtype=X.dtype)
    for e in range(obs.shape[-1]):
        y = obs[..., e].to(X.dtype).unsqueeze(-1)                        # (T, B, 1)
        seen = ~torch.isnan(y)
        y0 = torch.where(seen, y, torch.zeros_like(y))
        if emission == 2:
            lam = mean(r[..., e])
            term = y0 * torch.log(lam) - lam - torch.lgamma(y0.double() + 1).to(X.dtype)
        else:
            mu = mean(r[..., e]) if emission else r[..., e]
            s = sig_g[e].to(X.dtype)
            z = (y0 - mu) / s
            term = -0.5 * z * z - (torch.log(s) + 0.5 * math.log(2 * math.pi))
        acc = acc + torch.where(seen, term, torch.zeros_like(term))
    return acc


def log_prior(X0, fm0, fsig0):
    """(B, N): log N(X0[b, :, j]; fm0[b, :], fsig0)"""
    Dx = X0.shape[1]
    s = fsig0.to(X0.dtype).reshape(1, Dx, 1)
    d = (X0 - fm0.to(X0.dtype).unsqueeze(-1)) / s
    return (-0.5 * d * d - torch.log(s)).sum(1) - 0.5 * Dx * math.log(2 * math.pi)


def lowest_argmax(s):
    """(max over the last axis, the LOWEST index that attains it)"""
    m = s.max(-1, keepdim=True).values
    n = s.shape[-1]
    idx = torch.where(s == m, torch.arange(n).expand_as(s), torch.full_like(s, n, dtype=torch.long)).min(-1).values
    return m.squeeze(-1), idx.clamp(max=n - 1)


def _scales(sig_f, B, Dx, N, dtype):
    return sig_f.to(dtype).reshape(1, Dx, 1).expand(B, Dx, N)


def backtrack(delta, bp):
    """path (T, B): the lowest j with delta[T-1, b, j] == 0, then bp downwards"""
    T, B, N = delta.shape
    path = torch.empty(T, B, dtype=torch.long)
    path[T - 1] = lowest_argmax(delta[T - 1])[1]
    for t in range(T - 1, 0, -1):
        path[t - 1] = torch.gather(bp[t].long(), 1, path[t].unsqueeze(-1)).squeeze(-1)
    return path


def gather(X, path):
    """Xmap[t, b, :] = X[t, b, :, path[t, b]]"""
    T, B, Dx, N = X.shape
    return torch.gather(X, 3, path.long().reshape(T, B, 1, 1).expand(T, B, Dx, 1)).squeeze(-1)


def viterbi(X, Fm, sig_f, fm0, fsig0, G):
    """the recursion of the header on the emission terms G (T, B, N) -> dict(delta, lmax, bp, path, Xmap), in G's dtype"""
    T, B, Dx, N = X.shape
    S = _scales(sig_f, B, Dx, N, X.dtype)
    delta = torch.empty(T, B, N, dtype=X.dtype)
    lmax = torch.empty(T, B, dtype=X.dtype)
    bp = torch.empty(T, B, N, dtype=torch.long)
    for t in range(T):
        if t == 0:
            d = log_prior(X[0], fm0, fsig0) + G[0]
            bp[0] = torch.arange(N).expand(B, N)
        else:
            best, bp[t] = lowest_argmax(delta[t - 1].unsqueeze(-2) + log_transition(X[t], Fm[t - 1], S))      # (B, j, k)
            d = G[t] + best
        lmax[t] = d.max(-1).values
        delta[t] = d - lmax[t].unsqueeze(-1)
    path = backtrack(delta, bp)
    return {"delta": delta, "lmax": lmax, "bp": bp, "path": path, "Xmap": gather(X, path)}


def map_path(X, Fm, sig_f, fm0, fsig0, obs, g, sig_g, emission, dtype=torch.float64):
    """psvo_map_path in `dtype` on fp32 inputs; the dict of `viterbi` plus G"""
    c = lambda v: None if v is None else v.to(dtype)
    Gt = emission_terms(c(X), obs, [c(w) for w in g], c(sig_g), emission)
    out = viterbi(c(X), c(Fm), c(sig_f), c(fm0), c(fsig0), Gt)
    out["G"] = Gt
    return out


def joint64(path, X, Fm, sig_f, fm0, fsig0, G64):
    """J64 (B,): the fp64 joint log-density log mu(x_0) + sum log f + sum log g of the path (T, B) through the particles"""
    T, B, Dx, N = X.shape
    X, Fm = X.double(), Fm.double()
    path = path.long()
    pick = lambda v, t: torch.gather(v, 1, path[t].unsqueeze(-1)).squeeze(-1)
    J = pick(log_prior(X[0], fm0.double(), fsig0.double()), 0) + pick(G64[0], 0)
    S = _scales(sig_f, B, Dx, N, torch.float64)
    for t in range(1, T):
        l = log_transition(X[t], Fm[t - 1], S)                                                # (B, j, k)
        J = J + l[torch.arange(B), path[t], path[t - 1]] + pick(G64[t], t)
    return J


def brute_force(X, Fm, sig_f, fm0, fsig0, G64):
    """(best score (B,), best path (T, B)) over all N^T paths, fp64; the first maximiser in lexicographic order"""
    T, B, Dx, N = X.shape
    best = torch.full((B,), -float("inf"), dtype=torch.float64)
    arg = torch.zeros(T, B, dtype=torch.long)
    for p in itertools.product(range(N), repeat=T):
        path = torch.tensor(p).unsqueeze(-1).expand(T, B)
        J = joint64(path, X, Fm, sig_f, fm0, fsig0, G64)
        up = J > best
        best = torch.where(up, J, best)
        arg = torch.where(up.unsqueeze(0), path, arg)
    return best, arg


def one_step(delta, bp, X, Fm, sig_f):
    """the backpointers of steps 1 .. T-1 against the delta[t-1] THEY were computed from, in fp64: with
    s[j, k] = delta[t-1][k] + l64[j, k] a backpointer is off where it differs from the lowest fp64 argmax of s[j, :]; its
    distance is max_k s - s[j, bp].  Returns dict(off (T-1,B,N) bool, dist, s_bp (T-1,B,N) fp64)."""
    T, B, Dx, N = X.shape
    S = _scales(sig_f, B, Dx, N, torch.float64)
    off, dist, s_bp = [], [], []
    for t in range(1, T):
        s = delta[t - 1].double().unsqueeze(-2) + log_transition(X[t].double(), Fm[t - 1].double(), S)
        m, arg = lowest_argmax(s)
        at = torch.gather(s, 2, bp[t].long().unsqueeze(-1)).squeeze(-1)
        off.append(arg != bp[t].long())
        dist.append(m - at)
        s_bp.append(at)
    z = lambda v, dt: torch.stack(v) if v else torch.zeros(0, B, N, dtype=dt)
    return {"off": z(off, torch.bool), "dist": z(dist, torch.float64), "s_bp": z(s_bp, torch.float64)}


# ---- the inputs of the direct kernel tests (tests/test_gpu_map_path.py) and of the CPU checks of this restatement -------------
# (id, (T, B, Dx, N, sig), Dy, H, emission, kind)   kind: None, "tie" (particles N/2 .. N-1 are bit-copies of 0 .. N/2-1 in X and
# Fm) or "nan" (30 % of the observation entries NaN and one whole row)
DIRECT = [
    ((1, 1, 2, 8, 1.0), 1, 16, 0, None),             # no recursion
    ((2, 2, 2, 12, 1.0), 2, 32, 1, None),            # one step, sub-wave N that is not a power of two
    ((6, 2, 3, 100, 1.0), 10, 32, 0, None),
    ((7, 2, 2, 130, 0.3), 1, 64, 0, None),           # N just past two waves
    ((6, 2, 4, 300, 0.1), 32, 16, 2, None),          # the 512-thread configuration, partly filled; the widest observation
    ((5, 1, 4, 512, 1.0), 3, 64, 2, None),
    ((40, 2, 2, 64, 0.05), 1, 32, 0, None),          # sharp transitions
    ((200, 1, 2, 64, 0.3), 5, 32, 0, None),          # a bench-length T
    ((3, 1, 2, 1, 1.0), 1, 32, 0, None),             # N = 1
    ((4, 1, 2, 16, 1.0), 1, 32, 0, "tie"),
    ((6, 2, 3, 100, 1.0), 10, 32, 0, "nan"),
    ((6, 2, 3, 100, 1.0), 10, 32, 2, "nan"),
]
# one problem per instantiated (Dx, H, count form) of the emission kernel
INSTANCES = [((3, 1, Dx, 70, 0.5), 5, H, 2 if cnt else 0, None) for Dx in (2, 3, 4) for H in (16, 32, 64) for cnt in (0, 1)]


def case_id(c):
    shape, Dy, H, emission, kind = c
    return "-".join(map(str, shape)) + "-Dy%d-H%d-e%d" % (Dy, H, emission) + ("-" + kind if kind else "")


NAN_ROW = (2, 1)        # the (t, b) whose whole observation row is NaN in the "nan" cases

_CACHE = {}


def case(c):
    """inputs (fp32, CPU; seed 3) and both references of a case, computed once and shared: the non-cov system of
    tests/test_gpu_ffbs._system, a random one-hidden-layer relu g, observations 1.5 randn (the count emission scores counts:
    there |round(3 randn)|), fm0 = the mean of the cloud at t = 0"""
    if c not in _CACHE:
        from tests.test_gpu_ffbs import _system
        shape, Dy, H, emission, kind = c
        T, B, Dx, N, sig = shape
        X, Fm, S, _, _ = _system(T, B, Dx, N, sig, False, seed=3)
        if kind == "tie":
            X[..., N // 2:] = X[..., :N // 2]
            Fm[..., N // 2:] = Fm[..., :N // 2]
        gen = torch.Generator().manual_seed(31)
        rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
        g = [(rn(Dx, H) / math.sqrt(Dx)).float(), (0.3 * rn(H)).float(), (rn(H, Dy) / math.sqrt(H)).float(), (0.3 * rn(Dy)).float()]
        obs = 1.5 * rn(T, B, Dy)
        if emission == 2:
            obs = (2 * obs).round().abs()
        obs = obs.float()
        if kind == "nan":
            obs[torch.rand(T, B, Dy, generator=gen) < 0.3] = float("nan")
            obs[NAN_ROW] = float("nan")
        sig_g = None if emission == 2 else (torch.ones(Dy) if emission == 1
                                            else (0.5 + torch.rand(Dy, generator=gen, dtype=torch.float64)).float())
        sig_f = S[0, 0, :, 0].contiguous()
        fm0 = X[0].mean(-1).contiguous()                                                   # (B, Dx)
        fsig0 = torch.full((Dx,), 2.0 * sig)
        inp = dict(X=X, Fm=Fm, sig_f=sig_f, fm0=fm0, fsig0=fsig0, obs=obs, g=g, sig_g=sig_g, emission=emission)
        out = dict(inp, Dy=Dy, H=H, shape=shape, kind=kind)
        out["ref64"] = map_path(dtype=torch.float64, **inp)
        out["ref32"] = map_path(dtype=torch.float32, **inp)
        _CACHE[c] = out
    return _CACHE[c]


def delta_rule(c):
    """(err_32, floor) of delta for the smoother's rule err_hip <= 8 err_32 + 8 2^-24 max|ref|, over the finite entries"""
    d64, d32 = c["ref64"]["delta"], c["ref32"]["delta"].double()
    fin = torch.isfinite(d64)
    return float((d32 - d64)[fin].abs().max()), 8 * ULP * float(d64[fin].abs().max())
