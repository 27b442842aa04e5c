"""Reference restatement of the marginal particle smoother (include/psvo_hip.h: psvo_ffbs_smooth) in plain torch, written from
the recursion in the header.  It runs in the dtype of its inputs (fp64: the reference; fp32 on the CPU: the yardstick that
says what fp32 arithmetic costs at a given shape).  A helper, not a test; only tests import it.

Layouts are the library's: particles (T, B, Dx, N), log-weights (T, B, N).
"""
import math

import torch


def log_transition(X_next, Fm, S):
    """l[b, j, k] = log N(X_next[b, :, j]; Fm[b, :, k], S[b, :, k]) -- diagonal Gaussian on SCALES, the -sum log s term kept"""
    Dx = X_next.shape[1]
    d = (X_next.unsqueeze(-1) - Fm.unsqueeze(-2)) / S.unsqueeze(-2)                       # (B, Dx, j, k)
    return (-0.5 * d * d - torch.log(S).unsqueeze(-2)).sum(1) - 0.5 * Dx * math.log(2 * math.pi)


def smooth(X, Fm, S, logW):
    """normalised smoothed log-weights (T, B, N):
        a_t = logW[t] - logsumexp logW[t];  S[T-1] = a_{T-1};
        den[j] = logsumexp_k (a_t[k] + l_t[j,k]);  S[t][k] = a_t[k] + logsumexp_j (S[t+1][j] - den[j] + l_t[j,k])."""
    T = X.shape[0]
    out = torch.empty_like(logW)
    a = logW - torch.logsumexp(logW, -1, keepdim=True)
    out[T - 1] = a[T - 1]
    for t in range(T - 2, -1, -1):
        l = log_transition(X[t + 1], Fm[t], S[t])                                         # (B, j, k)
        den = torch.logsumexp(a[t].unsqueeze(-2) + l, -1)                                 # (B, j)
        out[t] = a[t] + torch.logsumexp((out[t + 1] - den).unsqueeze(-1) + l, -2)         # (B, k)
    return out


def moments(logWs, X):
    """(Xmean (T, B, Dx), ess (T, B)) of the weights exp(logWs) on the particles X"""
    p = logWs.exp()
    return (p.unsqueeze(2) * X).sum(-1), 1.0 / (p * p).sum(-1)


def scales(sig, T, B, Dx, N, dtype=torch.float64):
    """a constant scale vector (Dx,) as the (T, B, Dx, N) tensor `smooth` takes"""
    return torch.as_tensor(sig, dtype=dtype).reshape(1, 1, Dx, 1).expand(T, B, Dx, N)


def quantities(X, Fm, S, logW):
    """{"p": exp(logWs), "Xmean", "ess"} in fp64 values, computed in the dtype of the inputs"""
    lw = smooth(X, Fm, S, logW)
    xm, ess = moments(lw, X)
    return {"logWs": lw.double(), "p": lw.exp().double(), "Xmean": xm.double(), "ess": ess.double()}


def draw(logWs, u):
    """the filter's inverse-CDF draw on the weights exp(logWs[t, b, :]): idx = #{k : cdf[k] <= u total}, clamped to N - 1"""
    w = torch.exp(logWs - logWs.max(-1, keepdim=True).values)
    cdf = torch.cumsum(w, -1)
    target = u * cdf[..., -1:]
    idx = (cdf.unsqueeze(-2) <= target.unsqueeze(-1)).sum(-1)
    return idx.clamp(max=logWs.shape[-1] - 1)
