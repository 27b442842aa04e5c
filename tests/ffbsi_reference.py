"""Reference restatement of the backward sampler (include/psvo_hip.h: psvo_ffbs_sample) in plain torch, written from the
recursion in the header on top of tests/ffbs_reference.log_transition.  It runs in the dtype of its inputs (fp64: the
reference; fp32 on the CPU: the yardstick that says what fp32 arithmetic costs at a given shape).  A helper, not a test.

Layouts are the library's: particles (T, B, Dx, N), log-weights, uniforms and indices (T, B, N).
"""
import torch

from oracle import psvo_oracle as O
from tests.ffbs_reference import log_transition


def _step_logits(X, Fm, S, a, t, succ):
    """v[b, n, k] of step t: a_t[k] at t = T-1 (succ None), else a_t[k] + l_t(X[t+1, b, :, succ[b, n]]; k)"""
    B, Dx, N = X.shape[1:]
    if succ is None:
        return a[t].unsqueeze(-2).expand(B, N, N)
    x = torch.gather(X[t + 1], 2, succ.unsqueeze(1).expand(-1, Dx, -1))                   # (B, Dx, n)
    return a[t].unsqueeze(-2) + log_transition(x, Fm[t], S[t])                            # (B, n, k)


def sample(X, Fm, S, logW, u=None, idx_in=None):
    """N backward-sampled paths per sequence.  `u` (T, B, N) uniforms or `idx_in` (T, B, N) forced indices (clamped to [0, N)).
    Returns dict(idx (T,B,N) int64, logq (T,B,N), Xs (T,B,Dx,N), distinct (T,B) int64).  The draw is the filter's:
    idx = #{k : cdf[k] <= u total} on the inclusive prefix sums of exp(v - max v), clamped to N - 1."""
    T, B, Dx, N = X.shape
    a = logW - torch.logsumexp(logW, -1, keepdim=True)
    idx = torch.empty(T, B, N, dtype=torch.int64)
    logq = torch.empty_like(logW)
    for t in range(T - 1, -1, -1):
        v = _step_logits(X, Fm, S, a, t, None if t == T - 1 else idx[t + 1])
        if idx_in is not None:
            j = idx_in[t].long().clamp(0, N - 1)
        else:
            cdf = torch.cumsum(torch.exp(v - v.max(-1, keepdim=True).values), -1)
            j = (cdf <= u[t].to(v.dtype).unsqueeze(-1) * cdf[..., -1:]).sum(-1).clamp(max=N - 1)
        idx[t] = j
        logq[t] = torch.gather(v, 2, j.unsqueeze(-1)).squeeze(-1) - torch.logsumexp(v, -1)
    return {"idx": idx, "logq": logq, "Xs": gather(X, idx), "distinct": distinct(idx)}


def gather(X, idx):
    """Xs[t, b, :, n] = X[t, b, :, idx[t, b, n]]"""
    return torch.gather(X, 3, idx.long().unsqueeze(2).expand(-1, -1, X.shape[2], -1))


def distinct(idx):
    """(T, B): how many different values idx[t, b, :] holds"""
    s = torch.sort(idx.long(), -1).values
    return 1 + (s[..., 1:] != s[..., :-1]).sum(-1)


def draw_distances(X, Fm, S, logW, u, idx):
    """(T, B, N) fp64: oracle.draw_distance of every idx[t, b, n] as the inverse-CDF draw by u[t, b, n] from exp v[n, :], where v
    is formed in fp64 from the chain's OWN successor index idx[t+1, b, n].  0 = the draw fp64 arithmetic makes."""
    X, Fm, S, logW, u = (v.double() for v in (X, Fm, S, logW, u))
    idx = idx.long()
    T, B, Dx, N = X.shape
    a = logW - torch.logsumexp(logW, -1, keepdim=True)
    out = torch.empty(T, B, N, dtype=torch.float64)
    for t in range(T):
        v = _step_logits(X, Fm, S, a, t, None if t == T - 1 else idx[t + 1])
        d = O.draw_distance(v.reshape(B * N, N).t(), u[t].reshape(B * N), idx[t].reshape(B * N))
        out[t] = d.reshape(B, N)
    return out


# ---- the inputs of the direct kernel tests (tests/test_gpu_ffbsi.py) and of the CPU check of this restatement -------------------
def cases():
    """[(id, shape, masked)]: the smoother's nine shapes, N = 1, and two systems in which every third particle and the last one
    have weight zero (logW = -inf)"""
    from tests.test_gpu_ffbs import SHAPES
    out = [(s, False) for s in SHAPES] + [((3, 2, 2, 1, 1.0, False), False)]
    out += [((4, 2, 2, 12, 1.0, False), True), ((5, 1, 3, 70, 0.3, True), True)]
    return [("-".join(map(str, s)) + ("-masked" if m else ""), s, m) for s, m in out]


_CACHE = {}


def case(shape, masked):
    """inputs (fp32, CPU; seed 3), forced indices (seed 9) and the references of a case, computed once and shared: the forced
    run in fp64 and fp32, the free run in fp32"""
    key = (shape, masked)
    if key not in _CACHE:
        from tests.test_gpu_ffbs import _system
        T, B, Dx, N = shape[:4]
        X, Fm, S, logW, u = _system(*shape, seed=3)
        if masked:
            logW[:, :, ::3] = float("-inf")
            logW[:, :, N - 1] = float("-inf")
        idx_in = torch.randint(0, N, (T, B, N), generator=torch.Generator().manual_seed(9), dtype=torch.int32)
        c = dict(X=X, Fm=Fm, S=S, logW=logW, u=u, idx_in=idx_in)
        c["forced64"] = sample(X.double(), Fm.double(), S.double(), logW.double(), idx_in=idx_in)
        c["forced32"] = sample(X, Fm, S, logW, idx_in=idx_in)
        c["free32"] = sample(X, Fm, S, logW, u=u)
        _CACHE[key] = c
    return _CACHE[key]


def forced_error(logq, ref64):
    """max |logq - ref64| over the entries where the fp64 value is finite (a forced index of weight zero has logq = -inf in
    every precision: those entries must be -inf, which is asserted here, and carry no error)"""
    logq, fin = logq.double(), torch.isfinite(ref64)
    assert torch.equal(logq[~fin], ref64[~fin])
    return float((logq[fin] - ref64[fin]).abs().max()), float(ref64[fin].abs().max())
