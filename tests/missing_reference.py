"""fp64 reference of missing observations (FLAGS.missing_obs; psvo_filter_forward_wobs_missing): the oracle objective of
tests/helpers.py with two changes,

  * its emission is wrapped so that log_prob(x, y) sums the terms of the observed entries only, a NaN in y being an entry that
    was not observed:    log g(y | x) = sum_{e: y_e == y_e} term_e(x, y_e).
    NaN is replaced by 0 before the arithmetic and the term is selected away afterwards, so that autograd stays finite (a NaN
    that is multiplied by a zero mask is still NaN in the gradient);
  * its preprocess_obs -- the encoders, the X0 feature and what q2 reads -- is fed the observations with missing entries set to
    0 (zero imputation on the proposal side; the bound holds for any proposal).

Both the Gaussian / unit-normal emission (the oracle's own OracleMVN / OraclePoisson) and the count emission
(tests/count_reference.CountEmission) are covered.  With every entry observed the Gaussian form repeats diag_log_prob's
arithmetic operation for operation, so the unmodified oracle is reproduced exactly.  run_oracle / oracle_grads /
replay_with_hip_indices mirror tests/count_reference.py.  A helper, not a test; only tests and tools import it.

The mask of the GPU tests (mask()) is seeded and identical for the reference and the kernel: about 30 % of the entries missing
independently, one step with every output missing, one output missing at every step (Dy >= 2: at Dy = 1 that output would be
the whole data set), where B = 2 sequence 1 missing from t = T-2 on (a ragged tail), and step 0 of sequence 0 observed in every
output but the one that is never observed.
"""
import torch

from oracle import psvo_oracle as O
from tests import helpers as Hh
from tests.count_reference import CountEmission

RATE = 0.3          # share of entries knocked out independently


def zero_filled(obs):
    return torch.where(torch.isnan(obs), torch.zeros_like(obs), obs)


class MissingEmission:
    """an emission of the oracle (mean, log_prob) whose log_prob leaves the NaN entries of `output` out"""

    def __init__(self, inner):
        self.inner, self.p = inner, inner.p

    def mean(self, Input):
        return self.inner.mean(Input)

    def log_prob(self, Input, output):
        seen = ~torch.isnan(output)
        if isinstance(self.inner, CountEmission):
            lam = self.inner.mean(Input)
            y = zero_filled(output).to(lam.dtype)
            terms = y * torch.log(lam) - lam - torch.lgamma(y + 1.0)
            return torch.where(seen, terms, torch.zeros_like(terms)).sum(-1)
        if isinstance(self.inner, O.OraclePoisson):
            mu, s = self.inner.mean(Input), self.inner.sigma()
        else:
            mu, s = self.inner.mean_and_sigma(Input)
        y = zero_filled(output).to(mu.dtype)
        z = (y - mu) / s
        zero = torch.zeros_like(z)
        # (diag_log_prob's three sums, each over the observed entries)
        return (-0.5 * torch.where(seen, z * z, zero).sum(-1) - torch.where(seen, torch.log(s) + zero, zero).sum(-1)
                - 0.5 * seen.sum(-1).to(z.dtype) * O.LOG2PI)


def objective(P, FLAGS, obj):
    """the oracle objective on the parameters P with the observed-terms-only emission and zero-filled proposal inputs"""
    o = O.OBJECTIVES[obj](P, Hh.oracle_flags(FLAGS, obj))
    o.g = MissingEmission(CountEmission(P["g"]) if getattr(FLAGS, "count_emission", False) else o.g)
    pre = o.preprocess_obs
    o.preprocess_obs = lambda obs: pre(zero_filled(obs))
    return o


def mask(B, T, Dy, seed):
    """(missing (B,T,Dy) bool, t_all: the step with nothing observed, e_never: the output never observed or None)"""
    g = torch.Generator().manual_seed(7000 + seed)
    miss = torch.rand(B, T, Dy, generator=g) < RATE
    t_all = 1 + (seed % (T - 2)) if B == 1 else 1 + (seed % max(T - 3, 1))      # (inside the sequence, ahead of the ragged tail)
    e_never = Dy // 2 if Dy >= 2 else None
    miss[0, 0, :] = False
    miss[:, t_all, :] = True
    if B == 2:
        miss[1, T - 2:, :] = True
    if e_never is not None:
        miss[:, :, e_never] = True
    return miss, t_all, e_never


def knock_out(obs, miss):
    return torch.where(miss, torch.full_like(obs, float("nan")), obs)


def _cast(nz, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in nz.items()}


def run_oracle(model, FLAGS, obj, obs, noise, teacher=None, dtype=torch.float64):
    o = objective(model.export_reference_layout(dtype), FLAGS, obj)
    with torch.no_grad():
        z, log = o.get_log_ZSMC(obs.to(dtype).cpu(), _cast({**noise, **(teacher or {})}, dtype))
    return z, log


def require_grad(P):
    if torch.is_tensor(P):
        P.requires_grad_(True)
    elif isinstance(P, dict):
        [require_grad(v) for v in P.values()]
    elif isinstance(P, (list, tuple)):
        [require_grad(v) for v in P]
    return P


def oracle_grads(model, FLAGS, obj, obs, noise, teacher, dtype=torch.float64):
    """ELBO and the autograd gradients of the reference in `dtype` (tests/test_gpu_parity.py::_oracle_grads)"""
    P = require_grad(model.export_reference_layout(dtype))
    o = objective(P, FLAGS, obj)
    z, _ = o.get_log_ZSMC(obs.to(dtype), _cast({**noise, **teacher}, dtype))
    z.backward()
    return z.detach(), P


def replay_with_hip_indices(model, FLAGS, obj, obs, noise, log):
    """helpers.replay_with_hip_indices on this reference: (z_ref, ref_log, dict(draws, off, worst))"""
    o = objective(model.export_reference_layout(torch.float64), FLAGS, obj)
    o.draw_log = []
    nz = dict(noise)
    nz.update(Hh.hip_indices(log, obj))
    with torch.no_grad():
        z, ref = o.get_log_ZSMC(obs.double().cpu(), nz)
    draws = off = 0
    worst = 0.0
    for log_W, u, idx in o.draw_log:
        d = O.draw_distance(log_W, u, idx)
        draws += d.numel()
        off += int((d > 0).sum())
        worst = max(worst, float(d.max()))
    return z, ref, {"draws": draws, "off": off, "worst": worst}
