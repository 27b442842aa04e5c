"""fp64 reference of the count emission (FLAGS.count_emission, psvo_desc.emission = 2): the oracle objective of tests/helpers.py
with its emission replaced by a Poisson law per output,

    log g(y | x) = sum_e [ y_e log lam_e - lam_e - log Gamma(y_e + 1) ],    lam = softplus(MLP_g(x)) + 1e-6.

The oracle calls two methods on its emission, log_prob(Input, output) and mean(Input); CountEmission has both and runs in the
dtype of its parameters (fp64: the reference; fp32 on the CPU: the yardstick of what the arithmetic type costs on a case).
run_oracle / oracle_grads / replay_with_hip_indices mirror tests/helpers.py and tests/test_gpu_parity.py::_oracle_grads on top of
that.  A helper, not a test; only tests import it.
"""
import torch

from oracle import psvo_oracle as O
from tests import helpers as Hh

RATE = 4.0          # observations of all count tests: torch.poisson(RATE * U[0, 1)), seeded; they contain zeros


class CountEmission:
    def __init__(self, p):
        self.p = p

    def mean(self, Input):
        return torch.nn.functional.softplus(O.mlp_transform(self.p, Input)) + 1e-6

    def log_prob(self, Input, output):
        lam = self.mean(Input)
        y = output.to(lam.dtype)
        return (y * torch.log(lam) - lam - torch.lgamma(y + 1.0)).sum(-1)


def counts(B, T, Dy, seed, rate=RATE):
    """(B, T, Dy) fp64 counts, Poisson with rates rate * U[0, 1)"""
    g = torch.Generator().manual_seed(seed)
    lam = rate * torch.rand(B, T, Dy, generator=g, dtype=torch.float64)
    return torch.poisson(lam, generator=g)


def objective(P, FLAGS, obj):
    """the oracle objective on the parameters P with the count emission in place of its own"""
    o = O.OBJECTIVES[obj](P, Hh.oracle_flags(FLAGS, obj))
    o.g = CountEmission(P["g"])
    return o


def run_oracle(model, FLAGS, obj, obs, noise, teacher=None, dtype=torch.float64):
    o = objective(model.export_reference_layout(dtype), FLAGS, obj)
    nz = dict(noise)
    if teacher:
        nz.update(teacher)
    nz = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in nz.items()}
    with torch.no_grad():
        z, log = o.get_log_ZSMC(obs.to(dtype).cpu(), nz)
    return z, log


def oracle_grads(model, FLAGS, obj, obs, noise, teacher, dtype=torch.float64):
    """ELBO and the autograd gradients of the reference in `dtype` (tests/test_gpu_parity.py::_oracle_grads)"""
    P = model.export_reference_layout(dtype)

    def req(x):
        if torch.is_tensor(x):
            x.requires_grad_(True)
        elif isinstance(x, dict):
            [req(v) for v in x.values()]
        elif isinstance(x, (list, tuple)):
            [req(v) for v in x]
    req(P)
    o = objective(P, FLAGS, obj)
    nz = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in {**noise, **teacher}.items()}
    z, _ = o.get_log_ZSMC(obs.to(dtype), nz)
    z.backward()
    return z.detach(), P


def replay_with_hip_indices(model, FLAGS, obj, obs, noise, log):
    """helpers.replay_with_hip_indices on the count reference: (z_ref, ref_log, dict(draws, off, worst))"""
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
