"""fp64 reference of PSVO on missing observations (FLAGS.missing_obs with FLAGS.BSim_missing_obs; psvo_bsim_forward_wobs_missing
behind psvo_filter_forward_wobs_missing): tests/missing_reference.objective(P, FLAGS, "PSVO") -- the oracle's PSVO whose emission
sums the observed terms only, in the filter and wherever the backward simulation scores it, and whose filter-side proposal reads
the observations with missing entries set to 0 -- with one more change,

  * BS_preprocess_obs, which feeds BSim_q2 and BSim_q_init (the oracle's `enc`), is fed the zero-filled observations too.  With
    the bi-LSTM encoder that method does not go through preprocess_obs, so missing_reference's wrapper does not reach it.

Nothing in the oracle changes.  With every entry observed zero_filled is the identity and MissingEmission repeats
diag_log_prob's arithmetic, so the unmodified oracle's PSVO value and gradients are reproduced exactly
(tests/test_missing_bsim_host.py).  The mask is missing_reference.mask().  A helper, not a test; only tests and tools import it."""
import torch

from tests import helpers as Hh
from tests import missing_reference as MR
from tests.missing_reference import _cast, knock_out, mask, require_grad, zero_filled      # noqa: F401  (re-exported)


def objective(P, FLAGS, obj="PSVO"):
    """missing_reference.objective with the backward simulation's proposal side on zero-filled observations"""
    o = MR.objective(P, FLAGS, obj)
    bs_pre = o.BS_preprocess_obs
    o.BS_preprocess_obs = lambda obs: bs_pre(zero_filled(obs))
    return o


def run_oracle(model, FLAGS, obs, noise, teacher=None, dtype=torch.float64, obj="PSVO"):
    o = objective(model.export_reference_layout(dtype), FLAGS, obj)
    with torch.no_grad():
        z, log = o.get_log_ZSMC(obs.to(dtype).cpu(), _cast({**noise, **(teacher or {})}, dtype))
    return z, log


def oracle_grads(model, FLAGS, obs, noise, teacher, dtype=torch.float64, obj="PSVO"):
    """ELBO and the autograd gradients of the reference in `dtype`"""
    P = require_grad(model.export_reference_layout(dtype))
    o = objective(P, FLAGS, obj)
    z, _ = o.get_log_ZSMC(obs.to(dtype), _cast({**noise, **teacher}, dtype))
    z.backward()
    return z.detach(), P


def teacher(ref):
    """the indices of a reference run, to be forced on the kernels: no draw can flip"""
    return {"idx_f": ref["idx_f"], "idx_b": ref["idx_b"]}


def hip_noise(noise, teach, device="cuda"):
    nz = Hh.noise_to_hip({**noise, **teach}, device)
    if "idx_f" in nz:
        nz.pop("u_f", None)
    if "sel_b" in nz:
        nz.pop("u_b", None)
    return nz
