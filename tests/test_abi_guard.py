"""The gradient guard's C ABI (include/psvo_hip.h: psvo_grad_norm_blocks, psvo_grad_sumsq, psvo_adam_step_guarded) and its two
flags, as far as they can be checked without a GPU: refusals come back as PSVO_ERR_INVALID before anything is launched."""
import ctypes
import math

import pytest


def _host_buffers():
    f = (ctypes.c_float * 8)()
    d = (ctypes.c_double * 8)()
    return f, d, ctypes.c_void_p(ctypes.addressof(f)), ctypes.c_void_p(ctypes.addressof(d))


def _guarded_args(F, D, **kw):
    a = dict(params=F, grads=F, m=F, v=F, n=8, lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=-1.0,
             clip_norm=10.0, skip_nonfinite=1, partial=D, state=D, stream=None)
    a.update(kw)
    return [a[k] for k in ("params", "grads", "m", "v", "n", "lr", "beta1", "beta2", "eps", "step", "grad_scale", "clip_norm",
                           "skip_nonfinite", "partial", "state", "stream")]


def test_guarded_step_refusals(built_lib):
    """null pointers, n <= 0, step <= 0, a negative or non-finite clip_norm: PSVO_ERR_INVALID, nothing launched (every other
    argument of each call is valid, so the refusal is that argument's)"""
    from psvo_amd import _lib
    lib = _lib.load()
    keep_f, keep_d, F, D = _host_buffers()
    bad = [dict(params=None), dict(grads=None), dict(m=None), dict(v=None), dict(partial=None), dict(state=None),
           dict(n=0), dict(n=-5), dict(step=0), dict(step=-1),
           dict(clip_norm=-1.0), dict(clip_norm=-1e-30), dict(clip_norm=float("inf")), dict(clip_norm=float("-inf")),
           dict(clip_norm=float("nan"))]
    for kw in bad:
        assert lib.psvo_adam_step_guarded(*_guarded_args(F, D, **kw)) == _lib.PSVO_ERR_INVALID, kw
    assert all(x == 0.0 for x in keep_f) and all(x == 0.0 for x in keep_d)
    with pytest.raises(ValueError):
        _lib.check(lib.psvo_adam_step_guarded(*_guarded_args(F, D, n=0)), "psvo_adam_step_guarded")


def test_sumsq_refusals(built_lib):
    from psvo_amd import _lib
    lib = _lib.load()
    keep_f, keep_d, F, D = _host_buffers()
    assert lib.psvo_grad_sumsq(None, 8, D, None) == _lib.PSVO_ERR_INVALID
    assert lib.psvo_grad_sumsq(F, 8, None, None) == _lib.PSVO_ERR_INVALID
    assert lib.psvo_grad_sumsq(F, 0, D, None) == _lib.PSVO_ERR_INVALID
    assert lib.psvo_grad_sumsq(F, -1, D, None) == _lib.PSVO_ERR_INVALID
    assert all(x == 0.0 for x in keep_d)


def test_norm_blocks(built_lib):
    """G: 1 for n = 1, never above 256, monotone in n, a function of n alone (asked twice, the same answer)"""
    from psvo_amd import _lib
    lib = _lib.load()
    assert lib.psvo_grad_norm_blocks(1) == 1
    ns = sorted(set([1, 2, 255, 256, 257, 4095, 4096, 4097, 22426, 10 ** 6, 1000003, 256 * 4096 - 1, 256 * 4096, 256 * 4096 + 1,
                     10 ** 9, 2 ** 40] + [int(1.37 ** k) for k in range(1, 80)]))
    prev = 0
    for n in ns:
        G = lib.psvo_grad_norm_blocks(n)
        assert 1 <= G <= 256, (n, G)
        assert G >= prev, (n, G, prev)
        assert lib.psvo_grad_norm_blocks(n) == G
        assert G == min(256, max(1, math.ceil(n / 4096))), (n, G)       # (the header's formula)
        prev = G
    assert lib.psvo_grad_norm_blocks(2 ** 40) == 256
    assert lib.psvo_grad_norm_blocks(22426) == 6 and lib.psvo_grad_norm_blocks(1000003) == 245


def test_abi_version_is_unchanged(built_lib):
    from psvo_amd import _lib
    assert _lib.load().psvo_abi_version() == 6        # (three functions added, nothing existing changed)


def test_flags():
    from psvo_amd.flags import Flags, parse_flags
    F = Flags()
    assert F.clip_norm == 0.0 and isinstance(F.clip_norm, float) and F.skip_nonfinite_steps is False
    F = parse_flags(["--clip_norm=10", "--skip_nonfinite_steps"])
    assert F.clip_norm == 10.0 and isinstance(F.clip_norm, float) and F.skip_nonfinite_steps is True
    F = parse_flags(["--clip_norm", "2.5", "--noskip_nonfinite_steps"])
    assert F.clip_norm == 2.5 and F.skip_nonfinite_steps is False
    assert parse_flags(["--skip_nonfinite_steps=true"]).skip_nonfinite_steps is True
    d = Flags(clip_norm=10.0).as_dict()
    assert d["clip_norm"] == 10.0 and d["skip_nonfinite_steps"] is False
    assert parse_flags([]).clip_norm == 0.0


def test_optimizer_refuses_a_bad_clip_norm_before_it_allocates():
    """TFAdam validates clip_norm itself (so the error names the argument, not a status code); flat is never touched"""
    from psvo_amd.optim import TFAdam

    class _Flat:
        @property
        def flat(self):
            raise AssertionError("the buffer was touched before clip_norm was checked")
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            TFAdam(_Flat(), clip_norm=bad)
