"""Tensor-level wrappers over the C ABI: argument checking, output allocation, stream plumbing.

All tensors use the library's particle-minor HBM layout (include/psvo_hip.h):
particles (T, B, Dx, N), log-weights (T, B, N), features (T, B, D), bsim noise (T, B, Dx, N, M).
PyTorch is only the allocator / stream provider here.
"""
import contextlib
import ctypes
import threading

import torch

from . import _lib


# Deterministic mode (PSVO_TUNE_DETERMINISTIC, include/psvo_hip.h): on when the library switch is 1 (psvo_set_tuning or the
# PSVO_DETERMINISTIC environment variable) or when torch.use_deterministic_algorithms(True) is in force.  Under torch's flag
# the reverse wrappers hold the switch at 1 around their own launch (counted, so that launches from several threads share
# one setting and the last one out restores it).
def deterministic():
    """True when the reverse launches issued now take their fixed-order routes"""
    return (torch.are_deterministic_algorithms_enabled()
            or _lib.load().psvo_get_tuning(_lib.PSVO_TUNE_DETERMINISTIC) == 1)


_FIXED_LOCK = threading.Lock()
_FIXED_HOLD = [0, False]        # _fixed_order blocks open under torch's flag; whether they set the switch


@contextlib.contextmanager
def _fixed_order():
    """the enclosed launch runs under PSVO_TUNE_DETERMINISTIC = 1 when torch's flag is on; yields whether the switch is 1"""
    lib = _lib.load()
    key = _lib.PSVO_TUNE_DETERMINISTIC
    if not torch.are_deterministic_algorithms_enabled():
        yield lib.psvo_get_tuning(key) == 1
        return
    with _FIXED_LOCK:
        if _FIXED_HOLD[0] == 0 and lib.psvo_get_tuning(key) == 0:
            _lib.check(lib.psvo_set_tuning(key, 1), "psvo_set_tuning")
            _FIXED_HOLD[1] = True
        _FIXED_HOLD[0] += 1
    try:
        yield True
    finally:
        with _FIXED_LOCK:
            _FIXED_HOLD[0] -= 1
            if _FIXED_HOLD[0] == 0 and _FIXED_HOLD[1]:
                _FIXED_HOLD[1] = False
                lib.psvo_set_tuning(key, 0)


# Optional side stream for the native launches of one wrapper call.  Buffers the wrapper allocates come from
# the SIDE stream's pool: a block of the current stream's pool may have been freed by work that is still
# queued there (the caching allocator recycles within a stream without waiting), and the side stream is not
# ordered after that work.  Tensors that arrive from the current stream are record_stream()'ed when their
# pointer is taken; whoever consumes the outputs on the current stream must order the streams (event /
# wait_stream) and record_stream() them there (autograd.FilterFunction does).
_LAUNCH_STREAM = None


_NO_STREAM = contextlib.nullcontext()


def _on_launch_stream():
    """with _on_launch_stream(): torch's own work in the block (allocations, copies, fills) goes to the launch stream, if one is set"""
    return torch.cuda.stream(_LAUNCH_STREAM) if _LAUNCH_STREAM is not None else _NO_STREAM


def _empty(*shape, **kw):
    with _on_launch_stream():
        return torch.empty(*shape, **kw)


def _zeros(*shape, **kw):
    """zero-filled where it was allocated (for what a kernel accumulates into)"""
    with _on_launch_stream():
        return torch.empty(*shape, **kw).zero_()


class launch_on(object):
    """with ops.launch_on(stream): native kernels of the enclosed wrapper calls go to `stream`."""

    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        global _LAUNCH_STREAM
        self.prev, _LAUNCH_STREAM = _LAUNCH_STREAM, self.stream
        return self.stream

    def __exit__(self, *exc):
        global _LAUNCH_STREAM
        _LAUNCH_STREAM = self.prev
        return False


class _wgrad_on(object):
    """launch_on(stream), ordered after everything issued so far on the current stream; a no-op for None"""

    def __init__(self, stream):
        self.stream, self.ctx = stream, None

    def __enter__(self):
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())
            self.ctx = launch_on(self.stream)
            self.ctx.__enter__()
        return self.stream

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


def _ptr(t):
    if t is None:
        return None
    if _LAUNCH_STREAM is not None:
        t.record_stream(_LAUNCH_STREAM)
    return ctypes.c_void_p(t.data_ptr())


def _chk(t, shape, name, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda:
        raise ValueError("%s must live in HBM (cuda tensor); got %s" % (name, t.device))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def _mlp_struct(p, Din, H, Dout, name):
    """p = (W1 (Din,H), b1 (H), W2 (H,Dout), b2 (Dout)) keras-layout tensors; with two hidden layers
    (W1, b1, W2, b2, Wh (H,H), bh (H)): hidden_0, mu_layer, hidden_1."""
    W1, b1, W2, b2 = p[:4]
    _chk(W1, (Din, H), name + ".W1")
    _chk(b1, (H,), name + ".b1")
    _chk(W2, (H, Dout), name + ".W2")
    _chk(b2, (Dout,), name + ".b2")
    s = _lib.psvo_mlp()
    if len(p) == 6:
        _chk(p[4], (H, H), name + ".Wh")
        _chk(p[5], (H,), name + ".bh")
        s.Wh, s.bh = p[4].data_ptr(), p[5].data_ptr()
    elif len(p) != 4:
        raise ValueError("%s: an MLP is 4 tensors (one hidden layer) or 6 (two), got %d" % (name, len(p)))
    if _LAUNCH_STREAM is not None:
        for t in p:
            t.record_stream(_LAUNCH_STREAM)
    s.W1, s.b1, s.W2, s.b2 = W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr()
    return s


def mlp_grad_size(Din, H, Dout, layers=1):
    return Din * H + H + H * Dout + Dout + (H * H + H if layers == 2 else 0)


def make_desc(B, T, N, M, Dx, Dy, H, resample=True, two_q=True, bootstrap=True, emission=0, layers=1):
    d = _lib.psvo_desc()
    d.B, d.T, d.N, d.M, d.Dx, d.Dy, d.H = B, T, N, M, Dx, Dy, H
    d.layers = int(layers)            # hidden layers of every per-particle MLP of the call (1 or 2)
    d.resample, d.two_q, d.bootstrap = int(resample), int(two_q), int(bootstrap)
    d.emission = int(emission)        # 1: tf_poisson emission (unit-scale normal, softplus mean); 2: count (Poisson) emission, wide kernels
    return d


def _cur_stream():
    return _LAUNCH_STREAM if _LAUNCH_STREAM is not None else torch.cuda.current_stream()


def _stream():
    return ctypes.c_void_p(_cur_stream().cuda_stream)


# Optional instrumentation: bench.py installs a hook that records HIP events (on the stream the
# kernels are launched on) right before and after each native launch.  None = no overhead.
_HOOK = None


def set_timing_hook(hook):
    global _HOOK
    _HOOK = hook


def _mark(name, phase):
    if _HOOK is not None:
        _HOOK(name, phase, _cur_stream())


def _launch(name, fn, *args):
    """one native launch: the hook's marks around it, its status checked under `name`"""
    _mark(name, 0)
    st = fn(*args)
    _mark(name, 1)
    _lib.check(st, name)


# the entry points that take ess_frac / rs_in, by the `entry` they are asked for under (filter_forward_wobs with ess_frac stays a
# refusal: the wide adaptive route is filter_forward_wobs_adaptive)
_ADAPTIVE_ENTRY = {"psvo_filter_forward": "psvo_filter_forward_adaptive",
                   "psvo_filter_forward_wobs_adaptive": "psvo_filter_forward_wobs_adaptive",
                   "psvo_filter_forward_wobs_missing_adaptive": "psvo_filter_forward_wobs_missing_adaptive",
                   "psvo_filter_forward_wobs_input_adaptive": "psvo_filter_forward_wobs_input_adaptive"}
# ... and the ones that take the bias rows hb
_INPUT_ENTRY = ("psvo_filter_forward_wobs_input", "psvo_filter_forward_wobs_input_adaptive")


def filter_forward(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0,
                   obs, eps, u=None, idx_in=None, entry="psvo_filter_forward", ess_frac=None, rs_in=None, hb=None):
    """psvo_filter_forward (`entry`: an entry point with the same contract).  Returns dict(X, Xanc, Fm, logW, idx, lse).
    hb = (hb_q1, hb_f) (T,B,H) each, hb_f None under bootstrap: the bias rows of psvo_filter_forward_wobs_input and
    psvo_filter_forward_wobs_input_adaptive, the only entries that take them.
    ess_frac (a float > 0): psvo_filter_forward_adaptive -- resampling where ESS < ess_frac N; rs_in (T,B) int32 teacher-forces
    the decisions; the dict then also holds rs (T,B) int32 and ess (T,B)."""
    lib = _lib.load()
    B, T, N, Dx, Dy, H = desc.B, desc.T, desc.N, desc.Dx, desc.Dy, desc.H
    dev = eps.device
    q1s = _mlp_struct(q1, Dx, H, Dx, "q1")
    fs = None if desc.bootstrap else _mlp_struct(f, Dx, H, Dx, "f")
    gs = _mlp_struct(g, Dx, H, Dy, "g")
    _chk(sig_q1, (Dx,), "sig_q1"); _chk(sig_g, (Dy,), "sig_g")
    if desc.two_q:
        _chk(sig_q2, (Dx,), "sig_q2"); _chk(mu2, (T, B, Dx), "mu2")
    if not desc.bootstrap:
        _chk(sig_f, (Dx,), "sig_f")
    _chk(m0, (B, Dx), "m0"); _chk(sig0, (Dx,), "sig0")
    _chk(fm0, (B, Dx), "fm0"); _chk(fsig0, (Dx,), "fsig0")
    _chk(obs, (T, B, Dy), "obs"); _chk(eps, (T, B, Dx, N), "eps")
    _chk(u, (T, B, N), "u"); _chk(idx_in, (T, B, N), "idx_in", torch.int32)
    if desc.resample and u is None and idx_in is None:
        raise ValueError("resampling needs uniforms `u` or teacher-forced `idx_in`")
    adaptive = ()
    if ess_frac is not None:
        if entry not in _ADAPTIVE_ENTRY:
            raise ValueError("filter_forward: ess_frac belongs to the plain filter kernels (psvo_filter_forward_adaptive)")
        entry = _ADAPTIVE_ENTRY[entry]
        _chk(rs_in, (T, B), "rs_in", torch.int32)
    elif rs_in is not None:
        raise ValueError("filter_forward: rs_in without ess_frac")
    if (hb is not None) != (entry in _INPUT_ENTRY):
        raise ValueError("filter_forward: the bias rows hb belong to psvo_filter_forward_wobs_input, and it needs them")
    rows = ()
    if hb is not None:
        _chk(hb[0], (T, B, H), "hb_q1")
        if hb[0] is None or (not desc.bootstrap and hb[1] is None):
            raise ValueError("filter_forward_wobs_input needs hb_q1 and, unless bootstrap, hb_f")
        _chk(hb[1], (T, B, H), "hb_f")
        rows = (_ptr(hb[0]), None if desc.bootstrap else _ptr(hb[1]))
    out = {
        "X": _empty(T, B, Dx, N, device=dev), "Xanc": _empty(T, B, Dx, N, device=dev),
        "Fm": _empty(T, B, Dx, N, device=dev), "logW": _empty(T, B, N, device=dev),
        "idx": _empty(T, B, N, device=dev, dtype=torch.int32), "lse": _empty(T, B, device=dev),
        "P1": None if desc.bootstrap else _empty(T, B, Dx, N, device=dev),
    }
    if ess_frac is not None:
        out["rs"], out["ess"] = _empty(T, B, device=dev, dtype=torch.int32), _empty(T, B, device=dev)
        adaptive = (ctypes.c_float(float(ess_frac)), _ptr(rs_in), _ptr(out["rs"]), _ptr(out["ess"]))
    _launch(
        entry, getattr(lib, entry),
        ctypes.byref(desc), ctypes.byref(q1s), ctypes.byref(fs) if fs is not None else None, ctypes.byref(gs),
        _ptr(sig_q1), _ptr(sig_q2), _ptr(sig_f), _ptr(sig_g), _ptr(mu2), _ptr(m0), _ptr(sig0), _ptr(fm0),
        _ptr(fsig0), _ptr(obs), _ptr(eps), _ptr(u), _ptr(idx_in),
        _ptr(out["X"]), _ptr(out["Xanc"]), _ptr(out["Fm"]), _ptr(out["P1"]), _ptr(out["logW"]), _ptr(out["idx"]),
        _ptr(out["lse"]), *adaptive, *rows, _stream())
    return out


def filter_forward_wobs(*args, **kw):
    """psvo_filter_forward_wobs: the forward filter for wide observations (3 <= Dy <= 32, one hidden layer); arguments,
    outputs and layouts of filter_forward."""
    return filter_forward(*args, entry="psvo_filter_forward_wobs", **kw)


def filter_forward_wobs_adaptive(*args, ess_frac, rs_in=None, **kw):
    """psvo_filter_forward_wobs_adaptive: filter_forward_wobs resampling where ESS < ess_frac N; arguments of filter_forward,
    the result also holds rs (T,B) int32 and ess (T,B)."""
    if ess_frac is None:
        raise ValueError("filter_forward_wobs_adaptive needs the threshold ess_frac")
    return filter_forward(*args, entry="psvo_filter_forward_wobs_adaptive", ess_frac=ess_frac, rs_in=rs_in, **kw)


def filter_forward_wobs_missing(*args, **kw):
    """psvo_filter_forward_wobs_missing: filter_forward_wobs where a NaN in obs (T,B,Dy) is an observation that was not made -- its
    term is left out of the emission log-density (1 <= Dy <= 32, one hidden layer, every emission form); arguments, outputs and
    layouts of filter_forward."""
    return filter_forward(*args, entry="psvo_filter_forward_wobs_missing", **kw)


def filter_forward_wobs_input(*args, hb, **kw):
    """psvo_filter_forward_wobs_input: filter_forward_wobs_missing with input-driven transitions -- the first-layer bias of MLP_q1 /
    MLP_f at step t is b1 + hb[t,b,:], hb = (hb_q1, hb_f) (T,B,H) the input's share v_t W1[Dx:] of the hidden pre-activation
    (hb_f None under bootstrap); q1 / f hold W1[:Dx].  Arguments, outputs and layouts of filter_forward."""
    return filter_forward(*args, entry="psvo_filter_forward_wobs_input", hb=hb, **kw)


def filter_forward_wobs_input_adaptive(*args, hb, ess_frac, rs_in=None, **kw):
    """psvo_filter_forward_wobs_input_adaptive: filter_forward_wobs_input resampling where ESS < ess_frac N; arguments of
    filter_forward with the bias rows hb = (hb_q1, hb_f), the result also holds rs (T,B) int32 and ess (T,B)."""
    if ess_frac is None:
        raise ValueError("filter_forward_wobs_input_adaptive needs the threshold ess_frac")
    return filter_forward(*args, entry="psvo_filter_forward_wobs_input_adaptive", hb=hb, ess_frac=ess_frac, rs_in=rs_in, **kw)


def filter_forward_wobs_missing_adaptive(*args, ess_frac, rs_in=None, **kw):
    """psvo_filter_forward_wobs_missing_adaptive: filter_forward_wobs_missing resampling where ESS < ess_frac N (1 <= Dy <= 32, one
    hidden layer, every emission form); arguments of filter_forward, the result also holds rs (T,B) int32 and ess (T,B)."""
    if ess_frac is None:
        raise ValueError("filter_forward_wobs_missing_adaptive needs the threshold ess_frac")
    return filter_forward(*args, entry="psvo_filter_forward_wobs_missing_adaptive", ess_frac=ess_frac, rs_in=rs_in, **kw)


# The plain backward simulations (PSVO: bsim_*, PSVOwR: bsimwr_*) take the same inputs ahead of their own and their reverse
# launches write the same rows: what the four wrappers share is below; the argument lists mirror include/psvo_hip.h in each.
def _bsim_structs(d, f, g, q1_inv):
    return _mlp_struct(f, d.Dx, d.H, d.Dx, "f"), _mlp_struct(g, d.Dx, d.H, d.Dy, "g"), _mlp_struct(q1_inv, d.Dx, d.H, d.Dx, "q1_inv")


def _bsim_chk(desc, filt, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2, minit, sig_init, imean, isig, obs, eps_b, u_b, sel_in):
    B, T, N, M, Dx, Dy = desc.B, desc.T, desc.N, desc.M, desc.Dx, desc.Dy
    _chk(filt["Fm"], (T, B, Dx, N), "Fm"); _chk(filt["logW"], (T, B, N), "logW"); _chk(filt["lse"], (T, B), "lse")
    _chk(sig_f, (Dx,), "sig_f"); _chk(sig_g, (Dy,), "sig_g"); _chk(sig_q1inv, (Dx,), "sig_q1inv"); _chk(sig_bq2, (Dx,), "sig_bq2")
    _chk(bmu2, (T, B, Dx), "bmu2"); _chk(minit, (B, Dx), "minit"); _chk(sig_init, (Dx,), "sig_init")
    _chk(imean, (B, Dx), "imean"); _chk(isig, (Dx,), "isig"); _chk(obs, (T, B, Dy), "obs"); _chk(eps_b, (T, B, Dx, N, M), "eps_b")
    _chk(u_b, (T, B, N), "u_b"); _chk(sel_in, (T, B, N), "sel_in", torch.int32)


def _bsim_saves(desc, dev, save):
    """what the reverse launch reads back (allocated when a reverse pass will follow); row T-1 of mu1 is written as zeros: no predecessor"""
    B, T, N, M, Dx = desc.B, desc.T, desc.N, desc.M, desc.Dx
    z = lambda *s: _empty(*s, device=dev) if save else None
    return {"lam2": z(T, B, N, M), "om": z(T, B, N, M), "mu1": z(T, B, Dx, N)}


def _bsim_chk_saves(desc, bs, fn, own):
    """`bs` has what `fn`_forward(save=True) returns: the saves, and the caller's `own` ((key, shape), ...)"""
    B, T, N, M, Dx = desc.B, desc.T, desc.N, desc.M, desc.Dx
    for k, shp in (("lam2", (T, B, N, M)), ("om", (T, B, N, M)), ("mu1", (T, B, Dx, N))) + own:
        if bs.get(k) is None:
            raise ValueError("%s_backward needs %s_forward(save=True) outputs (missing %s)" % (fn, fn, k))
        _chk(bs[k], shp, k)


def _bsim_grads(desc, dev, nparts, own):
    """the outputs of the reverse launches, in allocation order: the rows for psvo_mlp_wgrad, the per-workgroup partials (nparts
    per sequence; 0: none, the entry point folds them itself), the caller's `own` ((key, shape), ...), the scale gradients"""
    B, T, N, M, Dx, Dy = desc.B, desc.T, desc.N, desc.M, desc.Dx, desc.Dy
    z = lambda *s: _empty(*s, device=dev)
    out = {"xt": z(T, B, Dx, N, M), "dFt": z(T, B, Dx, N, M), "dGt": z(T, B, Dy, N, M), "dmu1": z(T, B, Dx, N)}
    if nparts:
        out.update({"dFm_part": z(T, B, nparts, Dx, N), "dlogW_part": z(T, B, nparts, N)})
    out.update((k, z(*shp)) for k, shp in own)
    out.update({"dsig_f": z(Dx), "dsig_g": z(Dy), "dsig_q1inv": z(Dx), "dsig_bq2": z(Dx), "dsig_init": z(Dx), "disig": z(Dx)})
    return out


def _bsim_wgrad(out, desc, f, g, q1_inv, x_next, gb):
    """MLP_f / MLP_g on the sub-particles, MLP_q1inv on x_next[t+1]; gb: the slices of the flat gradient buffer to add to, or Nones"""
    T, Dx, Dy, H = desc.T, desc.Dx, desc.Dy, desc.H
    out["gf"] = mlp_wgrad(out["xt"][:T - 1], out["dFt"][:T - 1], f, Dx, H, Dx, grad=gb[0])
    out["gg"] = mlp_wgrad(out["xt"], out["dGt"], g, Dx, H, Dy, grad=gb[1])
    out["gq1inv"] = mlp_wgrad(x_next[1:], out["dmu1"][:T - 1], q1_inv, Dx, H, Dx, grad=gb[2])


def bsim_forward(desc, filt, f, g, q1_inv, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2, minit, sig_init,
                 imean, isig, obs, eps_b, u_b=None, sel_in=None, save=False, entry="psvo_bsim_forward"):
    """psvo_bsim_forward (`entry`: an entry point with the same contract).  `filt` is the dict returned by filter_forward.
    Returns dict(bwX, flp, glp, Omega, sel, score)."""
    lib = _lib.load()
    B, T, N, Dx = desc.B, desc.T, desc.N, desc.Dx
    dev = eps_b.device
    fs, gs, qs = _bsim_structs(desc, f, g, q1_inv)
    _chk(filt["X"], (T, B, Dx, N), "X")
    _bsim_chk(desc, filt, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2, minit, sig_init, imean, isig, obs, eps_b, u_b, sel_in)
    if u_b is None and sel_in is None:
        raise ValueError("backward simulation needs uniforms `u_b` or teacher-forced `sel_in`")
    z = lambda *s: _empty(*s, device=dev)
    out = {"bwX": z(T, B, Dx, N), "flp": z(T, B, N), "glp": z(T, B, N), "Omega": z(T, B, N),
           "sel": _empty(T, B, N, device=dev, dtype=torch.int32), "score": z(B, N), **_bsim_saves(desc, dev, save)}
    _launch(
        entry, getattr(lib, entry),
        ctypes.byref(desc), _ptr(filt["X"]), _ptr(filt["Fm"]), _ptr(filt["logW"]), _ptr(filt["lse"]),
        ctypes.byref(fs), ctypes.byref(gs), ctypes.byref(qs),
        _ptr(sig_f), _ptr(sig_g), _ptr(sig_q1inv), _ptr(sig_bq2), _ptr(bmu2), _ptr(minit), _ptr(sig_init),
        _ptr(imean), _ptr(isig), _ptr(obs), _ptr(eps_b), _ptr(u_b), _ptr(sel_in),
        _ptr(out["bwX"]), _ptr(out["flp"]), _ptr(out["glp"]), _ptr(out["Omega"]), _ptr(out["sel"]),
        _ptr(out["score"]), _ptr(out["lam2"]), _ptr(out["om"]), _ptr(out["mu1"]), _stream())
    return out


def bsim_forward_wobs(*args, **kw):
    """psvo_bsim_forward_wobs: the backward simulation for wide observations (3 <= Dy <= 32, one hidden layer); arguments,
    outputs and layouts of bsim_forward."""
    return bsim_forward(*args, entry="psvo_bsim_forward_wobs", **kw)


def bsim_forward_wobs_missing(*args, **kw):
    """psvo_bsim_forward_wobs_missing: bsim_forward_wobs where a NaN in obs (T,B,Dy) is an observation that was not made -- its
    term is left out of the emission log-density (1 <= Dy <= 32, one hidden layer, every emission form); arguments, outputs and
    layouts of bsim_forward."""
    return bsim_forward(*args, entry="psvo_bsim_forward_wobs_missing", **kw)


def elbo_filter(desc, lse):
    lib = _lib.load()
    _chk(lse, (desc.T, desc.B), "lse")
    out = _empty(desc.B, device=lse.device)
    _lib.check(lib.psvo_elbo_filter(ctypes.byref(desc), _ptr(lse), _ptr(out), _stream()), "psvo_elbo_filter")
    return out


def elbo_bsim(desc, score):
    lib = _lib.load()
    _chk(score, (desc.B, desc.N), "score")
    out = _empty(desc.B, device=score.device)
    _lib.check(lib.psvo_elbo_bsim(ctypes.byref(desc), _ptr(score), _ptr(out), _stream()), "psvo_elbo_bsim")
    return out


def elbo_bsim_mean(desc, score):
    """psvo_elbo_bsim_mean: scalar mean_b [logsumexp_n score - log N] (0-d tensor)."""
    lib = _lib.load()
    _chk(score, (desc.B, desc.N), "score")
    out = _empty(1, device=score.device)
    _lib.check(lib.psvo_elbo_bsim_mean(ctypes.byref(desc), _ptr(score), _ptr(out), _stream()), "psvo_elbo_bsim_mean")
    return out.reshape(())


def elbo_bsim_mean_backward(desc, score, dz):
    lib = _lib.load()
    _chk(score, (desc.B, desc.N), "score")
    dz = dz.detach().float().contiguous().reshape(1)
    dscore = _empty(desc.B, desc.N, device=score.device)
    _lib.check(lib.psvo_elbo_bsim_mean_backward(ctypes.byref(desc), _ptr(score), _ptr(dz), _ptr(dscore), _stream()),
               "psvo_elbo_bsim_mean_backward")
    return dscore


def bilstm_forward(x, W_fw, b_fw, W_bw, b_bw, save=False):
    """psvo_bilstm_forward: x (B,T,Din) -> out (B,T,2Dh) [, cs (2,B,T,Dh), gates (2,B,T,4Dh)]."""
    lib = _lib.load()
    B, T, Din = x.shape
    Dh = W_fw.shape[1] // 4
    _chk(x, (B, T, Din), "x")
    for nm, W, b in (("fw", W_fw, b_fw), ("bw", W_bw, b_bw)):
        _chk(W, (Din + Dh, 4 * Dh), "W_" + nm)
        _chk(b, (4 * Dh,), "b_" + nm)
    out = _empty(B, T, 2 * Dh, device=x.device)
    cs = _empty(2, B, T, Dh, device=x.device) if save else None
    gates = _empty(2, B, T, 4 * Dh, device=x.device) if save else None
    _launch("psvo_bilstm_forward", lib.psvo_bilstm_forward, B, T, Din, Dh, _ptr(x), _ptr(W_fw), _ptr(b_fw), _ptr(W_bw),
            _ptr(b_bw), _ptr(out), _ptr(cs), _ptr(gates), _stream())
    return (out, cs, gates) if save else out


def mlp_wgrad(X, dOut, w, Din, H, Dout, grad=None, axis=2, wobs=False):
    """psvo_mlp_wgrad / psvo_mlp2_wgrad: rows X [S][Din][L], dOut [S][Dout][L] -> flat grad [dW1|db1|dW2|db2]
    (two hidden layers, len(w) == 6: [dW1|db1|dWh|dbh|dW2|db2], the H x H products on the f32 matrix instruction).
    wobs: psvo_mlp_wgrad_wobs, one hidden layer with 3 <= Dout <= 32 (the H x Dout products on the matrix instruction).
    X / dOut are contiguous tensors whose feature axis is `axis` (dims before it flatten to the
    segments S, dims after it to the rows L of a segment), e.g. (T,B,Din,N) or (T,B,Din,N,M)."""
    lib = _lib.load()
    dev = X.device
    ax = axis
    if (not X.is_contiguous() or not dOut.is_contiguous() or X.shape[ax] != Din or dOut.shape[ax] != Dout
            or X.shape[:ax] != dOut.shape[:ax] or X.shape[ax + 1:] != dOut.shape[ax + 1:]):
        raise ValueError("mlp_wgrad: bad row tensors %s / %s for Din=%d, Dout=%d, axis=%d"
                         % (tuple(X.shape), tuple(dOut.shape), Din, Dout, ax))
    S = 1
    for v in X.shape[:ax]:
        S *= v
    L = 1
    for v in X.shape[ax + 1:]:
        L *= v
    ws = _mlp_struct(w, Din, H, Dout, "w")
    two = len(w) == 6
    if two and wobs:
        raise ValueError("mlp_wgrad: the wide-output weight gradient takes one hidden layer")
    name = "psvo_mlp2_wgrad" if two else "psvo_mlp_wgrad_wobs" if wobs else "psvo_mlp_wgrad"
    NP = mlp_grad_size(Din, H, Dout, 2 if two else 1)
    nblk = getattr(lib, name + "_blocks")(S * L)
    partial = _empty(nblk, NP, device=dev)
    acc = grad is not None
    if grad is None:
        grad = _empty(NP, device=dev)
    elif grad.numel() != NP:
        raise ValueError("mlp_wgrad: gradient slice of %d floats for an MLP of %d parameters" % (grad.numel(), NP))
    _launch(name, getattr(lib, name), S, L, Din, H, Dout, _ptr(X), _ptr(dOut), ctypes.byref(ws), _ptr(partial), _ptr(grad),
            int(acc), _stream())
    return grad


def mlp_wgrad_rowbias(X, dOut, hb, w, Din, H, Dout, grad=None, axis=2):
    """psvo_mlp_wgrad_rowbias: mlp_wgrad (one hidden layer, Din, Dout <= 4) where the first-layer bias of segment s is
    b1 + hb[s]; hb has the shape of X ahead of `axis`, then H.  Returns (flat grad [dW1|db1|dW2|db2], dhb like hb) with
    dhb[s] = sum over the segment's rows of d pre; `grad` given: accumulated into (dhb is always written)."""
    lib = _lib.load()
    dev = X.device
    ax = axis
    if (not X.is_contiguous() or not dOut.is_contiguous() or X.shape[ax] != Din or dOut.shape[ax] != Dout
            or X.shape[:ax] != dOut.shape[:ax] or X.shape[ax + 1:] != dOut.shape[ax + 1:]):
        raise ValueError("mlp_wgrad_rowbias: bad row tensors %s / %s for Din=%d, Dout=%d, axis=%d"
                         % (tuple(X.shape), tuple(dOut.shape), Din, Dout, ax))
    _chk(hb, tuple(X.shape[:ax]) + (H,), "hb")
    if hb is None or len(w) != 4:
        raise ValueError("mlp_wgrad_rowbias: needs the bias rows hb and an MLP with one hidden layer")
    S = 1
    for v in X.shape[:ax]:
        S *= v
    L = 1
    for v in X.shape[ax + 1:]:
        L *= v
    ws = _mlp_struct(w, Din, H, Dout, "w")
    NP = mlp_grad_size(Din, H, Dout)
    partial = _empty(lib.psvo_mlp_wgrad_rowbias_blocks(S), NP, device=dev)
    acc = grad is not None
    if grad is None:
        grad = _empty(NP, device=dev)
    elif grad.numel() != NP:
        raise ValueError("mlp_wgrad_rowbias: gradient slice of %d floats for an MLP of %d parameters" % (grad.numel(), NP))
    dhb = _empty(*hb.shape, device=dev)
    _launch("psvo_mlp_wgrad_rowbias", lib.psvo_mlp_wgrad_rowbias, S, L, Din, H, Dout, _ptr(X), _ptr(dOut), _ptr(hb),
            ctypes.byref(ws), _ptr(partial), _ptr(grad), _ptr(dhb), int(acc), _stream())
    return grad, dhb


def mlp_wgrad_wobs(X, dOut, w, Din, H, Dout, grad=None, axis=2):
    """psvo_mlp_wgrad_wobs: mlp_wgrad for an MLP with 3 <= Dout <= 32 outputs"""
    return mlp_wgrad(X, dOut, w, Din, H, Dout, grad=grad, axis=axis, wobs=True)


def rows_mlp_forward(X, w):
    """psvo_rows_mlp_forward: X (R, Din) -> (R, Dout); w = (W1 (Din,H), b1, W2 (H,Dout), b2)."""
    lib = _lib.load()
    R, Din = X.shape
    H, Dout = w[2].shape
    _chk(X, (R, Din), "X")
    ws = _mlp_struct(w, Din, H, Dout, "w")
    out = _empty(R, Dout, device=X.device)
    _launch("psvo_rows_mlp_forward", lib.psvo_rows_mlp_forward, R, Din, H, Dout, _ptr(X), ctypes.byref(ws), _ptr(out), _stream())
    return out


def rows_mlp_backward(X, dOut, w, need_dX=True, grad=None):
    """psvo_rows_mlp_backward -> (dX (R,Din) or None, flat grad [dW1|db1|dW2|db2]); `grad` given: accumulate."""
    lib = _lib.load()
    R, Din = X.shape
    H, Dout = w[2].shape
    _chk(X, (R, Din), "X"); _chk(dOut, (R, Dout), "dOut")
    ws = _mlp_struct(w, Din, H, Dout, "w")
    NP = Din * H + H + H * Dout + Dout
    dX = _empty(R, Din, device=X.device) if need_dX else None
    partial = _empty(lib.psvo_rows_mlp_blocks(R), NP, device=X.device)
    acc = grad is not None
    if grad is None:
        grad = _empty(NP, device=X.device)
    _launch("psvo_rows_mlp_backward", lib.psvo_rows_mlp_backward, R, Din, H, Dout, _ptr(X), _ptr(dOut), ctypes.byref(ws),
            _ptr(dX), _ptr(partial), _ptr(grad), int(acc), _stream())
    return dX, grad


def dense_forward(X, W, b, relu):
    """psvo_dense_forward: X (R, Din) -> act(X W + b) (R, Dout) on the f32 matrix instruction."""
    lib = _lib.load()
    R, Din = X.shape
    Dout = W.shape[1]
    _chk(X, (R, Din), "X"); _chk(W, (Din, Dout), "W"); _chk(b, (Dout,), "b")
    Y = _empty(R, Dout, device=X.device)
    _launch("psvo_dense_forward", lib.psvo_dense_forward, R, Din, Dout, _ptr(X), _ptr(W), _ptr(b), int(relu), _ptr(Y), _stream())
    return Y


def dense_backward(X, Y, dY, W, relu, need_dX=True):
    """psvo_dense_backward -> (dX (R, Din) or None, dW (Din, Dout), db (Dout))."""
    lib = _lib.load()
    R, Din = X.shape
    Dout = W.shape[1]
    _chk(X, (R, Din), "X"); _chk(dY, (R, Dout), "dY"); _chk(W, (Din, Dout), "W")
    if relu:
        _chk(Y, (R, Dout), "Y")
    dX = _empty(R, Din, device=X.device) if need_dX else None
    partial = _empty(lib.psvo_dense_wgrad_slices(R), (Din + 1) * Dout, device=X.device)
    grad = _empty((Din + 1) * Dout, device=X.device)
    _launch("psvo_dense_backward", lib.psvo_dense_backward, R, Din, Dout, _ptr(X), _ptr(Y) if relu else None, _ptr(dY), _ptr(W),
            int(relu), _ptr(dX), _ptr(partial), _ptr(grad), 0, _stream())
    return dX, grad[:Din * Dout].view(Din, Dout), grad[Din * Dout:]


def split_mlp_grad(g, Din, H, Dout, layers=1):
    """flat [dW1|db1|dW2|db2] -> (dW1 (Din,H), db1 (H), dW2 (H,Dout), db2 (Dout)) views; two hidden layers: flat
    [dW1|db1|dWh|dbh|dW2|db2] -> (dW1, db1, dW2, db2, dWh (H,H), dbh (H)), the order of the 6-tensor MLP tuples."""
    a = Din * H
    if layers == 2:
        b = a + H + H * H + H
        return (g[:a].view(Din, H), g[a:a + H], g[b:b + H * Dout].view(H, Dout), g[b + H * Dout:],
                g[a + H:a + H + H * H].view(H, H), g[a + H + H * H:b])
    return (g[:a].view(Din, H), g[a:a + H], g[a + H:a + H + H * Dout].view(H, Dout), g[a + H + H * Dout:])


def filter_backward(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, filt,
                    dlse=None, dFm=None, dlogW=None, gbufs=None, before_wgrad=None, defer_wgrad=False, wobs=False,
                    nparts=None, ext=False, adaptive=False, missing=False, hb=None):
    """psvo_filter_backward + psvo_mlp_wgrad (adaptive: psvo_filter_backward_adaptive, following the decisions filt["rs"]).
    `filt` = forward outputs.  dFm (T,B,Dx,N) / dlogW (T,B,N)
    are upstream gradients (or None); with nparts > 1 they come in parts, (T,B,nparts,Dx,N) / (T,B,nparts,N), which the
    kernel adds in part order.  Returns a dict of gradients.
    wobs: psvo_filter_backward_wobs + psvo_mlp_wgrad_wobs for MLP_g (wide observations); with dFm / dlogW -- a backward
    simulation ran behind the wide filter -- or with ext=True, psvo_filter_backward_wobs_ext.
    missing (with wobs): psvo_filter_backward_wobs_missing, 1 <= Dy <= 32 (with dFm / dlogW or ext=True -- the missing-observation
    backward simulation ran behind it -- psvo_filter_backward_wobs_missing_ext); MLP_g's weight gradient from the d G rows is
    psvo_mlp_wgrad_wobs for Dy >= 3 and the plain psvo_mlp_wgrad for Dy <= 2; with adaptive="wobs" as well,
    psvo_filter_backward_wobs_missing_adaptive, following filt["rs"] (dlse only).
    hb = (hb_q1, hb_f) (with wobs and missing, dlse only): psvo_filter_backward_wobs_input, the reverse of
    filter_forward_wobs_input; the weight gradients of MLP_q1 / MLP_f are psvo_mlp_wgrad_rowbias and the result also holds
    dhb_q1 and dhb_f (T,B,H; dhb_f None under bootstrap).  With adaptive="wobs" as well: psvo_filter_backward_wobs_input_adaptive,
    following filt["rs"]."""
    lib = _lib.load()
    B, T, N, Dx, Dy, H = desc.B, desc.T, desc.N, desc.Dx, desc.Dy, desc.H
    dev = eps.device
    q1s = _mlp_struct(q1, Dx, H, Dx, "q1")
    fs = None if desc.bootstrap else _mlp_struct(f, Dx, H, Dx, "f")
    gs = _mlp_struct(g, Dx, H, Dy, "g")
    if not wobs and (ext or nparts is not None):
        raise ValueError("filter_backward: `nparts` / `ext` belong to the wide-observation route (wobs=True)")
    parts = () if nparts in (None, 1) else (int(nparts),)
    _chk(dlse, (T, B), "dlse"); _chk(dFm, (T, B) + parts + (Dx, N), "dFm"); _chk(dlogW, (T, B) + parts + (N,), "dlogW")
    z = lambda *s: _empty(*s, device=dev)
    out = {"dP": z(T, B, Dx, N), "dF": None if desc.bootstrap else z(T, B, Dx, N), "dG": z(T, B, Dy, N),
           "dmu2": z(T, B, Dx) if desc.two_q else None, "dm0": z(B, Dx), "dfm0": z(B, Dx),
           "dsig_q1": z(Dx), "dsig_q2": z(Dx), "dsig_f": z(Dx), "dsig_g": z(Dy), "dsig0": z(Dx), "dfsig0": z(Dx)}
    nparts = (parts[0] if parts else 1) if (dFm is not None or dlogW is not None) else 0
    ext = bool(ext or nparts)
    name = ("psvo_filter_backward_wobs_ext" if ext else "psvo_filter_backward_wobs") if wobs else "psvo_filter_backward"
    wide_g = wobs                # MLP_g's weight gradient on psvo_mlp_wgrad_wobs
    if missing:
        # (adaptive == "wobs" with missing: filter_backward_wobs_missing_adaptive, below)
        if not wobs or (adaptive and adaptive != "wobs") or (ext and adaptive):
            raise ValueError("filter_backward: missing observations run on the wide-observation route (wobs=True), resampling at "
                             "every step or never; the adaptive form takes the upstream gradient dlse only (no gradients of "
                             "Fm / logW)")
        name, wide_g = "psvo_filter_backward_wobs_missing_ext" if ext else "psvo_filter_backward_wobs_missing", Dy >= 3
    decisions = ()
    if adaptive and missing:
        if filt.get("rs") is None:
            raise ValueError("filter_backward_wobs_missing_adaptive needs the forward pass's decisions filt['rs']")
        _chk(filt["rs"], (T, B), "filt['rs']", torch.int32)
        name = "psvo_filter_backward_wobs_missing_adaptive"
        decisions = (_ptr(filt["rs"]),)
    elif adaptive:
        if wobs and adaptive != "wobs":     # (the wide adaptive route is filter_backward_wobs_adaptive)
            raise ValueError("filter_backward: adaptive resampling belongs to the plain filter kernels (Dy <= 2)")
        if wobs and ext:
            raise ValueError("filter_backward_wobs_adaptive: no upstream gradient of Fm / logW (nothing runs behind an adaptive "
                             "filter under autograd)")
        if filt.get("rs") is None:
            raise ValueError("filter_backward(adaptive=True) needs the forward pass's decisions filt['rs']")
        _chk(filt["rs"], (T, B), "filt['rs']", torch.int32)
        name = "psvo_filter_backward_wobs_adaptive" if wobs else "psvo_filter_backward_adaptive"
        decisions = (_ptr(filt["rs"]),)
    if hb is not None:
        if not (wobs and missing) or ext:
            raise ValueError("filter_backward: the bias rows hb belong to psvo_filter_backward_wobs_input -- the missing-observation "
                             "route, upstream gradient dlse only")
        _chk(hb[0], (T, B, H), "hb_q1"); _chk(hb[1], (T, B, H), "hb_f")
        if hb[0] is None or (not desc.bootstrap and hb[1] is None):
            raise ValueError("filter_backward_wobs_input needs hb_q1 and, unless bootstrap, hb_f")
        # (adaptive: the decisions filt["rs"], checked above, ahead of the rows)
        name = "psvo_filter_backward_wobs_input_adaptive" if adaptive else "psvo_filter_backward_wobs_input"
        decisions = decisions + (_ptr(hb[0]), None if desc.bootstrap else _ptr(hb[1]))
    sacc = z((lib.psvo_filter_wobs_ws_floats if wobs else lib.psvo_filter_ws_floats)(B, T, N, Dx, Dy))
    upstream = (_ptr(dlse),) if (wobs and not ext) else (_ptr(dlse), nparts, _ptr(dFm), _ptr(dlogW))
    with _fixed_order():
        _launch(
            name, getattr(lib, name),
            ctypes.byref(desc), ctypes.byref(q1s), ctypes.byref(fs) if fs is not None else None, ctypes.byref(gs),
            _ptr(sig_q1), _ptr(sig_q2), _ptr(sig_f), _ptr(sig_g), _ptr(mu2), _ptr(m0), _ptr(sig0), _ptr(fm0), _ptr(fsig0),
            _ptr(obs), _ptr(eps), _ptr(filt["X"]), _ptr(filt["Fm"]), _ptr(filt["P1"]), _ptr(filt["logW"]),
            _ptr(filt["lse"]), _ptr(filt["idx"]), *upstream,
            _ptr(out["dP"]), _ptr(out["dF"]), _ptr(out["dG"]), _ptr(out["dmu2"]), _ptr(out["dm0"]), _ptr(out["dfm0"]),
            _ptr(out["dsig_q1"]), _ptr(out["dsig_q2"]), _ptr(out["dsig_f"]), _ptr(out["dsig_g"]), _ptr(out["dsig0"]),
            _ptr(out["dfsig0"]), _ptr(sacc), *decisions, _stream())
    # weight gradients from rows; gbufs = (q1, f, g) slices of the flat gradient buffer to accumulate into
    # directly (then no gradient tensor is returned for that MLP), or None
    gb = gbufs or (None, None, None)

    def wgrad(g_stream=None, after=None):
        """the two or three weight-gradient launches; g_stream: issue MLP_g's on that stream (ordered after the event
        `after`, i.e. after this kernel's rows exist) beside MLP_q1's on the current one -- the caller joins both"""
        if hb is not None:      # the first-layer bias of a row's segment is b1 + hb[t,b]; the segment sums of d pre are d hb
            out["gq1"], out["dhb_q1"] = mlp_wgrad_rowbias(filt["X"], out["dP"], hb[0], q1, Dx, H, Dx, grad=gb[0])
            out["gf"], out["dhb_f"] = ((None, None) if desc.bootstrap else
                                       mlp_wgrad_rowbias(filt["X"], out["dF"], hb[1], f, Dx, H, Dx, grad=gb[1]))
        else:
            out["gq1"] = mlp_wgrad(filt["X"], out["dP"], q1, Dx, H, Dx, grad=gb[0])
            out["gf"] = None if desc.bootstrap else mlp_wgrad(filt["X"], out["dF"], f, Dx, H, Dx, grad=gb[1])
        if g_stream is not None and gb[2] is not None:
            g_stream.wait_event(after)
            for t in (filt["X"], out["dG"]):
                t.record_stream(g_stream)
            with launch_on(g_stream):
                out["gg"] = mlp_wgrad(filt["X"], out["dG"], g, Dx, H, Dy, grad=gb[2], wobs=wide_g)
        else:
            out["gg"] = mlp_wgrad(filt["X"], out["dG"], g, Dx, H, Dy, grad=gb[2], wobs=wide_g)
    if defer_wgrad:          # the caller issues them later (out["_wgrad"]()), e.g. after other writers of the same slices
        out["_wgrad"] = wgrad
        return out
    if before_wgrad is not None:
        before_wgrad()
    wgrad()
    return out


def filter_backward_wobs(*args, **kw):
    """psvo_filter_backward_wobs + psvo_mlp_wgrad (q1, f) + psvo_mlp_wgrad_wobs (g): the reverse of filter_forward_wobs;
    arguments and result of filter_backward (dFm / dlogW given: psvo_filter_backward_wobs_ext)."""
    return filter_backward(*args, wobs=True, **kw)


def filter_backward_wobs_adaptive(*args, **kw):
    """psvo_filter_backward_wobs_adaptive + psvo_mlp_wgrad (q1, f) + psvo_mlp_wgrad_wobs (g): the reverse of
    filter_forward_wobs_adaptive, following the decisions filt["rs"]; arguments and result of filter_backward (dlse only)."""
    return filter_backward(*args, wobs=True, adaptive="wobs", **kw)


def filter_backward_wobs_missing(*args, **kw):
    """psvo_filter_backward_wobs_missing + psvo_mlp_wgrad (q1, f; g at Dy <= 2) + psvo_mlp_wgrad_wobs (g at Dy >= 3): the reverse
    of filter_forward_wobs_missing; arguments and result of filter_backward (dlse only)."""
    return filter_backward(*args, wobs=True, missing=True, **kw)


def filter_backward_wobs_input(*args, hb, **kw):
    """psvo_filter_backward_wobs_input + psvo_mlp_wgrad_rowbias (q1, f) + MLP_g's weight gradient as in
    filter_backward_wobs_missing: the reverse of filter_forward_wobs_input; arguments of filter_backward (dlse only) plus
    hb = (hb_q1, hb_f); the result also holds dhb_q1 / dhb_f."""
    return filter_backward(*args, wobs=True, missing=True, hb=hb, **kw)


def filter_backward_wobs_input_adaptive(*args, hb, **kw):
    """psvo_filter_backward_wobs_input_adaptive + the weight gradients of filter_backward_wobs_input: the reverse of
    filter_forward_wobs_input_adaptive, following the decisions filt["rs"]; arguments and result of filter_backward_wobs_input."""
    return filter_backward(*args, wobs=True, missing=True, adaptive="wobs", hb=hb, **kw)


def filter_backward_wobs_missing_adaptive(*args, **kw):
    """psvo_filter_backward_wobs_missing_adaptive + the weight gradients of filter_backward_wobs_missing: the reverse of
    filter_forward_wobs_missing_adaptive, following the decisions filt["rs"]; arguments and result of filter_backward (dlse only)."""
    return filter_backward(*args, wobs=True, missing=True, adaptive="wobs", **kw)


# ---------------------------------------------------------------------------------------------
# state-dependent scales (FLAGS.output_cov and FLAGS.diag_cov): psvo_filter_forward_cov / psvo_filter_backward_cov.
# A per-particle MLP is the 6-tuple (W1, b1, W_mu, b_mu, W_sigma, b_sigma); the kernels take the two heads as one output
# layer, W2 = [W_mu | W_sigma] (H, 2 Dout).
# ---------------------------------------------------------------------------------------------
def _cov_struct(p, Din, H, Dout, name):
    """(psvo_mlp with the concatenated output layer, the tensors that must stay alive until the launch has been issued)"""
    W1, b1, Wm, bm, Ws, bs = p
    _chk(Wm, (H, Dout), name + ".W_mu"); _chk(bm, (Dout,), name + ".b_mu")
    _chk(Ws, (H, Dout), name + ".W_sigma"); _chk(bs, (Dout,), name + ".b_sigma")
    with _on_launch_stream():
        W2, b2 = torch.cat([Wm, Ws], dim=1).contiguous(), torch.cat([bm, bs]).contiguous()
    return _mlp_struct((W1, b1, W2, b2), Din, H, 2 * Dout, name), (W2, b2)


def _head_grads(p, X, rows_mu, rows_sig, Din, H, Dout, axis=2):
    """[W1 | b1 | W_head | b_head] of each head from its rows -> (dW1, db1, dW_mu, db_mu, dW_sigma, db_sigma)"""
    W1, b1, Wm, bm, Ws, bs = p
    gm = split_mlp_grad(mlp_wgrad(X, rows_mu, (W1, b1, Wm, bm), Din, H, Dout, axis=axis), Din, H, Dout)
    gs = split_mlp_grad(mlp_wgrad(X, rows_sig, (W1, b1, Ws, bs), Din, H, Dout, axis=axis), Din, H, Dout)
    return (gm[0] + gs[0], gm[1] + gs[1], gm[2], gm[3], gs[2], gs[3])


def filter_forward_cov(desc, q1, f, g, sigc_q1, sigc_f, sigc_g, mu2, sig2, m0, sig0, fm0, fsig0, obs, eps,
                       u=None, idx_in=None):
    """psvo_filter_forward_cov.  Returns dict(X, Xanc, Fm, Fs, P1, P1s, logW, idx, lse)."""
    lib = _lib.load()
    B, T, N, Dx, Dy, H = desc.B, desc.T, desc.N, desc.Dx, desc.Dy, desc.H
    dev = eps.device
    q1s, k1 = _cov_struct(q1, Dx, H, Dx, "q1")
    fs, k2 = (None, None) if desc.bootstrap else _cov_struct(f, Dx, H, Dx, "f")
    gs, k3 = _cov_struct(g, Dx, H, Dy, "g")
    _chk(sigc_q1, (Dx,), "sigc_q1"); _chk(sigc_g, (Dy,), "sigc_g")
    if desc.two_q:
        _chk(mu2, (T, B, Dx), "mu2"); _chk(sig2, (T, B, Dx), "sig2")
    if not desc.bootstrap:
        _chk(sigc_f, (Dx,), "sigc_f")
    for t, nm in ((m0, "m0"), (sig0, "sig0"), (fm0, "fm0"), (fsig0, "fsig0")):
        _chk(t, (B, Dx), nm)
    _chk(obs, (T, B, Dy), "obs"); _chk(eps, (T, B, Dx, N), "eps")
    _chk(u, (T, B, N), "u"); _chk(idx_in, (T, B, N), "idx_in", torch.int32)
    if desc.resample and u is None and idx_in is None:
        raise ValueError("resampling needs uniforms `u` or teacher-forced `idx_in`")
    z = lambda *s: _empty(*s, device=dev)
    out = {"X": z(T, B, Dx, N), "Xanc": z(T, B, Dx, N), "Fm": z(T, B, Dx, N), "Fs": z(T, B, Dx, N), "logW": z(T, B, N),
           "idx": _empty(T, B, N, device=dev, dtype=torch.int32), "lse": z(T, B),
           "P1": None if desc.bootstrap else z(T, B, Dx, N), "P1s": None if desc.bootstrap else z(T, B, Dx, N)}
    _launch(
        "psvo_filter_forward_cov", lib.psvo_filter_forward_cov,
        ctypes.byref(desc), ctypes.byref(q1s), ctypes.byref(fs) if fs is not None else None, ctypes.byref(gs),
        _ptr(sigc_q1), _ptr(sigc_f), _ptr(sigc_g), _ptr(mu2), _ptr(sig2), _ptr(m0), _ptr(sig0), _ptr(fm0), _ptr(fsig0),
        _ptr(obs), _ptr(eps), _ptr(u), _ptr(idx_in),
        _ptr(out["X"]), _ptr(out["Xanc"]), _ptr(out["Fm"]), _ptr(out["Fs"]), _ptr(out["P1"]), _ptr(out["P1s"]),
        _ptr(out["logW"]), _ptr(out["idx"]), _ptr(out["lse"]), _stream())
    del k1, k2, k3
    return out


def _ffbs_inputs(fn, desc, filt, sig_f, u, idx_in):
    """what ffbs_smooth and ffbs_sample (`fn`: the caller's name) check alike -> the filter's (X, Fm, Fs, logW)"""
    B, T, N, Dx = desc.B, desc.T, desc.N, desc.Dx
    X, Fm, Fs, logW = filt["X"], filt["Fm"], filt.get("Fs"), filt["logW"]
    if X is None or Fm is None or logW is None:
        raise ValueError("%s needs the filter's X, Fm and logW" % fn)
    _chk(X, (T, B, Dx, N), "X"); _chk(Fm, (T, B, Dx, N), "Fm"); _chk(Fs, (T, B, Dx, N), "Fs"); _chk(logW, (T, B, N), "logW")
    _chk(sig_f, (Dx,), "sig_f")
    if (Fs is None) == (sig_f is None):
        raise ValueError("%s takes exactly one transition scale: the filter's per-particle `Fs` or a constant `sig_f`" % fn)
    _chk(u, (T, B, N), "u"); _chk(idx_in, (T, B, N), "idx_in", torch.int32)
    return X, Fm, Fs, logW


def ffbs_smooth(desc, filt, sig_f=None, u=None, idx_in=None, want_draws=True):
    """psvo_ffbs_smooth: the marginal particle smoother on a forward filter's outputs.  `filt` is the dict filter_forward /
    filter_forward_cov returned (X, Fm, logW, and Fs for state-dependent scales); `sig_f` (Dx) is the constant transition
    scale -- exactly one of filt["Fs"] / sig_f.  `u` (T,B,N) uniforms or `idx_in` (T,B,N) int32 teacher-forced draws are needed
    when want_draws.  Returns dict(logWs (T,B,N), Xmean (T,B,Dx), ess (T,B), Xs (T,B,Dx,N), idx (T,B,N)); Xs / idx are None
    without draws.  Asynchronous on the launch stream."""
    lib = _lib.load()
    B, T, N, Dx = desc.B, desc.T, desc.N, desc.Dx
    X, Fm, Fs, logW = _ffbs_inputs("ffbs_smooth", desc, filt, sig_f, u, idx_in)
    if want_draws and u is None and idx_in is None:
        raise ValueError("smoothed draws need uniforms `u` or teacher-forced `idx_in`")
    dev = X.device
    out = {"logWs": _empty(T, B, N, device=dev), "Xmean": _empty(T, B, Dx, device=dev), "ess": _empty(T, B, device=dev),
           "Xs": _empty(T, B, Dx, N, device=dev) if want_draws else None,
           "idx": _empty(T, B, N, device=dev, dtype=torch.int32) if want_draws else None}
    if not want_draws:
        u = idx_in = None
    _launch("psvo_ffbs_smooth", lib.psvo_ffbs_smooth, ctypes.byref(desc), _ptr(X), _ptr(Fm), _ptr(Fs), _ptr(sig_f), _ptr(logW),
            _ptr(u), _ptr(idx_in), _ptr(out["logWs"]), _ptr(out["Xmean"]), _ptr(out["ess"]), _ptr(out["Xs"]), _ptr(out["idx"]),
            _stream())
    return out


def ffbs_sample(desc, filt, sig_f=None, u=None, idx_in=None):
    """psvo_ffbs_sample: N backward-sampled trajectories per sequence (FFBSi) on a forward filter's outputs.  `filt` and `sig_f`
    as for ffbs_smooth -- exactly one of filt["Fs"] / sig_f.  `u` (T,B,N) uniforms, one per trajectory and step, or `idx_in`
    (T,B,N) int32 teacher-forced indices; at least one, idx_in wins.  Returns dict(Xs (T,B,Dx,N) the paths, idx (T,B,N) int32
    their particle indices, logq (T,B,N) the log-probability of each pick given the path's successor, distinct (T,B) int32 the
    number of different particles the N paths pass through).  Asynchronous on the launch stream."""
    lib = _lib.load()
    B, T, N, Dx = desc.B, desc.T, desc.N, desc.Dx
    X, Fm, Fs, logW = _ffbs_inputs("ffbs_sample", desc, filt, sig_f, u, idx_in)
    if u is None and idx_in is None:
        raise ValueError("backward sampling needs uniforms `u` or teacher-forced `idx_in`")
    dev = X.device
    out = {"Xs": _empty(T, B, Dx, N, device=dev), "idx": _empty(T, B, N, device=dev, dtype=torch.int32),
           "logq": _empty(T, B, N, device=dev), "distinct": _empty(T, B, device=dev, dtype=torch.int32)}
    _launch("psvo_ffbs_sample", lib.psvo_ffbs_sample, ctypes.byref(desc), _ptr(X), _ptr(Fm), _ptr(Fs), _ptr(sig_f), _ptr(logW),
            _ptr(u), _ptr(idx_in), _ptr(out["Xs"]), _ptr(out["idx"]), _ptr(out["logq"]), _ptr(out["distinct"]), _stream())
    return out


def particle_forecast(desc, K, f, g, sig_f, sig_g, X, logW=None, obs=None, eps=None, missing=False, hb_f=None):
    """psvo_particle_forecast: the k-step predictive distribution, k = 0..K, of the weighted cloud `X` (T,B,Dx,N) at every origin.
    `f`, `g` are the MLP tuples of the transition and the emission at the kernels' width (one hidden layer), `sig_f` (Dx) and
    `sig_g` (Dy) their scales (sig_g may be None for the count emission).  `logW` (T,B,N) log-weights or None = equal weights,
    `obs` (T,B,Dy) or None = no predictive log-density, `eps` (K,T,B,Dx,N) standard normals or None = noise-free propagation.
    Returns dict(ymean, yvar (K+1,T,B,Dy), xmean (K+1,T,B,Dx), lpd (K+1,T,B) or None without obs; lpd is 0 where t + k >= T).
    missing: psvo_particle_forecast_missing -- a NaN in `obs` is an entry that was not observed, lpd sums the observed entries of
    the target row and is 0 where that row has none.
    hb_f (Tv,B,H), Tv >= T: psvo_particle_forecast_input -- the exogenous input's share of the first layer of `f` (whose W1 is then
    the state's rows W1[:Dx]); the transition of horizon k from origin t adds hb_f[t+k,b,:] to b1, nothing where t + k >= Tv; rows
    T .. Tv-1 are inputs planned past the data.  Observations are read as under `missing`.  Asynchronous on the launch stream."""
    lib = _lib.load()
    B, T, N, Dx, Dy, H = desc.B, desc.T, desc.N, desc.Dx, desc.Dy, desc.H
    K = int(K)
    if K < 0:
        raise ValueError("particle_forecast: K = %d horizons; K >= 0" % K)
    Tv = T
    if hb_f is not None:
        Tv = int(hb_f.shape[0]) if hb_f.dim() == 3 else T
        if Tv < T:
            raise ValueError("hb_f must have shape (Tv, B, H) = (Tv, %d, %d) with Tv >= T = %d, got %s"
                             % (B, H, T, tuple(hb_f.shape)))
        _chk(hb_f, (Tv, B, H), "hb_f")
    if X is None:
        raise ValueError("particle_forecast needs the cloud X (T,B,Dx,N)")
    _chk(X, (T, B, Dx, N), "X"); _chk(logW, (T, B, N), "logW"); _chk(obs, (T, B, Dy), "obs")
    _chk(eps, (K, T, B, Dx, N), "eps"); _chk(sig_f, (Dx,), "sig_f"); _chk(sig_g, (Dy,), "sig_g")
    if eps is not None and sig_f is None:
        raise ValueError("particle_forecast: transition noise `eps` needs the transition scale `sig_f`")
    if sig_g is None and desc.emission != 2:
        raise ValueError("particle_forecast: the emission scale `sig_g` may be None for the count emission only")
    fs, gs = _mlp_struct(f, Dx, H, Dx, "f"), _mlp_struct(g, Dx, H, Dy, "g")
    dev = X.device
    out = {"ymean": _empty(K + 1, T, B, Dy, device=dev), "yvar": _empty(K + 1, T, B, Dy, device=dev),
           "xmean": _empty(K + 1, T, B, Dx, device=dev), "lpd": _empty(K + 1, T, B, device=dev) if obs is not None else None}
    name = "psvo_particle_forecast_missing" if missing else "psvo_particle_forecast"
    extra = ()
    if hb_f is not None:
        name, extra = "psvo_particle_forecast_input", (_ptr(hb_f), Tv)
    _launch(name, getattr(lib, name), ctypes.byref(desc), K, ctypes.byref(fs), ctypes.byref(gs),
            _ptr(sig_f), _ptr(sig_g), _ptr(X), _ptr(logW), _ptr(obs), _ptr(eps), _ptr(out["ymean"]), _ptr(out["yvar"]),
            _ptr(out["xmean"]), _ptr(out["lpd"]), *extra, _stream())
    return out


def map_path(desc, filt, g, sig_f, sig_g, fm0, fsig0, obs):
    """psvo_map_path: the MAP trajectory (particle Viterbi) through the particles of a forward filter.  `filt` is the dict the
    filter returned (X and Fm (T,B,Dx,N) are read; the weights are not), `g` the emission's MLP tuple at the kernels' width (one
    hidden layer), `sig_f` (Dx) the constant transition scale the filter weighted with, `sig_g` (Dy) the emission scale (may be
    None for the count emission), `fm0` (B,Dx) and `fsig0` (Dx) the t = 0 transition term, `obs` (T,B,Dy) with NaN = not
    observed.  Returns dict(delta (T,B,N), lmax (T,B), bp (T,B,N) int32, path (T,B) int32, Xmap (T,B,Dx)); sum_t lmax is the
    joint log-density of the path.  Asynchronous on the launch stream."""
    lib = _lib.load()
    B, T, N, Dx, Dy, H = desc.B, desc.T, desc.N, desc.Dx, desc.Dy, desc.H
    X, Fm = filt.get("X"), filt.get("Fm")
    if X is None or Fm is None:
        raise ValueError("map_path needs the filter's X and Fm")
    if filt.get("Fs") is not None:
        raise ValueError("map_path takes a constant transition scale `sig_f`; the filter left a scale per particle (Fs)")
    if sig_f is None or fm0 is None or fsig0 is None or obs is None:
        raise ValueError("map_path needs sig_f (Dx), fm0 (B,Dx), fsig0 (Dx) and obs (T,B,Dy)")
    if N > 512:
        raise ValueError("map_path: N = %d particles; the MAP-path kernel holds a sequence in one workgroup, N <= 512" % N)
    _chk(X, (T, B, Dx, N), "X"); _chk(Fm, (T, B, Dx, N), "Fm"); _chk(obs, (T, B, Dy), "obs")
    _chk(sig_f, (Dx,), "sig_f"); _chk(sig_g, (Dy,), "sig_g"); _chk(fm0, (B, Dx), "fm0"); _chk(fsig0, (Dx,), "fsig0")
    if sig_g is None and desc.emission != 2:
        raise ValueError("map_path: the emission scale `sig_g` may be None for the count emission only")
    gs = _mlp_struct(g, Dx, H, Dy, "g")
    dev = X.device
    out = {"delta": _empty(T, B, N, device=dev), "lmax": _empty(T, B, device=dev),
           "bp": _empty(T, B, N, device=dev, dtype=torch.int32), "path": _empty(T, B, device=dev, dtype=torch.int32),
           "Xmap": _empty(T, B, Dx, device=dev)}
    _launch("psvo_map_path", lib.psvo_map_path, ctypes.byref(desc), ctypes.byref(gs), _ptr(sig_f), _ptr(sig_g), _ptr(fm0),
            _ptr(fsig0), _ptr(obs), _ptr(X), _ptr(Fm), _ptr(out["delta"]), _ptr(out["lmax"]), _ptr(out["bp"]), _ptr(out["path"]),
            _ptr(out["Xmap"]), _stream())
    return out


def filter_backward_cov(desc, q1, f, g, sigc_q1, sigc_f, sigc_g, mu2, sig2, m0, sig0, fm0, fsig0, obs, eps, filt,
                        dlse=None, dFm=None, dFs=None, dlogW=None):
    """psvo_filter_backward_cov + two psvo_mlp_wgrad launches per MLP (one per head; both contribute to dW1 / db1).
    Returns a dict of gradients; the MLP entries gq1 / gf / gg are 6-tuples in the order of the MLP tuples."""
    lib = _lib.load()
    B, T, N, Dx, Dy, H = desc.B, desc.T, desc.N, desc.Dx, desc.Dy, desc.H
    dev = eps.device
    boot = bool(desc.bootstrap)
    q1s, k1 = _cov_struct(q1, Dx, H, Dx, "q1")
    fs, k2 = (None, None) if boot else _cov_struct(f, Dx, H, Dx, "f")
    gs, k3 = _cov_struct(g, Dx, H, Dy, "g")
    _chk(dlse, (T, B), "dlse"); _chk(dFm, (T, B, Dx, N), "dFm"); _chk(dFs, (T, B, Dx, N), "dFs")
    _chk(dlogW, (T, B, N), "dlogW")
    z = lambda *s: _empty(*s, device=dev)
    rows = lambda D: (z(T, B, D, N), z(T, B, D, N))
    out = {"dP": rows(Dx), "dF": (None, None) if boot else rows(Dx), "dG": rows(Dy),
           "dmu2": z(T, B, Dx) if desc.two_q else None, "dsig2": z(T, B, Dx) if desc.two_q else None,
           "dm0": z(B, Dx), "dsig0": z(B, Dx), "dfm0": z(B, Dx), "dfsig0": z(B, Dx),
           "dsigc_q1": z(Dx), "dsigc_f": None if boot else z(Dx), "dsigc_g": z(Dy)}
    ws = z(lib.psvo_filter_cov_ws_floats(B, T, N, Dx, Dy))
    with _fixed_order():
        _launch(
            "psvo_filter_backward_cov", lib.psvo_filter_backward_cov,
            ctypes.byref(desc), ctypes.byref(q1s), ctypes.byref(fs) if fs is not None else None, ctypes.byref(gs),
            _ptr(sigc_q1), _ptr(sigc_f), _ptr(sigc_g), _ptr(mu2), _ptr(sig2), _ptr(m0), _ptr(sig0), _ptr(fm0), _ptr(fsig0),
            _ptr(obs), _ptr(eps), _ptr(filt["X"]), _ptr(filt["Fm"]), _ptr(filt["Fs"]), _ptr(filt["P1"]), _ptr(filt["P1s"]),
            _ptr(filt["logW"]), _ptr(filt["lse"]), _ptr(filt["idx"]), _ptr(dlse), _ptr(dFm), _ptr(dFs), _ptr(dlogW),
            _ptr(out["dP"][0]), _ptr(out["dP"][1]), _ptr(out["dF"][0]), _ptr(out["dF"][1]), _ptr(out["dG"][0]),
            _ptr(out["dG"][1]), _ptr(out["dmu2"]), _ptr(out["dsig2"]), _ptr(out["dm0"]), _ptr(out["dsig0"]),
            _ptr(out["dfm0"]), _ptr(out["dfsig0"]), _ptr(out["dsigc_q1"]), _ptr(out["dsigc_f"]), _ptr(out["dsigc_g"]),
            _ptr(ws), _stream())
    del k1, k2, k3
    out["gq1"] = _head_grads(q1, filt["X"], *out["dP"], Dx, H, Dx)
    out["gf"] = None if boot else _head_grads(f, filt["X"], *out["dF"], Dx, H, Dx)
    out["gg"] = _head_grads(g, filt["X"], *out["dG"], Dx, H, Dy)
    return out


# The cov backward simulations (PSVO: bsim_*_cov, PSVOwR: bsimwr_*_cov) take the same inputs ahead of their own and their reverse
# launches write the same outputs: what the four wrappers share is below; the argument lists mirror include/psvo_hip.h in each.
def _bsim_cov_structs(desc, f, g, q1_inv):
    """the psvo_mlp structs of f, g, q1_inv, and their concatenated heads: keep those until the launch has been issued"""
    Dx, Dy, H = desc.Dx, desc.Dy, desc.H
    fs, k1 = _cov_struct(f, Dx, H, Dx, "f")
    gs, k2 = _cov_struct(g, Dx, H, Dy, "g")
    qs, k3 = _cov_struct(q1_inv, Dx, H, Dx, "q1_inv")
    return fs, gs, qs, (k1, k2, k3)


def _bsim_cov_chk(desc, filt, sigc_f, sigc_g, sigc_q1inv, bmu2, bsig2, minit, sinit, imean, isig, obs, eps_b, u_b, sel_in):
    B, T, N, M, Dx, Dy = desc.B, desc.T, desc.N, desc.M, desc.Dx, desc.Dy
    _chk(filt["Fm"], (T, B, Dx, N), "Fm"); _chk(filt["Fs"], (T, B, Dx, N), "Fs")
    _chk(filt["logW"], (T, B, N), "logW"); _chk(filt["lse"], (T, B), "lse")
    _chk(sigc_f, (Dx,), "sigc_f"); _chk(sigc_g, (Dy,), "sigc_g"); _chk(sigc_q1inv, (Dx,), "sigc_q1inv")
    _chk(bmu2, (T, B, Dx), "bmu2"); _chk(bsig2, (T, B, Dx), "bsig2")
    for t, nm in ((minit, "minit"), (sinit, "sinit"), (imean, "imean"), (isig, "isig")):
        _chk(t, (B, Dx), nm)
    _chk(obs, (T, B, Dy), "obs"); _chk(eps_b, (T, B, Dx, N, M), "eps_b")
    _chk(u_b, (T, B, N), "u_b"); _chk(sel_in, (T, B, N), "sel_in", torch.int32)


def _bsim_cov_saves(desc, dev, save):
    """what the reverse launch reads back (allocated when a reverse pass will follow)"""
    B, T, N, M, Dx = desc.B, desc.T, desc.N, desc.M, desc.Dx
    z = lambda *s: _empty(*s, device=dev) if save else None
    return {"lam": z(T, B, N, M), "om": z(T, B, N, M), "mu1": z(T, B, Dx, N), "s1": z(T, B, Dx, N)}


def _bsim_cov_grads(desc, dev):
    """the outputs of both reverse launches: the rows for psvo_mlp_wgrad, and the gradients the kernel accumulates into"""
    B, T, N, M, Dx, Dy = desc.B, desc.T, desc.N, desc.M, desc.Dx, desc.Dy
    z = lambda *s: _empty(*s, device=dev)
    zeros = lambda *s: _zeros(*s, device=dev)
    return {"xt": z(T, B, Dx, N, M), "dFt": z(T, B, Dx, N, M), "dFts": z(T, B, Dx, N, M), "dGt": z(T, B, Dy, N, M),
            "dGts": z(T, B, Dy, N, M), "dmu1": z(T, B, Dx, N), "dmu1s": z(T, B, Dx, N),
            # accumulated with float atomics by the kernel
            "dFm": zeros(T, B, Dx, N), "dFs": zeros(T, B, Dx, N), "dlogW": zeros(T, B, N), "dlse": zeros(T, B),
            "dbmu2": zeros(T, B, Dx), "dbsig2": zeros(T, B, Dx), "dminit": zeros(B, Dx), "dsinit": zeros(B, Dx),
            "dimean": zeros(B, Dx), "disig": zeros(B, Dx), "dsigc_f": zeros(Dx), "dsigc_g": zeros(Dy),
            "dsigc_q1inv": zeros(Dx)}


def _bsim_cov_det_ws(lib, desc, dev, det):
    """the fixed-order route's per-workgroup slices; allocated only in the mode"""
    return _empty(lib.psvo_bsim_cov_det_ws_floats(desc.B, desc.N, desc.M, desc.Dx, desc.Dy), device=dev) if det else None


def _bsim_cov_head_grads(out, desc, f, g, q1_inv, x_next):
    """gf / gg / gq1inv (6-tuples in the order of the MLP tuples) from the rows; x_next: what MLP_q1inv was evaluated at"""
    T, Dx, Dy, H = desc.T, desc.Dx, desc.Dy, desc.H
    out["gf"] = _head_grads(f, out["xt"][:T - 1], out["dFt"][:T - 1], out["dFts"][:T - 1], Dx, H, Dx)
    out["gg"] = _head_grads(g, out["xt"], out["dGt"], out["dGts"], Dx, H, Dy)
    out["gq1inv"] = _head_grads(q1_inv, x_next[1:], out["dmu1"][:T - 1], out["dmu1s"][:T - 1], Dx, H, Dx)


def bsim_forward_cov(desc, filt, f, g, q1_inv, sigc_f, sigc_g, sigc_q1inv, bmu2, bsig2, minit, sinit, imean, isig,
                     obs, eps_b, u_b=None, sel_in=None, save=False):
    """psvo_bsim_forward_cov.  Returns dict(bwX, flp, glp, Omega, sel, score[, lam, om, mu1, s1])."""
    lib = _lib.load()
    B, T, N, Dx = desc.B, desc.T, desc.N, desc.Dx
    dev = eps_b.device
    fs, gs, qs, keep = _bsim_cov_structs(desc, f, g, q1_inv)
    _bsim_cov_chk(desc, filt, sigc_f, sigc_g, sigc_q1inv, bmu2, bsig2, minit, sinit, imean, isig, obs, eps_b, u_b, sel_in)
    if u_b is None and sel_in is None:
        raise ValueError("the backward simulation needs uniforms `u_b` or teacher-forced `sel_in`")
    z = lambda *s: _empty(*s, device=dev)
    out = {"bwX": z(T, B, Dx, N), "flp": z(T, B, N), "glp": z(T, B, N), "Omega": z(T, B, N),
           "sel": _empty(T, B, N, device=dev, dtype=torch.int32), "score": z(B, N), **_bsim_cov_saves(desc, dev, save)}
    _launch(
        "psvo_bsim_forward_cov", lib.psvo_bsim_forward_cov,
        ctypes.byref(desc), _ptr(filt["Fm"]), _ptr(filt["Fs"]), _ptr(filt["logW"]), _ptr(filt["lse"]),
        ctypes.byref(fs), ctypes.byref(gs), ctypes.byref(qs), _ptr(sigc_f), _ptr(sigc_g), _ptr(sigc_q1inv),
        _ptr(bmu2), _ptr(bsig2), _ptr(minit), _ptr(sinit), _ptr(imean), _ptr(isig), _ptr(obs), _ptr(eps_b), _ptr(u_b),
        _ptr(sel_in), _ptr(out["bwX"]), _ptr(out["flp"]), _ptr(out["glp"]), _ptr(out["Omega"]), _ptr(out["sel"]),
        _ptr(out["score"]), _ptr(out["lam"]), _ptr(out["om"]), _ptr(out["mu1"]), _ptr(out["s1"]), _stream())
    del keep
    return out


def bsim_backward_cov(desc, filt, f, g, q1_inv, sigc_f, sigc_g, sigc_q1inv, bmu2, bsig2, minit, sinit, imean, isig,
                      obs, eps_b, bs, dscore):
    """psvo_bsim_backward_cov + two psvo_mlp_wgrad launches per MLP (one per head).  `bs` = the forward call's outputs with
    its saves.  Returns a dict of gradients; gf / gg / gq1inv are 6-tuples in the order of the MLP tuples."""
    lib = _lib.load()
    dev = eps_b.device
    fs, gs, qs, keep = _bsim_cov_structs(desc, f, g, q1_inv)
    _chk(dscore, (desc.B, desc.N), "dscore")
    out = _bsim_cov_grads(desc, dev)
    with _fixed_order() as det:
        det_ws = _bsim_cov_det_ws(lib, desc, dev, det)
        _launch(
            "psvo_bsim_backward_cov", lib.psvo_bsim_backward_cov_ws,      # (the name the hook and the checks know it by)
            ctypes.byref(desc), _ptr(filt["Fm"]), _ptr(filt["Fs"]), _ptr(filt["logW"]), _ptr(filt["lse"]),
            ctypes.byref(fs), ctypes.byref(gs), ctypes.byref(qs), _ptr(sigc_f), _ptr(sigc_g), _ptr(sigc_q1inv),
            _ptr(bmu2), _ptr(bsig2), _ptr(minit), _ptr(sinit), _ptr(imean), _ptr(isig), _ptr(obs), _ptr(eps_b),
            _ptr(bs["bwX"]), _ptr(bs["sel"]), _ptr(bs["lam"]), _ptr(bs["om"]), _ptr(bs["mu1"]), _ptr(bs["s1"]), _ptr(dscore),
            _ptr(out["xt"]), _ptr(out["dFt"]), _ptr(out["dFts"]), _ptr(out["dGt"]), _ptr(out["dGts"]), _ptr(out["dmu1"]),
            _ptr(out["dmu1s"]), _ptr(out["dFm"]), _ptr(out["dFs"]), _ptr(out["dlogW"]), _ptr(out["dlse"]),
            _ptr(out["dbmu2"]), _ptr(out["dbsig2"]), _ptr(out["dminit"]), _ptr(out["dsinit"]), _ptr(out["dimean"]),
            _ptr(out["disig"]), _ptr(out["dsigc_f"]), _ptr(out["dsigc_g"]), _ptr(out["dsigc_q1inv"]), _ptr(det_ws),
            _stream())
    del keep
    _bsim_cov_head_grads(out, desc, f, g, q1_inv, bs["bwX"])
    return out


def bsimwr_forward_cov(desc, filt, f, g, q1_inv, sigc_f, sigc_g, sigc_q1inv, bmu2, bsig2, minit, sinit, imean, isig,
                       obs, eps_b, u_b=None, u_r=None, sel_in=None, anc_in=None, save=False):
    """psvo_bsimwr_forward_cov (PSVOwR, state-dependent scales).  Returns dict(bwX, bwXanc, bwW, lseW, sel, anc, omsel
    [, lam, om, mu1, s1])."""
    lib = _lib.load()
    B, T, N, Dx = desc.B, desc.T, desc.N, desc.Dx
    dev = eps_b.device
    fs, gs, qs, keep = _bsim_cov_structs(desc, f, g, q1_inv)
    _bsim_cov_chk(desc, filt, sigc_f, sigc_g, sigc_q1inv, bmu2, bsig2, minit, sinit, imean, isig, obs, eps_b, u_b, sel_in)
    _chk(u_r, (T, B, N), "u_r"); _chk(anc_in, (T, B, N), "anc_in", torch.int32)
    if (u_b is None and sel_in is None) or (u_r is None and anc_in is None):
        raise ValueError("PSVOwR needs uniforms (`u_b`, `u_r`) or teacher-forced indices (`sel_in`, `anc_in`)")
    z = lambda *s: _empty(*s, device=dev)
    zi = lambda *s: _empty(*s, device=dev, dtype=torch.int32)
    out = {"bwX": z(T, B, Dx, N), "bwXanc": z(T, B, Dx, N), "bwW": z(T, B, N), "lseW": z(T, B), "sel": zi(T, B, N),
           "anc": zi(T, B, N), "omsel": z(T, B, N), **_bsim_cov_saves(desc, dev, save)}
    _launch(
        "psvo_bsimwr_forward_cov", lib.psvo_bsimwr_forward_cov,
        ctypes.byref(desc), _ptr(filt["Fm"]), _ptr(filt["Fs"]), _ptr(filt["logW"]), _ptr(filt["lse"]),
        ctypes.byref(fs), ctypes.byref(gs), ctypes.byref(qs), _ptr(sigc_f), _ptr(sigc_g), _ptr(sigc_q1inv),
        _ptr(bmu2), _ptr(bsig2), _ptr(minit), _ptr(sinit), _ptr(imean), _ptr(isig), _ptr(obs), _ptr(eps_b), _ptr(u_b),
        _ptr(u_r), _ptr(sel_in), _ptr(anc_in), _ptr(out["bwX"]), _ptr(out["bwXanc"]), _ptr(out["bwW"]), _ptr(out["lseW"]),
        _ptr(out["sel"]), _ptr(out["anc"]), _ptr(out["omsel"]), _ptr(out["lam"]), _ptr(out["om"]), _ptr(out["mu1"]),
        _ptr(out["s1"]), _stream())
    del keep
    return out


def bsimwr_backward_cov(desc, filt, f, g, q1_inv, sigc_f, sigc_g, sigc_q1inv, bmu2, bsig2, minit, sinit, imean, isig,
                        obs, eps_b, bs, dlseW):
    """psvo_bsimwr_backward_cov + two psvo_mlp_wgrad launches per MLP.  `bs` = the forward call's outputs with its saves."""
    lib = _lib.load()
    dev = eps_b.device
    fs, gs, qs, keep = _bsim_cov_structs(desc, f, g, q1_inv)
    _chk(dlseW, (desc.T, desc.B), "dlseW")
    out = _bsim_cov_grads(desc, dev)
    dXs = _zeros(desc.T, desc.B, desc.Dx, desc.N, device=dev)
    with _fixed_order() as det:
        det_ws = _bsim_cov_det_ws(lib, desc, dev, det)
        _launch(
            "psvo_bsimwr_backward_cov", lib.psvo_bsimwr_backward_cov_ws,      # (as above)
            ctypes.byref(desc), _ptr(filt["Fm"]), _ptr(filt["Fs"]), _ptr(filt["logW"]), _ptr(filt["lse"]),
            ctypes.byref(fs), ctypes.byref(gs), ctypes.byref(qs), _ptr(sigc_f), _ptr(sigc_g), _ptr(sigc_q1inv),
            _ptr(bmu2), _ptr(bsig2), _ptr(minit), _ptr(sinit), _ptr(imean), _ptr(isig), _ptr(obs), _ptr(eps_b),
            _ptr(bs["bwXanc"]), _ptr(bs["bwW"]), _ptr(bs["lseW"]), _ptr(bs["sel"]), _ptr(bs["anc"]), _ptr(bs["lam"]),
            _ptr(bs["om"]), _ptr(bs["mu1"]), _ptr(bs["s1"]), _ptr(dlseW),
            _ptr(out["xt"]), _ptr(out["dFt"]), _ptr(out["dFts"]), _ptr(out["dGt"]), _ptr(out["dGts"]), _ptr(out["dmu1"]),
            _ptr(out["dmu1s"]), _ptr(out["dFm"]), _ptr(out["dFs"]), _ptr(out["dlogW"]), _ptr(out["dlse"]),
            _ptr(out["dbmu2"]), _ptr(out["dbsig2"]), _ptr(out["dminit"]), _ptr(out["dsinit"]), _ptr(out["dimean"]),
            _ptr(out["disig"]), _ptr(out["dsigc_f"]), _ptr(out["dsigc_g"]), _ptr(out["dsigc_q1inv"]), _ptr(dXs),
            _ptr(det_ws), _stream())
    del keep
    _bsim_cov_head_grads(out, desc, f, g, q1_inv, bs["bwXanc"])
    return out


def _chain_rows(out, z, T, B, Dx, N):
    """per-chain rows of d bmu2 (T,B,Dx,N), d minit and d imean (B,Dx,N) in ONE buffer, so that one reduction over the
    chains serves all three (they sit on the dependent chain in front of the encoder BPTT)"""
    rows = z((T + 2) * B * Dx, N)
    n = T * B * Dx
    out["chain_rows"] = rows
    out["dbmu2_rows"] = rows[:n].view(T, B, Dx, N)
    out["dminit_rows"] = rows[n:n + B * Dx].view(B, Dx, N)
    out["dimean_rows"] = rows[n + B * Dx:].view(B, Dx, N)


def sum_chain_rows(out, T, B, Dx):
    """d bmu2 (T,B,Dx), d minit, d imean (B,Dx) from the chain rows of bsim_backward / bsimwr_backward.  Called by the
    autograd node when it returns, i.e. AFTER the weight-gradient launches were enqueued: issued between the kernel and
    those launches it changes the captured graph's topology, and the hipGraph executor then ran the filter's reverse pass
    and the weight gradients one after the other (+0.45 ms per replayed step at C*)."""
    s = out["chain_rows"].sum(-1)
    n = T * B * Dx
    out["dbmu2"], out["dminit"], out["dimean"] = s[:n].view(T, B, Dx), s[n:n + B * Dx].view(B, Dx), s[n + B * Dx:].view(B, Dx)


def bsim_backward(desc, filt, f, g, q1_inv, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2, minit, sig_init, imean, isig,
                  obs, eps_b, bs, dscore, gbufs=None, after_kernel=None, wgrad_stream=None, defer_wgrad=False):
    """psvo_bsim_backward + psvo_mlp_wgrad.  `bs` = bsim_forward(..., save=True) outputs."""
    lib = _lib.load()
    B, T, N, Dx, Dy = desc.B, desc.T, desc.N, desc.Dx, desc.Dy
    dev = eps_b.device
    fs, gs, qs = _bsim_structs(desc, f, g, q1_inv)
    _chk(dscore, (B, N), "dscore")
    _bsim_chk_saves(desc, bs, "bsim", (("bwX", (T, B, Dx, N)),))
    nblk = lib.psvo_bsim_blocks(ctypes.byref(desc))
    z = lambda *s: _empty(*s, device=dev)
    out = _bsim_grads(desc, dev, nblk, (("dFm", (T, B, Dx, N)), ("dlogW", (T, B, N)), ("dlse", (T, B))))
    _chain_rows(out, z, T, B, Dx, N)
    sacc = z(B, nblk, lib.psvo_bsim_acc_size(Dx, Dy))
    _launch(
        "psvo_bsim_backward", lib.psvo_bsim_backward,
        ctypes.byref(desc), _ptr(filt["Fm"]), _ptr(filt["logW"]), _ptr(filt["lse"]),
        ctypes.byref(fs), ctypes.byref(gs), ctypes.byref(qs),
        _ptr(sig_f), _ptr(sig_g), _ptr(sig_q1inv), _ptr(sig_bq2), _ptr(bmu2), _ptr(minit), _ptr(sig_init),
        _ptr(imean), _ptr(isig), _ptr(obs), _ptr(eps_b), _ptr(bs["bwX"]), _ptr(bs["sel"]),
        _ptr(bs["lam2"]), _ptr(bs["om"]), _ptr(bs["mu1"]), _ptr(dscore),
        _ptr(out["xt"]), _ptr(out["dFt"]), _ptr(out["dGt"]), _ptr(out["dmu1"]),
        _ptr(out["dFm_part"]), _ptr(out["dlogW_part"]), _ptr(out["dbmu2_rows"]), _ptr(out["dminit_rows"]),
        _ptr(out["dimean_rows"]), _ptr(sacc), _stream())
    # one more launch folds the per-workgroup partials into d Fm / d logW (which feed the filter's reverse pass) and the
    # scale gradients; then the caller publishes them
    _launch(
        "psvo_bsim_backward_fold", lib.psvo_bsim_backward_fold,
        ctypes.byref(desc), _ptr(out["dFm_part"]), _ptr(out["dlogW_part"]), _ptr(sacc), _ptr(sig_q1inv), _ptr(sig_bq2),
        _ptr(out["dFm"]), _ptr(out["dlogW"]), _ptr(out["dsig_f"]), _ptr(out["dsig_g"]), _ptr(out["dsig_q1inv"]),
        _ptr(out["dsig_bq2"]), _ptr(out["dsig_init"]), _ptr(out["disig"]), _ptr(out["dlse"]), _stream())
    if after_kernel is not None:
        after_kernel(out)
    # weight gradients from rows; gbufs = (f, g, q1_inv) slices of the flat gradient buffer to accumulate into, or None.  wgrad_stream
    # (only with gbufs: nothing is returned that the caller would read): issue them there, ordered after the kernel above
    wgrad = lambda: _bsim_wgrad(out, desc, f, g, q1_inv, bs["bwX"], gbufs or (None, None, None))
    if defer_wgrad:      # the caller issues them (out["_wgrad"]() under launch_on(stream), ordered after this kernel)
        out["_wgrad"] = wgrad
        return out
    with _wgrad_on(wgrad_stream if gbufs is not None else None):
        wgrad()
    return out


def bsim_backward_wobs(desc, filt, f, g, q1_inv, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2, minit, sig_init, imean, isig,
                       obs, eps_b, bs, dscore, missing=False):
    """psvo_bsim_backward_wobs + psvo_mlp_wgrad (f, q1_inv) + psvo_mlp_wgrad_wobs (g): the reverse of bsim_forward_wobs.
    `bs` = bsim_forward_wobs(..., save=True) outputs.  One stream; the result has bsim_backward's keys (no partials: the
    entry point folds them itself).
    missing: psvo_bsim_backward_wobs_missing, the reverse of bsim_forward_wobs_missing (1 <= Dy <= 32); MLP_g's weight gradient
    from the d G rows is psvo_mlp_wgrad_wobs for Dy >= 3 and the plain psvo_mlp_wgrad for Dy <= 2."""
    lib = _lib.load()
    B, T, N, M, Dx, Dy, H = desc.B, desc.T, desc.N, desc.M, desc.Dx, desc.Dy, desc.H
    dev = eps_b.device
    fs, gs, qs = _bsim_structs(desc, f, g, q1_inv)
    _bsim_chk(desc, filt, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2, minit, sig_init, imean, isig, obs, eps_b, None, None)
    _chk(dscore, (B, N), "dscore")
    _bsim_chk_saves(desc, bs, "bsim", (("bwX", (T, B, Dx, N)),))
    _chk(bs["sel"], (T, B, N), "sel", torch.int32)
    z = lambda *s: _empty(*s, device=dev)
    out = _bsim_grads(desc, dev, 0, (("dFm", (T, B, Dx, N)), ("dlogW", (T, B, N)), ("dlse", (T, B))))
    _chain_rows(out, z, T, B, Dx, N)
    ws = z(max(1, lib.psvo_bsim_wobs_ws_floats(B, T, N, M, Dx, Dy)))
    name = "psvo_bsim_backward_wobs_missing" if missing else "psvo_bsim_backward_wobs"
    _launch(
        name, getattr(lib, name),
        ctypes.byref(desc), _ptr(filt["Fm"]), _ptr(filt["logW"]), _ptr(filt["lse"]),
        ctypes.byref(fs), ctypes.byref(gs), ctypes.byref(qs),
        _ptr(sig_f), _ptr(sig_g), _ptr(sig_q1inv), _ptr(sig_bq2), _ptr(bmu2), _ptr(minit), _ptr(sig_init),
        _ptr(imean), _ptr(isig), _ptr(obs), _ptr(eps_b), _ptr(bs["bwX"]), _ptr(bs["sel"]),
        _ptr(bs["lam2"]), _ptr(bs["om"]), _ptr(bs["mu1"]), _ptr(dscore),
        _ptr(out["xt"]), _ptr(out["dFt"]), _ptr(out["dGt"]), _ptr(out["dmu1"]),
        _ptr(out["dbmu2_rows"]), _ptr(out["dminit_rows"]), _ptr(out["dimean_rows"]),
        _ptr(out["dFm"]), _ptr(out["dlogW"]), _ptr(out["dlse"]),
        _ptr(out["dsig_f"]), _ptr(out["dsig_g"]), _ptr(out["dsig_q1inv"]), _ptr(out["dsig_bq2"]), _ptr(out["dsig_init"]),
        _ptr(out["disig"]), _ptr(ws), _stream())
    # weight gradients from rows: MLP_g's through the wide-output kernel with L = N M rows per (t, b) segment
    out["gf"] = mlp_wgrad(out["xt"][:T - 1], out["dFt"][:T - 1], f, Dx, H, Dx)
    out["gg"] = mlp_wgrad(out["xt"], out["dGt"], g, Dx, H, Dy, wobs=not missing or Dy >= 3)
    out["gq1inv"] = mlp_wgrad(bs["bwX"][1:], out["dmu1"][:T - 1], q1_inv, Dx, H, Dx)
    return out


def bsim_backward_wobs_missing(*args, **kw):
    """psvo_bsim_backward_wobs_missing + the weight gradients: the reverse of bsim_forward_wobs_missing; arguments and result of
    bsim_backward_wobs."""
    return bsim_backward_wobs(*args, missing=True, **kw)


def bsimwr_forward(desc, filt, f, g, q1_inv, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2, minit, sig_init,
                   imean, isig, obs, eps_b, u_b=None, u_r=None, sel_in=None, anc_in=None, save=False):
    """psvo_bsimwr_forward (PSVOwR).  Returns dict(bwX, bwXanc, bwW, lseW, sel, anc[, lam2, om, mu1])."""
    lib = _lib.load()
    B, T, N, Dx = desc.B, desc.T, desc.N, desc.Dx
    dev = eps_b.device
    fs, gs, qs = _bsim_structs(desc, f, g, q1_inv)
    _bsim_chk(desc, filt, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2, minit, sig_init, imean, isig, obs, eps_b, u_b, sel_in)
    _chk(u_r, (T, B, N), "u_r"); _chk(anc_in, (T, B, N), "anc_in", torch.int32)
    if (u_b is None and sel_in is None) or (u_r is None and anc_in is None):
        raise ValueError("PSVOwR needs uniforms (`u_b`, `u_r`) or teacher-forced indices (`sel_in`, `anc_in`)")
    z = lambda *s: _empty(*s, device=dev)
    zi = lambda *s: _empty(*s, device=dev, dtype=torch.int32)
    out = {"bwX": z(T, B, Dx, N), "bwXanc": z(T, B, Dx, N), "bwW": z(T, B, N), "lseW": z(T, B),
           "sel": zi(T, B, N), "anc": zi(T, B, N), **_bsim_saves(desc, dev, save),
           "ws": z(lib.psvo_bsimwr_ws_floats(B, T, N))}   # (its last word, as int32, is nonzero iff a cluster barrier timed out)
    _launch(
        "psvo_bsimwr_forward", lib.psvo_bsimwr_forward,
        ctypes.byref(desc), _ptr(filt["Fm"]), _ptr(filt["logW"]), _ptr(filt["lse"]),
        ctypes.byref(fs), ctypes.byref(gs), ctypes.byref(qs),
        _ptr(sig_f), _ptr(sig_g), _ptr(sig_q1inv), _ptr(sig_bq2), _ptr(bmu2), _ptr(minit), _ptr(sig_init),
        _ptr(imean), _ptr(isig), _ptr(obs), _ptr(eps_b), _ptr(u_b), _ptr(u_r), _ptr(sel_in), _ptr(anc_in),
        _ptr(out["bwX"]), _ptr(out["bwXanc"]), _ptr(out["bwW"]), _ptr(out["lseW"]), _ptr(out["sel"]),
        _ptr(out["anc"]), _ptr(out["lam2"]), _ptr(out["om"]), _ptr(out["mu1"]), _ptr(out["ws"]), _stream())
    return out


def bsimwr_backward(desc, filt, f, g, q1_inv, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2, minit, sig_init, imean, isig,
                    obs, eps_b, bs, dlseW, gbufs=None, after_kernel=None, wgrad_stream=None):
    """psvo_bsimwr_backward + psvo_mlp_wgrad.  `bs` = bsimwr_forward(..., save=True) outputs."""
    lib = _lib.load()
    B, T, N, Dx, Dy = desc.B, desc.T, desc.N, desc.Dx, desc.Dy
    dev = eps_b.device
    fs, gs, qs = _bsim_structs(desc, f, g, q1_inv)
    _chk(dlseW, (T, B), "dlseW")
    _bsim_chk_saves(desc, bs, "bsimwr", (("bwXanc", (T, B, Dx, N)), ("bwW", (T, B, N)), ("lseW", (T, B))))
    z = lambda *s: _empty(*s, device=dev)
    K = lib.psvo_bsimwr_blocks(B, N, desc.M)
    out = _bsim_grads(desc, dev, K, (("dlse_part", (T, B, K)),))
    out["ws"] = z(lib.psvo_bsimwr_bwd_ws_floats(B, T, N, Dx))
    _chain_rows(out, z, T, B, Dx, N)
    sacc = z(B, K, lib.psvo_bsim_acc_size(Dx, Dy))
    _launch(
        "psvo_bsimwr_backward", lib.psvo_bsimwr_backward,
        ctypes.byref(desc), _ptr(filt["Fm"]), _ptr(filt["logW"]), _ptr(filt["lse"]),
        ctypes.byref(fs), ctypes.byref(gs), ctypes.byref(qs),
        _ptr(sig_f), _ptr(sig_g), _ptr(sig_q1inv), _ptr(sig_bq2), _ptr(bmu2), _ptr(minit), _ptr(sig_init),
        _ptr(imean), _ptr(isig), _ptr(obs), _ptr(eps_b), _ptr(bs["bwXanc"]), _ptr(bs["bwW"]), _ptr(bs["lseW"]),
        _ptr(bs["sel"]), _ptr(bs["anc"]), _ptr(bs["lam2"]), _ptr(bs["om"]), _ptr(bs["mu1"]), _ptr(dlseW),
        _ptr(out["xt"]), _ptr(out["dFt"]), _ptr(out["dGt"]), _ptr(out["dmu1"]),
        _ptr(out["dFm_part"]), _ptr(out["dlogW_part"]), _ptr(out["dlse_part"]), _ptr(out["dbmu2_rows"]),
        _ptr(out["dminit_rows"]), _ptr(out["dimean_rows"]), _ptr(out["dsig_f"]), _ptr(out["dsig_g"]),
        _ptr(out["dsig_q1inv"]), _ptr(out["dsig_bq2"]), _ptr(out["dsig_init"]), _ptr(out["disig"]), _ptr(sacc),
        _ptr(out["ws"]), _stream())
    # fold the per-workgroup partials that feed the filter's reverse pass, then let the caller publish them
    out["dFm"] = out["dFm_part"].sum(2)
    out["dlogW"] = out["dlogW_part"].sum(2)
    out["dlse"] = out["dlse_part"].sum(2)
    if after_kernel is not None:
        after_kernel(out)
    with _wgrad_on(wgrad_stream if gbufs is not None else None):
        _bsim_wgrad(out, desc, f, g, q1_inv, bs["bwXanc"], gbufs or (None, None, None))
    return out


def reduce_rows(part, nrows, stride, n, out, accumulate=False):
    """psvo_reduce_rows: out[p] (+)= sum_r part[r*stride + p]; `part` may be a strided view (its data_ptr is used)."""
    lib = _lib.load()
    st = lib.psvo_reduce_rows(_ptr(part), nrows, stride, n, _ptr(out), int(accumulate), _stream())
    _lib.check(st, "psvo_reduce_rows")
    return out


def sigma_forward(raw, mins):
    lib = _lib.load()
    sig = _empty(raw.shape, device=raw.device, dtype=raw.dtype)
    _lib.check(lib.psvo_sigma_forward(_ptr(raw), _ptr(mins), _ptr(sig), raw.numel(), _stream()), "psvo_sigma_forward")
    return sig


def sigma_backward(raw, mins, dsig, graw, accumulate=True):
    lib = _lib.load()
    _lib.check(lib.psvo_sigma_backward(_ptr(raw), _ptr(mins), _ptr(dsig), _ptr(graw), raw.numel(), int(accumulate),
                                       _stream()), "psvo_sigma_backward")
    return graw


def bilstm_backward(x, W_fw, W_bw, out, cs, gates, dout, gbufs=None, need_dx=True):
    """psvo_bilstm_backward -> (dx (B,T,Din) or None, dW_fw, db_fw, dW_bw, db_bw)."""
    lib = _lib.load()
    B, T, Din = x.shape
    Dh = W_fw.shape[1] // 4
    _chk(dout, (B, T, 2 * Dh), "dout"); _chk(out, (B, T, 2 * Dh), "out")
    _chk(cs, (2, B, T, Dh), "cs"); _chk(gates, (2, B, T, 4 * Dh), "gates")
    dev = x.device
    dx_part = _empty(2, B, T, Din, device=dev)
    dW_part = _empty(B, 2, Din + Dh, 4 * Dh, device=dev)
    db_part = _empty(B, 2, 4 * Dh, device=dev)
    _launch("psvo_bilstm_backward", lib.psvo_bilstm_backward, B, T, Din, Dh, _ptr(x), _ptr(W_fw), _ptr(W_bw), _ptr(out), _ptr(cs),
            _ptr(gates), _ptr(dout), _ptr(dx_part), _ptr(dW_part), _ptr(db_part), _stream())
    dx = dx_part.sum(0) if need_dx else None     # (the first layer's input is the observations: no gradient wanted)
    K, G4 = Din + Dh, 4 * Dh
    if gbufs is not None and gbufs[0] is not None and gbufs[1] is not None:
        # fold the per-sequence partials straight into the flat gradient buffer: [kernel (K,4Dh) | bias (4Dh)] per cell
        _lib.check(lib.psvo_bilstm_wgrad_fold(B, Din, Dh, _ptr(dW_part), _ptr(db_part), _ptr(gbufs[0]), _ptr(gbufs[1]), 1,
                                              _stream()), "psvo_bilstm_wgrad_fold")
        return dx, None, None, None, None
    dW = dW_part.sum(0)
    db = db_part.sum(0)
    return dx, dW[0], db[0], dW[1], db[1]
