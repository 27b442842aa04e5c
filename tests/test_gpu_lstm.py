"""The bi-LSTM encoder kernels (psvo_bilstm_forward, psvo_bilstm_backward, psvo_bilstm_wgrad_fold) on their own, in every
(DINP, DH) template instantiation, against the fp64 oracle (oracle.psvo_oracle.stack_bidirectional_rnn / bidirectional_rnn /
static_rnn, torch autograd of (out * dout).sum() for a fixed random dout).

Tolerances -- every figure is measured against the reference, none is tuned to what the kernels return:
  forward quantities (out, cs, gates)   atol 2e-5, rtol 1e-5
  gradients, block by block             max|g - r| <= K32 * max(err32, 1e-6 * max|r|), K32 = 4, with r the fp64 value of the
                                        block and err32 = max|r32 - r| the error of the SAME oracle run in fp32.
A kernel gradient is split into (x-rows, h-rows) x (gates i, j, f, o) = 8 blocks, a bias gradient into its 4 gate blocks (a gate
block is as small as 2 - 12 % of its tensor's largest entry: a per-tensor bound would let a whole block be 10 % off); dx is
one block, and per time step where the sequence is long.  No block and no element is left out.

Worst ratio err / bound per test, measured on an MI355X (1.0 is the bound; `pytest -s` prints them again):
  1 every instantiation      forward 0.039 (<128,8> Din=65, gates)        gradients 0.293 (<128,8> Din=128, db_bw[f])
  2 long sequences           forward 0.053 (T=400 <128,64>, gates)        gradients 0.393 (T=1000 <4,32>, db_bw[f]);
                             dx per time step 0.395 (T=400 <4,32>, t=391)
  3 saturating gates         forward 0.173 (Din=64 Dh=64 kscale=8, gates) gradients 0.510 (Din=3 Dh=16 kscale=8, dW_bw[x-rows, f])
  4 edges                    forward 0.012                                gradients 0.102 (B=600 T=3, dx)
  5 every element written    bit-identical to the wrapper, no prefilled element left
  6 directions do not leak   dead direction exactly 0                     gradients 0.113 (keep bw, Din=33 Dh=32, dx)
  7 wgrad fold               0.802 of the summation bound gamma_B * sum|terms| (B=3); repeats bit-identical
  8 wirings                  forward 0.014 (uni)                          gradients 0.258 (multi, fw.0.kernel[h-rows, o])
No bound was raised and no fault was found: the kernels' error is that of the fp32 oracle, the four scratch builds included.
"""
import ctypes
import math

import pytest
import torch

from oracle import psvo_oracle as O
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

K32 = 4.0            # accepted multiple of the fp32 oracle's own error (tests/test_gpu_instantiations.py)
FLOOR = 1e-6         # ... which is never taken below ~8 ulp of the block's largest entry
ATOL, RTOL = 2e-5, 1e-5
GATES = "ijfo"

_WORST = {}          # test name -> (worst ratio, where); printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for k in sorted(_WORST):
        print("\n[test_gpu_lstm] worst err/bound %-44s %.3f  (%s)" % (k, _WORST[k][0], _WORST[k][1]))


def _note(test, ratio, where):
    if ratio > _WORST.get(test, (-1.0, ""))[0]:
        _WORST[test] = (ratio, where)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and the reference
# ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(B, T, Din, Dh, kscale=1.0, seed=0):
    """(x, W_fw, b_fw, W_bw, b_bw, dout) as fp32 CPU tensors: StackBiRNN's own initialiser (glorot kernels) times kscale,
    biases N(0, 0.3), x N(0, 1.5^2), dout N(0, 1)"""
    from psvo_amd.model import StackBiRNN
    torch.manual_seed(1000 + seed)
    enc = StackBiRNN(Din, [Dh], "enc")
    g = torch.Generator().manual_seed(2000 + seed)
    Wf = (enc.fw[0].kernel.detach() * kscale).clone()
    Wb = (enc.bw[0].kernel.detach() * kscale).clone()
    bf = torch.randn(4 * Dh, generator=g) * 0.3
    bb = torch.randn(4 * Dh, generator=g) * 0.3
    x = torch.randn(B, T, Din, generator=g) * 1.5
    dout = torch.randn(B, T, 2 * Dh, generator=g)
    return x, Wf, bf, Wb, bb, dout


def _saves(x, W, b, reverse):
    """cell states (B, T, Dh) and activated gates (B, T, 4 Dh) of one direction, stepping O.lstm_block_cell"""
    B, T, _ = x.shape
    Dh = W.shape[1] // 4
    h, c = x.new_zeros(B, Dh), x.new_zeros(B, Dh)
    cs, gates, hs = [None] * T, [None] * T, [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        i, j, f, o = (torch.cat([x[:, t], h], dim=-1) @ W + b).chunk(4, dim=-1)
        gates[t] = torch.cat([torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o)], dim=-1)
        h, c = O.lstm_block_cell(x[:, t], h, c, W, b)
        cs[t], hs[t] = c, h
    return torch.stack(cs, 1), torch.stack(gates, 1), torch.stack(hs, 1)


def oracle_layer(inp, dtype, which="both"):
    """one bidirectional layer in `dtype` on the CPU: forward values, saves and the gradients of (out * dout).sum().
    which = "fw" / "bw": only that direction runs (static_rnn; the backward cell as static_rnn on the time-reversed input)."""
    x, Wf, bf, Wb, bb, dout = (t.to(dtype).clone() for t in inp)
    leaves = [x, Wf, bf, Wb, bb]
    for t in leaves:
        t.requires_grad_(True)
    Dh = Wf.shape[1] // 4
    if which == "both":
        out = O.stack_bidirectional_rnn(x, [{"fw": (Wf, bf), "bw": (Wb, bb)}])
        loss = (out * dout).sum()
    elif which == "fw":
        out = O.static_rnn(x, [{"fw": (Wf, bf)}])
        loss = (out * dout[..., :Dh]).sum()
    else:
        out = O.static_rnn(x.flip(1), [{"fw": (Wb, bb)}]).flip(1)
        loss = (out * dout[..., Dh:]).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    r = {"out": out.detach().double()}
    for k, v in zip(("dx", "dW_fw", "db_fw", "dW_bw", "db_bw"), grads):
        r[k] = None if v is None else v.double()
    if which == "both":
        with torch.no_grad():
            cf, gf, hf = _saves(x, Wf, bf, False)
            cb, gb, hb = _saves(x, Wb, bb, True)
        assert torch.equal(torch.cat([hf, hb], -1), out.detach()), "the stepped cell and run_rnn disagree"
        r["cs"], r["gates"] = torch.stack([cf, cb]).double(), torch.stack([gf, gb]).double()
    return r


def gpu_layer(inp, save_only=False):
    from psvo_amd import ops
    x, Wf, bf, Wb, bb, dout = (t.float().cuda().contiguous() for t in inp)
    out, cs, gates = ops.bilstm_forward(x, Wf, bf, Wb, bb, save=True)
    g = {"out": out, "cs": cs, "gates": gates}
    if not save_only:
        keys = ("dx", "dW_fw", "db_fw", "dW_bw", "db_bw")
        g.update(zip(keys, ops.bilstm_backward(x, Wf, Wb, out, cs, gates, dout)))
    torch.cuda.synchronize()
    return {k: v.double().cpu() for k, v in g.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------
def grad_blocks(name, Din, Dh):
    """(label, index) of every block a gradient is compared in"""
    if name.startswith("dW"):
        for rl, rs in (("x", slice(0, Din)), ("h", slice(Din, Din + Dh))):
            for k, gl in enumerate(GATES):
                yield "%s[%s-rows, %s]" % (name, rl, gl), (rs, slice(k * Dh, (k + 1) * Dh))
    elif name.startswith("db"):
        for k, gl in enumerate(GATES):
            yield "%s[%s]" % (name, gl), (slice(k * Dh, (k + 1) * Dh),)
    else:
        yield name, (Ellipsis,)


def block_ratio(g, r, r32):
    """err / bound of one block (0 where both the error and the bound are 0), and the figures behind it"""
    assert torch.isfinite(r).all() and torch.isfinite(r32).all(), "the reference itself is not finite"
    if not torch.isfinite(g).all():
        return math.inf, (math.nan, 0.0, 0.0)
    err, err32, scale = float((g - r).abs().max()), float((r32 - r).abs().max()), float(r.abs().max())
    bound = K32 * max(err32, FLOOR * scale)
    return (0.0 if err == 0.0 else (err / bound if bound > 0 else math.inf)), (err, err32, scale)


def check_grads(test, case, got, r64, r32, Din, Dh, names, per_step=()):
    bad = []
    for name in names:
        for label, idx in grad_blocks(name, Din, Dh):
            ratio, fig = block_ratio(got[name][idx], r64[name][idx], r32[name][idx])
            _note(test, ratio, "%s %s" % (case, label))
            if not ratio <= 1.0:
                bad.append((label, "ratio %.3g" % ratio, "err %.3g err32 %.3g scale %.3g" % fig))
    for t in per_step:                              # dx of single time steps against that step's own largest entry
        ratio, fig = block_ratio(got["dx"][:, t], r64["dx"][:, t], r32["dx"][:, t])
        _note(test + " (dx per step)", ratio, "%s t=%d" % (case, t))
        if not ratio <= 1.0:
            bad.append(("dx[t=%d]" % t, "ratio %.3g" % ratio, "err %.3g err32 %.3g scale %.3g" % fig))
    assert not bad, "%s: gradient blocks beyond K32 x max(fp32 oracle's error, 1e-6 scale): %s" % (case, bad)


def check_forward(test, case, got, r64, names=("out", "cs", "gates")):
    bad = []
    for name in names:
        g, r = got[name], r64[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if not torch.isfinite(g).all():
            bad.append((name, "not finite"))
            continue
        ratio = float(((g - r).abs() / (ATOL + RTOL * r.abs())).max())
        _note(test, ratio, "%s %s" % (case, name))
        if not ratio <= 1.0:
            k = int(((g - r).abs() / (ATOL + RTOL * r.abs())).argmax())
            bad.append((name, "ratio %.3g at flat index %d of shape %s" % (ratio, k, tuple(g.shape))))
    assert not bad, "%s: forward quantities beyond atol 2e-5 + rtol 1e-5: %s" % (case, bad)


GRADS = ("dx", "dW_fw", "db_fw", "dW_bw", "db_bw")
_RUNS = {}


def run_case(B, T, Din, Dh, kscale=1.0, seed=0, edit=None):
    """(inputs, GPU results, fp64 oracle, fp32 oracle) of one case; computed once, shared by the tests that read it"""
    key = (B, T, Din, Dh, kscale, seed, edit)
    if key not in _RUNS:
        inp = make_inputs(B, T, Din, Dh, kscale, seed)
        if edit is not None:
            EDITS[edit](inp, Dh)
        _RUNS[key] = (inp, gpu_layer(inp), oracle_layer(inp, torch.float64), oracle_layer(inp, torch.float32))
    return _RUNS[key]


def _pad(Din):
    return next(p for p in (4, 16, 32, 64, 128) if Din <= p)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. every instantiation, forward and reverse
# ---------------------------------------------------------------------------------------------------------------------------
def _inside(DINP, DH):
    """a width inside the class that leaves padding rows"""
    alt = DH in (16, 64)
    return {4: 3 if alt else 1, 16: 5, 32: 17, 64: 33, 128: 100 if alt else 65}[DINP]


INSTANCES = [(DINP, DH, Din) for DINP in (4, 16, 32, 64, 128) for DH in (8, 16, 32, 64) for Din in (DINP, _inside(DINP, DH))]


@pytest.mark.parametrize("DINP,DH,Din", INSTANCES, ids=["fwd-DINP%d-DH%d-Din%d" % c for c in INSTANCES])
def test_forward_every_instantiation(built_lib, DINP, DH, Din):
    assert _pad(Din) == DINP
    _, got, r64, _ = run_case(3, 6, Din, DH, seed=DINP + DH + Din)
    check_forward("1 forward, every instantiation", "<%d,%d> Din=%d" % (DINP, DH, Din), got, r64)


@pytest.mark.parametrize("DINP,DH,Din", INSTANCES, ids=["bwd-DINP%d-DH%d-Din%d" % c for c in INSTANCES])
def test_backward_every_instantiation(built_lib, DINP, DH, Din):
    assert _pad(Din) == DINP
    _, got, r64, r32 = run_case(3, 6, Din, DH, seed=DINP + DH + Din)
    check_grads("1 backward, every instantiation", "<%d,%d> Din=%d" % (DINP, DH, Din), got, r64, r32, Din, DH, GRADS)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. long sequences
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,Din,Dh", [(400, 3, 32), (1000, 1, 32), (400, 128, 64)], ids=lambda v: str(v))
def test_long_sequences(built_lib, T, Din, Dh):
    _, got, r64, r32 = run_case(2, T, Din, Dh, seed=T + Dh)
    case = "T=%d <%d,%d>" % (T, _pad(Din), Dh)
    check_forward("2 long sequences, forward", case, got, r64)
    steps = list(range(10)) + list(range(T // 2 - 5, T // 2 + 5)) + list(range(T - 10, T))
    check_grads("2 long sequences", case, got, r64, r32, Din, Dh, GRADS, per_step=steps)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. saturating gates
# ---------------------------------------------------------------------------------------------------------------------------
def _huge_biases(inp, Dh):
    """+-100 on a few units of every gate, both cells: expf overflows inside the sigmoid; 1 - g^2 and g (1 - g) are exactly 0"""
    for b, shift in ((inp[2], 0), (inp[4], 1)):
        for k in range(4):
            b[k * Dh + (2 * k + shift) % Dh] = 100.0
            b[k * Dh + (2 * k + 1 + shift) % Dh] = -100.0


EDITS = {"huge_biases": _huge_biases}
SATURATING = [(2, 40, 3, 16, 4.0, None), (2, 40, 3, 16, 8.0, None), (2, 40, 64, 64, 4.0, None), (2, 40, 64, 64, 8.0, None),
              (2, 400, 2, 32, 4.0, None), (2, 40, 3, 16, 1.0, "huge_biases")]


@pytest.mark.parametrize("B,T,Din,Dh,kscale,edit", SATURATING,
                         ids=["B%d-T%d-Din%d-Dh%d-k%g-%s" % (c[:5] + (c[5] or "plain",)) for c in SATURATING])
def test_saturating_gates(built_lib, B, T, Din, Dh, kscale, edit):
    _, got, r64, r32 = run_case(B, T, Din, Dh, kscale, seed=7, edit=edit)
    case = "T=%d Din=%d Dh=%d kscale=%g %s" % (T, Din, Dh, kscale, edit or "")
    for k, v in got.items():
        assert torch.isfinite(v).all(), (case, k)
    if edit:                                     # the point of the case: saturated gates are exactly 0, 1 or -1 on the device
        assert all(bool((got["gates"] == v).any()) for v in (0.0, 1.0, -1.0))
    check_forward("3 saturating gates, forward", case, got, r64)
    check_grads("3 saturating gates", case, got, r64, r32, Din, Dh, GRADS)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. edges of the time loop and the grid
# ---------------------------------------------------------------------------------------------------------------------------
EDGES = [(3, 1, 5, 16), (3, 2, 5, 16), (1, 6, 3, 32), (600, 3, 2, 32)]


@pytest.mark.parametrize("B,T,Din,Dh", EDGES, ids=["B%d-T%d-Din%d-Dh%d" % c for c in EDGES])
def test_time_loop_and_grid_edges(built_lib, B, T, Din, Dh):
    from psvo_amd import ops
    inp, got, r64, r32 = run_case(B, T, Din, Dh, seed=11)
    case = "B=%d T=%d Din=%d Dh=%d" % (B, T, Din, Dh)
    check_forward("4 edges, forward", case, got, r64)
    check_grads("4 edges", case, got, r64, r32, Din, Dh, GRADS)
    # save=False passes NULL for the saves: the same out, bit for bit
    out = ops.bilstm_forward(*(t.cuda() for t in inp[:5]), save=False)
    assert torch.equal(out.double().cpu(), got["out"])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. every output element is written
# ---------------------------------------------------------------------------------------------------------------------------
def _raw_call(inp, fill=float("nan")):
    """both launches straight through the C ABI into buffers prefilled with `fill`"""
    from psvo_amd import _lib
    lib = _lib.load()
    x, Wf, bf, Wb, bb, dout = (t.float().cuda().contiguous() for t in inp)
    B, T, Din = x.shape
    Dh = Wf.shape[1] // 4
    new = lambda *s: torch.full(s, fill, device="cuda", dtype=torch.float32)
    out, cs, gates = new(B, T, 2 * Dh), new(2, B, T, Dh), new(2, B, T, 4 * Dh)
    dx_part, dW_part, db_part = new(2, B, T, Din), new(B, 2, Din + Dh, 4 * Dh), new(B, 2, 4 * Dh)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.psvo_bilstm_forward(B, T, Din, Dh, p(x), p(Wf), p(bf), p(Wb), p(bb), p(out), p(cs), p(gates), st),
               "psvo_bilstm_forward")
    _lib.check(lib.psvo_bilstm_backward(B, T, Din, Dh, p(x), p(Wf), p(Wb), p(out), p(cs), p(gates), p(dout), p(dx_part),
                                        p(dW_part), p(db_part), st), "psvo_bilstm_backward")
    torch.cuda.synchronize()
    return dict(out=out, cs=cs, gates=gates, dx_part=dx_part, dW_part=dW_part, db_part=db_part)


@pytest.mark.parametrize("Din,Dh", [(5, 16), (128, 32)], ids=["padded-Din5-Dh16", "scratch-Din128-Dh32"])
def test_every_output_element_is_written(built_lib, Din, Dh):
    inp, got, _, _ = run_case(3, 6, Din, Dh, seed=21)
    raw = _raw_call(inp)
    for k, v in raw.items():
        assert not torch.isnan(v).any(), "%s keeps %d prefilled elements" % (k, int(torch.isnan(v).sum()))
    dW, db = raw["dW_part"].sum(0), raw["db_part"].sum(0)
    mine = dict(out=raw["out"], cs=raw["cs"], gates=raw["gates"], dx=raw["dx_part"].sum(0), dW_fw=dW[0], db_fw=db[0],
                dW_bw=dW[1], db_bw=db[1])
    for k, v in mine.items():
        assert torch.equal(v.double().cpu(), got[k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the directions do not leak
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", ["fw", "bw"])
@pytest.mark.parametrize("Din,Dh", [(3, 16), (33, 32)], ids=["Din3-Dh16", "Din33-Dh32"])
def test_directions_do_not_leak(built_lib, keep, Din, Dh):
    from psvo_amd import ops
    inp = list(make_inputs(3, 6, Din, Dh, seed=31))
    dout = inp[5]
    (dout[..., Dh:] if keep == "fw" else dout[..., :Dh]).zero_()
    x, Wf, bf, Wb, bb, d = (t.cuda() for t in inp)
    out, cs, gates = ops.bilstm_forward(x, Wf, bf, Wb, bb, save=True)
    got = dict(zip(GRADS, (v.double().cpu() for v in ops.bilstm_backward(x, Wf, Wb, out, cs, gates, d))))
    dead = "bw" if keep == "fw" else "fw"
    assert float(got["dW_" + dead].abs().max()) == 0.0 and float(got["db_" + dead].abs().max()) == 0.0
    r64, r32 = oracle_layer(inp, torch.float64, keep), oracle_layer(inp, torch.float32, keep)
    assert r64["dW_" + dead] is None
    check_grads("6 directions do not leak", "keep %s Din=%d Dh=%d" % (keep, Din, Dh), got, r64, r32, Din, Dh,
                ("dx", "dW_" + keep, "db_" + keep))


# ---------------------------------------------------------------------------------------------------------------------------
# 7. psvo_bilstm_wgrad_fold
# ---------------------------------------------------------------------------------------------------------------------------
def _gamma(n):
    """Higham's gamma_n for fp32: a sum of n + 1 terms in ANY order is within gamma_n * sum|terms| of the exact sum"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def _fold(B, Din, Dh, dW_part, db_part, g_fw, g_bw, accumulate):
    from psvo_amd import _lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.load().psvo_bilstm_wgrad_fold(B, Din, Dh, p(dW_part), p(db_part), p(g_fw), p(g_bw), accumulate,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "psvo_bilstm_wgrad_fold")
    torch.cuda.synchronize()


@pytest.mark.parametrize("B", [1, 3, 600])
def test_wgrad_fold(built_lib, B):
    """The fold against the fp64 sum of the partials.  Bound: fp32 summation of B terms (plus the target under accumulate),
    whatever the order, is within gamma_{B} * sum|terms| of the exact sum (Higham, Accuracy and Stability, section 4.2)."""
    from psvo_amd import ops
    Din, Dh = 5, 16
    K, G4 = Din + Dh, 4 * Dh
    n = K * G4 + G4
    inp = make_inputs(B, 3, Din, Dh, seed=41)
    raw = _raw_call(inp)
    dW_part, db_part = raw["dW_part"], raw["db_part"]
    parts = torch.cat([dW_part.reshape(B, 2, K * G4), db_part], dim=2).double().cpu()       # (B, 2, n): [kernel | bias]
    ref, mass = parts.sum(0), parts.abs().sum(0)

    # accumulate = 0 overwrites whatever the targets held
    g = torch.full((2, n), float("nan"), device="cuda")
    _fold(B, Din, Dh, dW_part, db_part, g[0], g[1], 0)
    got = g.double().cpu()
    assert torch.isfinite(got).all()
    assert bool(((got - ref).abs() <= _gamma(B - 1) * mass).all()) if B > 1 else torch.equal(got, ref)
    _note("7 fold (err / summation bound)", float(((got - ref).abs() / (_gamma(max(B - 1, 1)) * mass)).max()), "B=%d" % B)
    g2 = torch.full((2, n), float("nan"), device="cuda")
    _fold(B, Din, Dh, dW_part, db_part, g2[0], g2[1], 0)
    assert torch.equal(g, g2), "two folds of the same partials differ"

    # accumulate = 1 adds onto what is there
    base = torch.randn(2, n, generator=torch.Generator().manual_seed(5))
    h = base.cuda()
    _fold(B, Din, Dh, dW_part, db_part, h[0], h[1], 1)
    assert bool(((h.double().cpu() - (ref + base.double())).abs() <= _gamma(B) * (mass + base.double().abs())).all())

    # the gbufs route of the wrapper (fold into flat-gradient slices) against its tensor route (torch sums of the partials)
    x, Wf, bf, Wb, bb, dout = (t.cuda() for t in inp)
    fwd = (x, Wf, Wb, raw["out"], raw["cs"], raw["gates"], dout)
    dx, dWf, dbf, dWb, dbb = ops.bilstm_backward(*fwd)
    gf, gb = base[0].cuda(), base[1].cuda()
    dx2, *none = ops.bilstm_backward(*fwd, gbufs=(gf, gb))
    assert all(v is None for v in none) and torch.equal(dx, dx2)
    tensor_route = torch.stack([torch.cat([dWf.reshape(-1), dbf]), torch.cat([dWb.reshape(-1), dbb])]).double().cpu()
    flat_route = torch.stack([gf, gb]).double().cpu() - base.double()
    # (each route is within its own summation bound of the exact sum; removing `base` again costs one more rounding)
    slack = (_gamma(B) + _gamma(max(B - 1, 1)) + 2.0 ** -24) * (mass + base.double().abs())
    assert bool(((flat_route - tensor_route).abs() <= slack).all())
    if B == 1:
        assert torch.equal(tensor_route, ref)

    # the reverse kernel has no atomics: a second launch on the same inputs gives the same bits
    again = _raw_call(inp)
    for k in raw:
        assert torch.equal(raw[k], again[k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the three wirings at the wide instantiations
# ---------------------------------------------------------------------------------------------------------------------------
# The widest instantiation each wiring reaches.  ("uni" chains Dh-wide outputs, so "64,32" runs its second cell in <64,32>; the
# forward-cells-only wiring meets <128,32> only with observations wider than 64, which is what the last case is.)
WIRING_INST = {("stack", 2, (64, 64)): (128, 64), ("multi", 2, (32, 64)): (64, 64), ("uni", 2, (64, 32)): (64, 32),
               ("uni", 100, (32,)): (128, 32)}
WIRING_IDS = ["%s-%s-Din%d" % (m, "x".join(map(str, d)), n) for m, d, n in Hh.ENCODER_WIRINGS]


@pytest.mark.parametrize("mode,Dhs,Din", Hh.ENCODER_WIRINGS, ids=WIRING_IDS)
def test_wirings_at_the_wide_instantiations(built_lib, mode, Dhs, Din):
    enc, x, dout = Hh.make_encoder(mode, Dhs, Din)
    # the instantiation of every launch: multi embeds layer i >= 1 into a kernel that reads concat(fw, bw)
    insts = [(_pad(c.Din * (2 if (mode == "multi" and i) else 1)), c.Dh) for i, c in enumerate(enc.fw)]
    assert WIRING_INST[(mode, Din, tuple(Dhs))] in insts, insts
    o64, g64 = Hh.oracle_encoder(mode, Hh.encoder_layers(enc, torch.float64), x.double(), dout)
    o32, g32 = Hh.oracle_encoder(mode, Hh.encoder_layers(enc, torch.float32), x.float(), dout)
    enc = enc.cuda()
    xg = x.cuda().requires_grad_(True)
    out = enc(xg)
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    check_forward("8 wirings, forward", mode, {"out": out.detach().double().cpu()}, {"out": o64}, names=("out",))
    got = {"x": xg.grad.double().cpu()}
    for n, p in enc.named_parameters():
        assert p.grad is not None, n
        got[n] = p.grad.double().cpu()
    assert set(got) == set(g64)
    bad = []
    for n in sorted(got):
        i = int(n.split(".")[1]) if n != "x" else 0
        cell = enc.fw[i]
        kind = "dW" if n.endswith("kernel") else ("db" if n.endswith("bias") else "dx")
        for label, idx in grad_blocks(kind, cell.Din, cell.Dh):
            ratio, fig = block_ratio(got[n][idx], g64[n][idx], g32[n][idx])
            _note("8 wirings", ratio, "%s %s %s" % (mode, n, label))
            if not ratio <= 1.0:
                bad.append((n, label, "ratio %.3g" % ratio, "err %.3g err32 %.3g scale %.3g" % fig))
    assert not bad, "%s: gradient blocks beyond K32 x max(fp32 oracle's error, 1e-6 scale): %s" % (mode, bad)
