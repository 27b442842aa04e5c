"""The two entry points that are the single home of shared reductions, called directly on buffers written by torch:
psvo_bsim_backward_fold (the fold / finalize launch behind every backward-simulation reverse kernel, the wide ones included)
and psvo_reduce_rows (the fold of every weight gradient).  No reverse kernel runs here.

Bounds -- none is tuned to what the kernels return:
  dFm, dlogW           bit-equal to the float32 sum in part order computed on the host (v = 0; for k: v = float32(v + p[k])),
                       and bit-equal between 16-byte aligned buffers and views that start one float into an allocation
  dlse                 |err| <= 64 * 2^-24 * sum|terms| against fp64: the n-term fp32 summation bound, n = nblk * N <= 36
  scale gradients      against the fp64 evaluation of the product-of-Gaussians step, per tensor
                       err <= max(2e-3 * max|ref| + 1e-6, K32 * err32), err32 the error of the same evaluation in fp32
                       (the rule of tests/test_gpu_wobs.py::test_every_gradient); bit-equal between the two alignments
  psvo_reduce_rows     |err| <= nrows * 2^-24 * sum|x| against fp64 (accumulate = 1: bit-equal to float32(out + that sum)); two
                       calls bit-identical; with stride == n bit-equal to the
                       gradient psvo_mlp_wgrad folds from the same partials (it is the same kernel)
Measured on an MI355X (`pytest -s` prints them again): dlse at most 0.008 of its bound; scale gradients 4e-8 .. 7e-7 absolute at
scales 0.1 .. 5.5, the fp32 evaluation's own error 4e-8 .. 2e-7 (the first clause holds everywhere); psvo_reduce_rows at most
0.007 of its bound.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_instantiations import K32

pytestmark = pytest.mark.gpu

T, B, M, H, DY = 3, 2, 32, 16, 2
U = 2.0 ** -24


def _fold(lib, ops, desc, dFm_part, dlogW_part, sacc, sig1, sig2):
    Dx, N = desc.Dx, desc.N
    dev = sacc.device
    out = {"dFm": torch.full((T, B, Dx, N), float("nan"), device=dev), "dlogW": torch.full((T, B, N), float("nan"), device=dev),
           "dlse": torch.full((T, B), float("nan"), device=dev)}
    for k in ("dsig_f", "dsig_q1inv", "dsig_bq2", "dsig_init", "disig"):
        out[k] = torch.full((Dx,), float("nan"), device=dev)
    out["dsig_g"] = torch.full((DY,), float("nan"), device=dev)
    p = ops._ptr
    st = lib.psvo_bsim_backward_fold(ctypes.byref(desc), p(dFm_part), p(dlogW_part), p(sacc), p(sig1), p(sig2), p(out["dFm"]),
                                     p(out["dlogW"]), p(out["dsig_f"]), p(out["dsig_g"]), p(out["dsig_q1inv"]),
                                     p(out["dsig_bq2"]), p(out["dsig_init"]), p(out["disig"]), p(out["dlse"]), ops._stream())
    assert st == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ordered_sum32(parts, axis):
    """float32 sum over `axis` in index order"""
    parts = np.moveaxis(parts, axis, 0)
    v = np.zeros(parts.shape[1:], np.float32)
    for k in range(parts.shape[0]):
        v = (v + parts[k]).astype(np.float32)
    return v


def _scale_grads(tot, s1, s2, Dx, dt):
    """the finalize step on the (7 Dx + Dy) totals in precision dt: slots [Sc | Smm1 | Smb | Smm | Sf | Sinit | Siota | Sg]"""
    tot, s1, s2 = tot.astype(dt), s1.astype(dt), s2.astype(dt)
    one = dt(1)
    Sc, Smm1, Smb, Smm = (tot[i * Dx:(i + 1) * Dx] for i in range(4))
    i1, i2 = one / s1, one / s2
    c = one / (i1 + i2)
    dc = Sc + Smm / c
    di1 = c * Smm1 - c * c * dc
    di2 = c * Smb - c * c * dc
    return {"dsig_q1inv": -i1 * i1 * di1, "dsig_bq2": -i2 * i2 * di2, "dsig_f": tot[4 * Dx:5 * Dx],
            "dsig_init": tot[5 * Dx:6 * Dx], "disig": tot[6 * Dx:7 * Dx], "dsig_g": tot[7 * Dx:]}


@pytest.mark.parametrize("Dx,N", [(2, 12), (3, 10), (4, 12)])
def test_bsim_backward_fold(built_lib, Dx, N):
    from psvo_amd import _lib, ops
    lib = _lib.load()
    desc = ops.make_desc(B, T, N, M, Dx, DY, H)
    nblk = lib.psvo_bsim_blocks(ctypes.byref(desc))
    assert nblk >= 2, "precondition: more than one workgroup per sequence (nblk = %d)" % nblk
    nacc = lib.psvo_bsim_acc_size(Dx, DY)
    assert nacc == 7 * Dx + DY
    g = torch.Generator().manual_seed(100 * Dx + N)
    hF = torch.randn(T, B, nblk, Dx, N, generator=g)
    hW = torch.randn(T, B, nblk, N, generator=g)
    hS = torch.randn(B, nblk, nacc, generator=g)
    s1 = torch.rand(Dx, generator=g) + 0.5
    s2 = torch.rand(Dx, generator=g) + 0.5
    dev = "cuda"
    runs = [_fold(lib, ops, desc, hF.to(dev), hW.to(dev), hS.to(dev), s1.to(dev), s2.to(dev))]
    if (Dx, N) == (2, 12):      # the same partials one float into a larger allocation: not 16-byte aligned
        bF = torch.zeros(hF.numel() + 8, device=dev)
        bW = torch.zeros(hW.numel() + 8, device=dev)
        vF, vW = bF[1:1 + hF.numel()].view(hF.shape), bW[1:1 + hW.numel()].view(hW.shape)
        vF.copy_(hF)
        vW.copy_(hW)
        assert vF.data_ptr() % 16 == 4 and vW.data_ptr() % 16 == 4
        runs.append(_fold(lib, ops, desc, vF, vW, hS.to(dev), s1.to(dev), s2.to(dev)))
        for k in runs[0]:
            assert np.array_equal(runs[0][k].view(np.uint32), runs[1][k].view(np.uint32)), "%s differs with the alignment" % k

    F, W, S = hF.numpy(), hW.numpy(), hS.numpy()
    terms = W.astype(np.float64).reshape(T, B, nblk * N)
    tot64 = S.astype(np.float64).reshape(B * nblk, nacc).sum(0)
    ref = _scale_grads(tot64, s1.numpy(), s2.numpy(), Dx, np.float64)
    tot32 = _ordered_sum32(S.reshape(B * nblk, nacc), 0)
    ref32 = _scale_grads(tot32, s1.numpy(), s2.numpy(), Dx, np.float32)
    for out in runs:
        assert np.array_equal(out["dFm"].view(np.uint32), _ordered_sum32(F, 2).view(np.uint32))
        assert np.array_equal(out["dlogW"].view(np.uint32), _ordered_sum32(W, 2).view(np.uint32))
        err = np.abs(out["dlse"].astype(np.float64) + terms.sum(-1))
        bound = 64 * U * np.abs(terms).sum(-1)
        print("dlse: worst err / bound %.3f" % float((err / bound).max()))
        assert (err <= bound).all()
        for k, r in ref.items():
            e = float(np.abs(out[k].astype(np.float64) - r).max())
            e32 = float(np.abs(ref32[k].astype(np.float64) - r).max())
            scale = max(float(np.abs(r).max()), 1e-6)
            print("%s: err %.3e  scale %.3e  fp32 evaluation's own err %.3e" % (k, e, scale, e32))
            assert e <= max(2e-3 * scale + 1e-6, K32 * e32), k


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nrows", [1, 64, 65, 130])
def test_reduce_rows(built_lib, nrows, accumulate):
    from psvo_amd import ops
    n, stride = 5, 7
    g = torch.Generator().manual_seed(nrows)
    part = torch.randn(nrows, stride, generator=g)
    base = torch.randn(n, generator=g)

    def run(acc):
        out = base.clone().cuda()
        ops.reduce_rows(part.cuda(), nrows, stride, n, out, accumulate=acc)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    outs = [run(bool(accumulate)), run(bool(accumulate))]
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    plain = outs[0] if not accumulate else run(False)
    x = part[:, :n].double().numpy()
    err = np.abs(plain.astype(np.float64) - x.sum(0))
    bound = nrows * U * np.abs(x).sum(0)
    print("nrows=%d: worst err / bound %.3f" % (nrows, float((err / bound).max())))
    assert (err <= bound).all()
    if accumulate:      # out + sum, one float32 addition: the sum is the one checked above, bit for bit
        assert np.array_equal(outs[0].view(np.uint32), (base.numpy() + plain).astype(np.float32).view(np.uint32))


def test_reduce_rows_is_the_weight_gradient_fold(built_lib):
    """psvo_mlp_wgrad on caller-owned partials, then psvo_reduce_rows over the same partials with stride == n: bit-equal"""
    from psvo_amd import _lib, ops
    lib = _lib.load()
    Din, Hh, Dout, S, L = 2, 16, 2, 6, 700
    g = torch.Generator().manual_seed(7)
    X = torch.randn(S, Din, L, generator=g).cuda()
    dOut = torch.randn(S, Dout, L, generator=g).cuda()
    w = [torch.randn(*s, generator=g).cuda() for s in ((Din, Hh), (Hh,), (Hh, Dout), (Dout,))]
    ws = ops._mlp_struct(w, Din, Hh, Dout, "w")
    NP = ops.mlp_grad_size(Din, Hh, Dout)
    nblk = lib.psvo_mlp_wgrad_blocks(S * L)
    assert nblk >= 2, "precondition: more than one partial to fold (nblk = %d)" % nblk
    partial = torch.zeros(nblk, NP, device="cuda")
    grad = torch.zeros(NP, device="cuda")
    p = ops._ptr
    st = lib.psvo_mlp_wgrad(S, L, Din, Hh, Dout, p(X), p(dOut), ctypes.byref(ws), p(partial), p(grad), 0, ops._stream())
    assert st == 0
    out = torch.zeros(NP, device="cuda")
    ops.reduce_rows(partial, nblk, NP, NP, out)
    torch.cuda.synchronize()
    assert float(grad.abs().max()) > 0
    assert torch.equal(grad.view(torch.int32), out.view(torch.int32))
