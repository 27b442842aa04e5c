// Exogenous inputs for the filter objectives: the wide-observation filter pair in its missing-observation form (every
// 1 <= Dy <= 32, the three emission forms, NaN = not observed) with input-driven transitions,
//     x_{t+1} ~ f(. | x_t, v_t),   proposal q1(. | x_t, v_t),
//     MLP(x_t[n]; v_t) = relu(x_t[n] W1[:Dx] + (b1 + v_t W1[Dx:])) W2 + b2
// (include/psvo_hip.h: psvo_filter_forward_wobs_input, psvo_filter_backward_wobs_input).  The input's share of the hidden
// pre-activation, hb[t,b,:] = v[b,t,:] W1[Dx:], does not depend on the particle: the host computes it with plain matrix products
// (T,B,H per network, zero beyond the model's hidden width) and the kernels need only a first-layer bias that changes every
// step.  This unit is filter_wobs_impl.h compiled a fifth time, PSVO_IN = 1 on top of PSVO_MS = 1 (PSVO_AD = 0): 18 forward and
// 18 reverse kernels (no EXT form: nothing runs behind this filter under autograd).  What differs sits under `#if PSVO_IN` there.
// The gradient of hb is not the kernels' business: the reverse kernel leaves the rows d P / d F as always, and
// psvo_mlp_wgrad_rowbias (mlp_wgrad_rowbias.hip) turns them into the weight gradients and the per-(step, sequence) sums d hb.
#include "filter_wobs_args.h"

namespace psvo {
namespace wobs {

// MlpLds<DX, H, DX, 1>::eval<true> / bwd_input<true> with the first-layer bias read from a row of its own (`hb`: H floats in
// LDS, 16-byte aligned, wave-uniform) where those read the image's b1.  The same operations in the same order on the same
// image, so that a zero input share reproduces the missing-observation kernels bit for bit; kept here, beside their only
// users, so that no unit that instantiates MlpLds sees a changed member.
template <int DX, int H>
struct RowBias {
    using M = MlpLds<DX, H, DX, 1>;
    static_assert(H % 8 == 0 && H > 8, "the rolled forms walk groups of eight hidden units");

    __device__ __forceinline__ static void group4(const float* __restrict__ w, const float* __restrict__ hb, int k,
                                                  const float (&x)[DX], f2 (&acc)[DX]) {
        const float4 b = *reinterpret_cast<const float4*>(hb + k);
        f2 ha = f2{b.x, b.y}, hc = f2{b.z, b.w};
#pragma unroll
        for (int i = 0; i < DX; ++i) {
            const float4 wi = *reinterpret_cast<const float4*>(w + M::kW1 + i * H + k);
            const f2 xi = f2{x[i], x[i]};
            ha = pk_fma(xi, f2{wi.x, wi.y}, ha);
            hc = pk_fma(xi, f2{wi.z, wi.w}, hc);
        }
        const f2 zero = f2{0.f, 0.f};
        ha = pk_max(ha, zero);
        hc = pk_max(hc, zero);
#pragma unroll
        for (int o = 0; o < DX; ++o) {
            const float4 wo = *reinterpret_cast<const float4*>(w + M::kW2 + o * H + k);
            acc[o] = pk_fma(ha, f2{wo.x, wo.y}, acc[o]);
            acc[o] = pk_fma(hc, f2{wo.z, wo.w}, acc[o]);
        }
    }

    // out = relu(x W1 + hb) W2 + b2
    __device__ __forceinline__ static void eval(const float* __restrict__ w, const float* __restrict__ hb, const float (&x)[DX],
                                                float (&out)[DX]) {
        f2 acc[DX];
#pragma unroll
        for (int o = 0; o < DX; ++o) acc[o] = f2{w[M::kB2 + o], 0.f};
#pragma unroll 1
        for (int k = 0; k < H; k += 8) {
            group4(w, hb, k, x, acc);
            group4(w, hb, k + 4, x, acc);
        }
#pragma unroll
        for (int o = 0; o < DX; ++o) out[o] = acc[o].x + acc[o].y;
    }

    __device__ __forceinline__ static void bwd_group4(const float* __restrict__ w, const float* __restrict__ hb, int k,
                                                      const float (&x)[DX], const float (&dout)[DX], f2 (&dxa)[DX]) {
        const float4 b = *reinterpret_cast<const float4*>(hb + k);
        f2 pa = f2{b.x, b.y}, pb = f2{b.z, b.w};
        f2 wa[DX], wb[DX];
#pragma unroll
        for (int i = 0; i < DX; ++i) {
            const float4 wi = *reinterpret_cast<const float4*>(w + M::kW1 + i * H + k);
            wa[i] = f2{wi.x, wi.y};
            wb[i] = f2{wi.z, wi.w};
            const f2 xi = f2{x[i], x[i]};
            pa = pk_fma(xi, wa[i], pa);
            pb = pk_fma(xi, wb[i], pb);
        }
        f2 da = f2{0.f, 0.f}, db = da;
#pragma unroll
        for (int o = 0; o < DX; ++o) {
            const float4 wo = *reinterpret_cast<const float4*>(w + M::kW2 + o * H + k);
            const f2 go = f2{dout[o], dout[o]};
            da = pk_fma(go, f2{wo.x, wo.y}, da);
            db = pk_fma(go, f2{wo.z, wo.w}, db);
        }
        da = f2{pa.x > 0.f ? da.x : 0.f, pa.y > 0.f ? da.y : 0.f};
        db = f2{pb.x > 0.f ? db.x : 0.f, pb.y > 0.f ? db.y : 0.f};
#pragma unroll
        for (int i = 0; i < DX; ++i) {
            dxa[i] = pk_fma(da, wa[i], dxa[i]);
            dxa[i] = pk_fma(db, wb[i], dxa[i]);
        }
    }

    // dx += (d out / d x)^T dout, the relu mask taken from x W1 + hb
    __device__ __forceinline__ static void bwd_input(const float* __restrict__ w, const float* __restrict__ hb,
                                                     const float (&x)[DX], const float (&dout)[DX], float (&dx)[DX]) {
        f2 dxa[DX];
#pragma unroll
        for (int i = 0; i < DX; ++i) dxa[i] = f2{dx[i], 0.f};
#pragma unroll 1
        for (int k = 0; k < H; k += 8) {
            bwd_group4(w, hb, k, x, dout, dxa);
            bwd_group4(w, hb, k + 4, x, dout, dxa);
        }
#pragma unroll
        for (int i = 0; i < DX; ++i) dx[i] = dxa[i].x + dxa[i].y;
    }
};

#define PSVO_AD 0
#define PSVO_MS 1
#define PSVO_IN 1
#include "filter_wobs_impl.h"
#undef PSVO_IN
#undef PSVO_MS
#undef PSVO_AD

// (the LDS of the missing-observation form with both rows of the count form, plus hbuf[2][2 H])
template <int DX, int H>
static int launch_fwd_in(const FwdArgsIn& a, hipStream_t stream) {
    const int NT = (a.N + 63) & ~63;
    const size_t lds = fwd_lds_bytes<DX, H>(NT, true) + sizeof(float) * 4 * H;
    clear_hip_error();
    if (a.emission == 2) hipLaunchKernelGGL((filter_fwd_wobs_in_kernel<DX, H, true>), dim3(a.B), dim3(NT), lds, stream, a);
    else hipLaunchKernelGGL((filter_fwd_wobs_in_kernel<DX, H, false>), dim3(a.B), dim3(NT), lds, stream, a);
    return launch_status();
}

template <int DX, int H>
static int launch_bwd_in(const BwdArgsIn& a, const BwdOut& o, hipStream_t stream) {
    const int NT = (a.N + 63) & ~63;
    const size_t lds = bwd_lds_bytes<DX, H>(NT, a.Dy, a.bootstrap != 0) + sizeof(float) * 4 * H;
    clear_hip_error();
    if (a.emission == 2) hipLaunchKernelGGL((filter_bwd_wobs_in_kernel<DX, H, false, true>), dim3(a.B), dim3(NT), lds, stream, a);
    else hipLaunchKernelGGL((filter_bwd_wobs_in_kernel<DX, H, false, false>), dim3(a.B), dim3(NT), lds, stream, a);
    if (a.two_q) {
        launch_row_sum(a.dm2_rows, (long long)a.T * a.B * DX, a.N, a.dmu2, stream);
    }
    (void)launch_filter_bwd_finalize(DX, {a.sacc, a.B, a.Dy, a.two_q, a.bootstrap, a.sig_q1, a.sig_q2, a.sig0, (int)(a.fsig0 == a.sig0),
                                          o.dsig_q1, o.dsig_q2, o.dsig_f, o.dsig_g, o.dsig0, o.dfsig0}, stream);
    return launch_status();
}

}  // namespace wobs
}  // namespace psvo

extern "C" int psvo_filter_forward_wobs_input(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                              const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                                              const float* mu2, const float* m0, const float* sig0, const float* fm0,
                                              const float* fsig0, const float* obs, const float* eps, const float* u,
                                              const int32_t* idx_in, float* X, float* Xanc, float* Fm, float* P1, float* logW,
                                              int32_t* idx_out, float* lse, const float* hb_q1, const float* hb_f, void* stream) {
    using namespace psvo;
    using namespace psvo::wobs;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!desc || !q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X || !Xanc || !Fm ||
        !logW || !idx_out || !lse || !hb_q1)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T < 2 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f || !hb_f)) return PSVO_ERR_INVALID;
    if (desc->resample && !u && !idx_in) return PSVO_ERR_INVALID;
    if (!filter_shape_ok(desc, 1)) return PSVO_ERR_UNSUPPORTED;

    FwdArgsIn a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy;
    a.resample = desc->resample; a.two_q = desc->two_q; a.bootstrap = desc->bootstrap; a.emission = desc->emission;
    a.q1 = *q1; a.f = desc->bootstrap ? *q1 : *f; a.g = *g;
    a.sig_q1 = sig_q1; a.sig_q2 = sig_q2; a.sig_f = sig_f; a.sig_g = sig_g;
    a.mu2 = mu2; a.m0 = m0; a.sig0 = sig0; a.fm0 = fm0; a.fsig0 = fsig0;
    a.obs = obs; a.eps = eps; a.u = u; a.idx_in = idx_in;
    a.X = X; a.Xanc = Xanc; a.Fm = Fm; a.P1 = P1; a.logW = logW; a.idx_out = idx_out; a.lse = lse;
    a.hb_q1 = hb_q1; a.hb_f = desc->bootstrap ? hb_q1 : hb_f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_fwd_in<dx(), h()>(a, s); });
}

extern "C" int psvo_filter_backward_wobs_input(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, float* dP, float* dF,
    float* dG, float* dmu2, float* dm0, float* dfm0, float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g,
    float* dsig0, float* dfsig0, float* ws, const float* hb_q1, const float* hb_f, void* stream) {
    using namespace psvo;
    using namespace psvo::wobs;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!desc || !q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X || !Fm || !logW ||
        !lse || !dP || !dG || !dm0 || !dfm0 || !dsig_q1 || !dsig_q2 || !dsig_f || !dsig_g || !dsig0 || !dfsig0 || !ws || !hb_q1)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T < 2 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2 || !dmu2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f || !P1 || !dF || !hb_f)) return PSVO_ERR_INVALID;
    if (desc->resample && !idx) return PSVO_ERR_INVALID;
    if (!filter_shape_ok(desc, 1)) return PSVO_ERR_UNSUPPORTED;

    BwdArgsIn a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy;
    a.resample = desc->resample; a.two_q = desc->two_q; a.bootstrap = desc->bootstrap; a.emission = desc->emission;
    a.q1 = *q1; a.f = desc->bootstrap ? *q1 : *f; a.g = *g;
    a.sig_q1 = sig_q1; a.sig_q2 = sig_q2; a.sig_f = sig_f; a.sig_g = sig_g;
    a.mu2 = mu2; a.m0 = m0; a.sig0 = sig0; a.fm0 = fm0; a.fsig0 = fsig0; a.obs = obs; a.eps = eps;
    a.X = X; a.Fm = Fm; a.P1 = P1; a.logW = logW; a.lse = lse; a.idx = idx; a.dlse = dlse;
    a.nparts = 0; a.dFm_ext = nullptr; a.dlogW_ext = nullptr;
    a.dP = dP; a.dF = dF; a.dG = dG; a.dmu2 = dmu2; a.dm0 = dm0; a.dfm0 = dfm0;
    a.sacc = ws;
    a.dm2_rows = ws + (long long)desc->B * (10 * desc->Dx + desc->Dy);
    a.hb_q1 = hb_q1; a.hb_f = desc->bootstrap ? hb_q1 : hb_f;
    BwdOut o{dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_bwd_in<dx(), h()>(a, o, s); });
}
