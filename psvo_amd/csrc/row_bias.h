// A one-hidden-layer MLP evaluated with a first-layer bias row of its own: the bias of the step, b1 + (the exogenous input's share
// of the hidden pre-activation), which the input-driven kernels keep in LDS (filter_wobs_in.hip, filter_wobs_inad.hip: the filter
// pairs; forecast.hip: the input form of the particle forecast).
#pragma once
#include "common.h"

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

}  // namespace wobs
}  // namespace psvo
