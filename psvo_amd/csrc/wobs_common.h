// What the wide-observation ("wobs") units share: the run-time width bound, the terms of the count emission and the LDS image
// of MLP_g with its output layer transposed (filter_wobs.hip, bsim_wobs.hip).
#pragma once
#include "common.h"

namespace psvo {
namespace wobs {

constexpr int kMaxDy = 32;

// Count emission (psvo_desc.emission = 2): log Gamma(y + 1) of an observed count.  Called by the lanes that stage the next
// step's observation row, once per (step, sequence, output), never per particle.  Evaluated in fp64 and rounded once, so the
// result is the fp32 nearest to the true value for every integer y (exactly 0 for y in {0, 1}): y < 8 takes log(y!) of the
// exact product, y >= 8 the Stirling series at n = y + 1 with three correction terms (next term 1 / (1680 n^7) < 1.3e-10).
// No table, hence no index: whatever y holds (negative, fractional, not finite), nothing is addressed with it.
__device__ __forceinline__ float log_factorial(float y) {
    const double n = (double)y + 1.0;
    double p = 1.0;
#pragma unroll
    for (int k = 2; k < 8; ++k) p *= (y >= (float)k) ? (double)k : 1.0;
    const bool small = !(y >= 8.f);
    const double l = log(small ? p : n);
    const double i = 1.0 / n, i2 = i * i;
    const double series = i * (1.0 / 12.0 - i2 * (1.0 / 360.0 - i2 * (1.0 / 1260.0)));
    return (float)(small ? l : (n - 0.5) * l - n + 0.9189385332046727418 + series);
}

// one term of the count log-density, without the log-factorial: y log lam - lam, lam = emis_mean(r) (common.h)
__device__ __forceinline__ float count_term(float y, float r) {
    const float lam = emis_mean(r);
    return fmaf(y, logf(lam), -lam);
}

// d log g / d r = (y / lam - 1) sigmoid(r), written (y - lam) / lam: no cancellation where the rate fits the count.  Both
// quotients are hardware reciprocals (1 ulp): an IEEE division is a dozen instructions and a pair of lane masks each, which the
// reverse kernels have no scalar registers for
__device__ __forceinline__ float count_dterm(float y, float r) {
    const float lam = emis_mean(r);
    const float sig = __builtin_amdgcn_rcpf(1.f + expf(-r));     // emis_dmean
    return (y - lam) * __builtin_amdgcn_rcpf(lam) * sig;
}

// LDS image of MLP_g: W1[DX][H] | b1[H] | W2T[Dy][H] | b2[Dy]   (room for Dy = 32)
template <int DX, int H>
struct GLds {
    static constexpr int kW1 = 0;
    static constexpr int kB1 = DX * H;
    static constexpr int kW2 = kB1 + H;
    static constexpr int kB2 = kW2 + kMaxDy * H;
    static constexpr int kSize = kB2 + kMaxDy;

    __device__ static void load(float* __restrict__ w, const psvo_mlp& p, int Dy, int tid, int nthreads) {
        for (int i = tid; i < DX * H; i += nthreads) w[kW1 + i] = p.W1[i];
        for (int i = tid; i < H; i += nthreads) w[kB1 + i] = p.b1[i];
        for (int i = tid; i < Dy * H; i += nthreads) {
            const int o = i / H, k = i - o * H;
            w[kW2 + i] = p.W2[k * Dy + o];
        }
        for (int i = tid; i < Dy; i += nthreads) w[kB2 + i] = p.b2[i];
    }

    // h = relu(x W1 + b1)
    __device__ __forceinline__ static void hidden(const float* __restrict__ w, const float (&x)[DX], float (&h)[H]) {
#pragma unroll
        for (int k = 0; k < H; k += 4) {
            const float4 b = *reinterpret_cast<const float4*>(w + kB1 + k);
            float p0 = b.x, p1 = b.y, p2 = b.z, p3 = b.w;
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                const float4 wi = *reinterpret_cast<const float4*>(w + kW1 + d * H + k);
                p0 = fmaf(x[d], wi.x, p0); p1 = fmaf(x[d], wi.y, p1);
                p2 = fmaf(x[d], wi.z, p2); p3 = fmaf(x[d], wi.w, p3);
            }
            h[k] = fmaxf(p0, 0.f); h[k + 1] = fmaxf(p1, 0.f); h[k + 2] = fmaxf(p2, 0.f); h[k + 3] = fmaxf(p3, 0.f);
        }
    }

    // output e: h . W2T[e] + b2[e] (four partial sums, folded pairwise)
    __device__ __forceinline__ static float out(const float* __restrict__ w, int e, const float (&h)[H]) {
        const float* w2 = w + kW2 + e * H;
        float s0 = w[kB2 + e], s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int k = 0; k < H; k += 4) {
            const float4 wo = *reinterpret_cast<const float4*>(w2 + k);
            s0 = fmaf(h[k], wo.x, s0); s1 = fmaf(h[k + 1], wo.y, s1);
            s2 = fmaf(h[k + 2], wo.z, s2); s3 = fmaf(h[k + 3], wo.w, s3);
        }
        return (s0 + s1) + (s2 + s3);
    }

    // Input gradient of MLP_g from the rows dg[o] = row[o * stride] (the lane's own d G rows, already in HBM), hidden units
    // in chunks of HC so that a lane holds HC partial sums, not H:  dx += W1[:, chunk] ([pre > 0] * sum_o dg[o] W2T[o][chunk]).
    template <int HC>
    __device__ __forceinline__ static void bwd_input(const float* __restrict__ w, int Dy, const float* row, size_t stride,
                                                     bool valid, const float (&x)[DX], float (&dx)[DX]) {
        static_assert(H % HC == 0 && HC % 4 == 0, "hidden chunk");
#pragma unroll 1
        for (int kc = 0; kc < H; kc += HC) {
            float dh[HC];
#pragma unroll
            for (int k = 0; k < HC; ++k) dh[k] = 0.f;
#pragma unroll 1
            for (int o = 0; o < Dy; ++o) {
                const float dg = valid ? row[o * stride] : 0.f;
                const float* w2 = w + kW2 + o * H + kc;
#pragma unroll
                for (int k = 0; k < HC; k += 4) {
                    const float4 wo = *reinterpret_cast<const float4*>(w2 + k);
                    dh[k] = fmaf(dg, wo.x, dh[k]); dh[k + 1] = fmaf(dg, wo.y, dh[k + 1]);
                    dh[k + 2] = fmaf(dg, wo.z, dh[k + 2]); dh[k + 3] = fmaf(dg, wo.w, dh[k + 3]);
                }
            }
#pragma unroll
            for (int k = 0; k < HC; k += 4) {
                const float4 b = *reinterpret_cast<const float4*>(w + kB1 + kc + k);
                float p0 = b.x, p1 = b.y, p2 = b.z, p3 = b.w;
                float4 wi[DX];
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    wi[d] = *reinterpret_cast<const float4*>(w + kW1 + d * H + kc + k);
                    p0 = fmaf(x[d], wi[d].x, p0); p1 = fmaf(x[d], wi[d].y, p1);
                    p2 = fmaf(x[d], wi[d].z, p2); p3 = fmaf(x[d], wi[d].w, p3);
                }
                const float v0 = p0 > 0.f ? dh[k] : 0.f, v1 = p1 > 0.f ? dh[k + 1] : 0.f;
                const float v2 = p2 > 0.f ? dh[k + 2] : 0.f, v3 = p3 > 0.f ? dh[k + 3] : 0.f;
#pragma unroll
                for (int d = 0; d < DX; ++d)
                    dx[d] = fmaf(v3, wi[d].w, fmaf(v2, wi[d].z, fmaf(v1, wi[d].y, fmaf(v0, wi[d].x, dx[d]))));
            }
        }
    }
};

}  // namespace wobs
}  // namespace psvo
