// Pair-phase helpers shared by the marginal smoother (ffbs.hip), the backward sampler (ffbsi.hip) and the MAP decoder
// (map_path.hip): the staged LDS rows of a step, the max-shifted log-sum-exp over them (pair_lse) and the running maximum with
// its index (pair_argmax).  The kernels walk N x N pair terms
//     log2(e) l[j,k] = cst[k] - sum_d ((x[j,d] - m[k,d]) r[k,d])^2
// with the lane's own point in registers and the other index's rows broadcast from LDS.
#pragma once
#include "common.h"

namespace psvo {

// floats per staged row: float4 reads for Dx = 3 as for Dx = 4
constexpr int ffbs_dxp(int DX) { return DX == 3 ? 4 : DX; }

template <int DX>
__device__ __forceinline__ void lds_row_store(float* __restrict__ p, const float (&v)[DX]) {
    if constexpr (DX == 2) *reinterpret_cast<float2*>(p) = float2{v[0], v[1]};
    else *reinterpret_cast<float4*>(p) = float4{v[0], v[1], v[2], DX == 4 ? v[DX - 1] : 0.f};
}

// a staged row as packed pairs: (d0, d1) [, (d2, d3)]; Dx = 3 carries a zero in the last slot (own and scale zero there too)
template <int DX>
__device__ __forceinline__ void lds_row_load2(const float* __restrict__ p, f2 (&v)[(DX + 1) / 2]) {
    if constexpr (DX == 2) {
        const float2 q = *reinterpret_cast<const float2*>(p);
        v[0] = f2{q.x, q.y};
    } else {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = f2{q.x, q.y};
        v[1] = f2{q.z, q.w};
    }
}
template <int DX>
__device__ __forceinline__ void pack_row(const float (&x)[DX], f2 (&v)[(DX + 1) / 2]) {
    v[0] = f2{x[0], x[1]};
    if constexpr (DX == 3) v[1] = f2{x[2], 0.f};
    if constexpr (DX == 4) v[1] = f2{x[2], x[3]};
}

// four staged rows of a pair phase in registers
template <int DX, bool ROWSCALE>
struct Rows4 {
    static constexpr int NP = (DX + 1) / 2;
    float v[4];
    f2 p[4][NP], rr[4][NP];
    __device__ __forceinline__ void load(const float* __restrict__ sv, const float* __restrict__ sp,
                                         const float* __restrict__ sr, int i0) {
        const float4 a4 = *reinterpret_cast<const float4*>(sv + i0);
        v[0] = a4.x; v[1] = a4.y; v[2] = a4.z; v[3] = a4.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lds_row_load2<DX>(sp + (i0 + i) * ffbs_dxp(DX), p[i]);
            if constexpr (ROWSCALE) lds_row_load2<DX>(sr + (i0 + i) * ffbs_dxp(DX), rr[i]);
        }
    }
};

// log2 sum_i exp2(sv[i] - sum_d ((sp[i][d] - own[d]) rr[d])^2) over the n8 staged rows (n8 a multiple of 8; padding rows carry
// sv = -inf), rr = the row's own scale factors sr[i][.] (ROWSCALE) or the lane's r[.].  Rows are read at wave-uniform addresses
// (LDS broadcasts), four at a time and one group AHEAD of the arithmetic: with one or two waves per SIMD nothing else hides
// the LDS latency (measured: without the read-ahead the loop ran at the sum of latency and arithmetic per group).  The squares
// run on packed f32 pairs (two dimensions per instruction); the max-shifted sum is kept online, rescaled once per four rows,
// in TWO accumulators (even and odd groups of four) that are merged at the end -- a fixed order.  -inf when every term is.
template <int DX, bool ROWSCALE>
__device__ __forceinline__ float pair_lse(const float* __restrict__ sv, const float* __restrict__ sp,
                                          const float* __restrict__ sr, const f2 (&own)[(DX + 1) / 2],
                                          const f2 (&r)[(DX + 1) / 2], int n8) {
    constexpr int NP = (DX + 1) / 2;
    const float ninf = -__builtin_huge_valf();
    float m[2] = {ninf, ninf}, s[2] = {0.f, 0.f};
    auto fold = [&](const Rows4<DX, ROWSCALE>& R, int h) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f2 acc = f2{0.f, 0.f};
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const f2 z = (R.p[i][q] - own[q]) * (ROWSCALE ? R.rr[i][q] : r[q]);
                acc = pk_fma(z, z, acc);
            }
            v[i] = R.v[i] - (acc.x + acc.y);
        }
        const float mn = fmaxf(fmaxf(m[h], fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
        const float mb = (mn == ninf) ? 0.f : mn;
        s[h] = fmaf(s[h], exp2_fast(m[h] - mb),
                    (exp2_fast(v[0] - mb) + exp2_fast(v[1] - mb)) + (exp2_fast(v[2] - mb) + exp2_fast(v[3] - mb)));
        m[h] = mn;
    };
    Rows4<DX, ROWSCALE> even, odd;
    even.load(sv, sp, sr, 0);
    for (int i0 = 0; i0 < n8; i0 += 8) {
        odd.load(sv, sp, sr, i0 + 4);
        fold(even, 0);
        even.load(sv, sp, sr, i0 + 8 < n8 ? i0 + 8 : 0);      // (the last read-ahead wraps to group 0 and is not used)
        fold(odd, 1);
    }
    const float mn = fmaxf(m[0], m[1]);
    const float mb = (mn == ninf) ? 0.f : mn;
    return mn + log2_fast(fmaf(s[0], exp2_fast(m[0] - mb), s[1] * exp2_fast(m[1] - mb)));
}

// max_i (sv[i] - sum_d ((sp[i][d] - own[d]) r[d])^2) over the n8 staged rows and the LOWEST i that attains it (map_path.hip):
// pair_lse's walk -- the same read-ahead, the same packed squares, the same two accumulators over even and odd groups of four --
// with a running (max, argmax) in place of the online sum, so no exponential.  An accumulator moves on strict `>` only and
// sees its rows in rising order: it holds the lowest index of its own maximum.  The merge takes the odd accumulator where it is
// larger, or equal with the lower index.  Both start at (-inf, 0): padding rows (sv = -inf) never win, and whatever the rows
// hold -- NaN included, every comparison with it is false -- the index returned is one the loop counted, 0 <= arg < n8, or 0.
template <int DX>
__device__ __forceinline__ void pair_argmax(const float* __restrict__ sv, const float* __restrict__ sp,
                                            const f2 (&own)[(DX + 1) / 2], const f2 (&r)[(DX + 1) / 2], int n8,
                                            float& best, int& arg) {
    constexpr int NP = (DX + 1) / 2;
    const float ninf = -__builtin_huge_valf();
    float m[2] = {ninf, ninf};
    int am[2] = {0, 0};
    auto fold = [&](const Rows4<DX, false>& R, int h, int i0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f2 acc = f2{0.f, 0.f};
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const f2 z = (R.p[i][q] - own[q]) * r[q];
                acc = pk_fma(z, z, acc);
            }
            const float v = R.v[i] - (acc.x + acc.y);
            const bool up = v > m[h];
            m[h] = up ? v : m[h];
            am[h] = up ? i0 + i : am[h];
        }
    };
    Rows4<DX, false> even, odd;
    even.load(sv, sp, nullptr, 0);
    for (int i0 = 0; i0 < n8; i0 += 8) {
        odd.load(sv, sp, nullptr, i0 + 4);
        fold(even, 0, i0);
        even.load(sv, sp, nullptr, i0 + 8 < n8 ? i0 + 8 : 0);      // (the last read-ahead wraps to group 0 and is not used)
        fold(odd, 1, i0 + 4);
    }
    const bool take = m[1] > m[0] || (m[1] == m[0] && am[1] < am[0]);
    best = take ? m[1] : m[0];
    arg = take ? am[1] : am[0];
}

}  // namespace psvo
