// Weight gradient of a one-hidden-layer MLP whose first-layer bias changes from segment to segment (exogenous inputs:
// include/psvo_hip.h, psvo_mlp_wgrad_rowbias).  The contract of psvo_mlp_wgrad (mlp_grad.hip) -- rows X [S][Din][L],
// dOut [S][Dout][L], Din, Dout <= 4 -- plus hb (S,H): the hidden layer of segment s is recomputed with b1 + hb[s] (one fp32 add
// per word, as the filter kernels make it), and beside grad = [dW1 | db1 | dW2 | db2] (db1 = sum over all rows of d pre) the
// kernel writes d hb (S,H) = sum_l d pre[s,l,:].
//
// A WAVE owns a segment (for the filter L = N <= 512: at most eight rows per lane) and a block column of KC hidden units, as
// mlp_wgrad_cols_kernel has them.  Orders, all fixed: a lane adds its rows l = lane, lane + 64, ... in that order; a segment's
// sum folds the 64 lanes in lane order (wave_sum); the accumulators of grad fold likewise, then the four waves of the
// workgroup in wave order, then the workgroups in workgroup order (reduce_rows).  No atomics; two calls on the same inputs
// give the same bits.  Every (segment, unit) of d hb has exactly one writer, so d hb needs no initial value.
#include "common.h"

namespace psvo {

struct WgradRowBiasArgs {
    long long S;     // segments
    int L;           // rows per segment
    const float* X;     // [S][DIN][L]
    const float* dOut;  // [S][DOUT][L]
    const float* hb;    // [S][H]
    psvo_mlp w;
    float* partial;  // [gridDim.x][NP]
    float* dhb;      // [S][H]
};

template <int DIN, int DOUT>
__global__ void __launch_bounds__(256) mlp_wgrad_rowbias_kernel(const WgradRowBiasArgs a, const int H) {
    constexpr int KC = (DIN + DOUT <= 4) ? 16 : 8;
    constexpr int NPC = (DIN + 1 + DOUT) * KC + DOUT;  // per-column partial sums (+ db2, kept from column 0)
    __shared__ float red[4][NPC];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k0 = blockIdx.y * KC;

    float w1[DIN][KC], b1[KC], w2[DOUT][KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        b1[k] = a.w.b1[k0 + k];
#pragma unroll
        for (int i = 0; i < DIN; ++i) w1[i][k] = a.w.W1[i * H + k0 + k];
#pragma unroll
        for (int o = 0; o < DOUT; ++o) w2[o][k] = a.w.W2[(k0 + k) * DOUT + o];
    }

    float gW1[DIN][KC], gb1[KC], gW2[DOUT][KC], gb2[DOUT];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        gb1[k] = 0.f;
#pragma unroll
        for (int i = 0; i < DIN; ++i) gW1[i][k] = 0.f;
#pragma unroll
        for (int o = 0; o < DOUT; ++o) gW2[o][k] = 0.f;
    }
#pragma unroll
    for (int o = 0; o < DOUT; ++o) gb2[o] = 0.f;

    const int L = a.L;
    for (long long s = (long long)blockIdx.x * 4 + wave; s < a.S; s += (long long)gridDim.x * 4) {
        float eb[KC], seg[KC];          // the segment's effective bias; its sum of d pre
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            eb[k] = b1[k] + a.hb[s * H + k0 + k];
            seg[k] = 0.f;
        }
        const float* Xs = a.X + s * DIN * L;
        const float* Ds = a.dOut + s * DOUT * L;
        for (int l = lane; l < L; l += 64) {
            float x[DIN], dout[DOUT];
#pragma unroll
            for (int i = 0; i < DIN; ++i) x[i] = Xs[(size_t)i * L + l];
#pragma unroll
            for (int o = 0; o < DOUT; ++o) {
                dout[o] = Ds[(size_t)o * L + l];
                gb2[o] += dout[o];
            }
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                float pre = eb[k];
#pragma unroll
                for (int i = 0; i < DIN; ++i) pre = fmaf(x[i], w1[i][k], pre);
                const float h = fmaxf(pre, 0.f);
                float dh = 0.f;
#pragma unroll
                for (int o = 0; o < DOUT; ++o) {
                    dh = fmaf(dout[o], w2[o][k], dh);
                    gW2[o][k] = fmaf(h, dout[o], gW2[o][k]);
                }
                dh = pre > 0.f ? dh : 0.f;
                gb1[k] += dh;
                seg[k] += dh;
#pragma unroll
                for (int i = 0; i < DIN; ++i) gW1[i][k] = fmaf(x[i], dh, gW1[i][k]);
            }
        }
        // (the wave is whole here: s and the trip count of the row loop's guard are wave-uniform only up to `l < L`, and the
        //  lanes that ran fewer rows have rejoined)
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const float v = wave_sum(seg[k]);
            if (lane == 0) a.dhb[s * H + k0 + k] = v;
        }
    }

    // block reduction: lanes in lane order, then the four waves in wave order
    auto put = [&](int p, float v) {
        v = wave_sum(v);
        if (lane == 0) red[wave][p] = v;
    };
#pragma unroll
    for (int k = 0; k < KC; ++k) {
#pragma unroll
        for (int i = 0; i < DIN; ++i) put(i * KC + k, gW1[i][k]);
        put(DIN * KC + k, gb1[k]);
#pragma unroll
        for (int o = 0; o < DOUT; ++o) put((DIN + 1 + o) * KC + k, gW2[o][k]);
    }
#pragma unroll
    for (int o = 0; o < DOUT; ++o) put((DIN + 1 + DOUT) * KC + o, gb2[o]);
    __syncthreads();
    // scatter the column into the flat keras-layout vector dW1 (DIN,H) | db1 (H) | dW2 (H,DOUT) | db2 (DOUT)
    const int NP = DIN * H + H + H * DOUT + DOUT;
    float* dst = a.partial + (size_t)blockIdx.x * NP;
    for (int p = tid; p < NPC; p += 256) {
        const float v = ((red[0][p] + red[1][p]) + red[2][p]) + red[3][p];
        if (p < (DIN + 1 + DOUT) * KC) {
            const int row = p / KC, k = p - row * KC;
            if (row < DIN) dst[row * H + k0 + k] = v;
            else if (row == DIN) dst[DIN * H + k0 + k] = v;
            else dst[DIN * H + H + (k0 + k) * DOUT + (row - DIN - 1)] = v;
        } else if (blockIdx.y == 0) {
            dst[DIN * H + H + H * DOUT + (p - (DIN + 1 + DOUT) * KC)] = v;
        }
    }
}

template <int DIN, int DOUT>
static int launch_wgrad_rowbias(const WgradRowBiasArgs& a, int H, int nblk, float* out, int accumulate, hipStream_t s) {
    constexpr int KC = (DIN + DOUT <= 4) ? 16 : 8;
    const int NP = DIN * H + H + H * DOUT + DOUT;
    clear_hip_error();
    hipLaunchKernelGGL((mlp_wgrad_rowbias_kernel<DIN, DOUT>), dim3(nblk, H / KC), dim3(256), 0, s, a, H);
    launch_reduce_rows(a.partial, nblk, NP, NP, out, accumulate, s);      // (workgroups in order)
    return launch_status();
}

}  // namespace psvo

// (four segments per workgroup and trip; >= 8 trips amortise the final reduction)
extern "C" int psvo_mlp_wgrad_rowbias_blocks(long long S) {
    long long nb = (S + 4 * 8 - 1) / (4 * 8);
    if (nb < 1) nb = 1;
    if (nb > 1024) nb = 1024;
    return (int)nb;
}

extern "C" int psvo_mlp_wgrad_rowbias(long long S, int L, int Din, int H, int Dout, const float* X, const float* dOut,
                                      const float* hb, const psvo_mlp* w, float* partial, float* grad, float* dhb,
                                      int accumulate, void* stream) {
    using namespace psvo;
    if (!X || !dOut || !hb || !w || !partial || !grad || !dhb || S <= 0 || L <= 0) return PSVO_ERR_INVALID;
    if (H != 16 && H != 32 && H != 64) return PSVO_ERR_UNSUPPORTED;
    WgradRowBiasArgs a{S, L, X, dOut, hb, *w, partial, dhb};
    const int nblk = psvo_mlp_wgrad_rowbias_blocks(S);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return pick<1, 2, 3, 4>(Din, [&](auto din) {
        return pick<1, 2, 3, 4>(Dout, [&](auto dout) { return launch_wgrad_rowbias<din(), dout()>(a, H, nblk, grad, accumulate, s); });
    });
}
