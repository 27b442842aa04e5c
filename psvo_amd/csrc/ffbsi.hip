// Backward-sampled trajectories (forward filtering, backward simulation: FFBSi) on the particle system a forward filter left
// in HBM -- see include/psvo_hip.h (psvo_ffbs_sample) for the contract.  N whole paths per sequence: path n picks its particle
// of step t given the particle it picked at t+1,
//     v[n,k] = a_t[k] + l_t(X[t+1][j_{t+1}(n)]; k),   j_t(n) ~ exp v[n,.],   logq = v[n,j_t(n)] - logsumexp_k v[n,.].
//
// Work decomposition (MI355X), the one of ffbs_kernel: one persistent workgroup per sequence walks t = T-1 .. 0.  Here a lane
// is a TRAJECTORY; its own point is its successor state (the row it gathered one step earlier, kept in registers) and the rows
// k of the step sit in LDS: a_t[k] log2(e) + cst[k], Fm[t][k], r[k] (per-particle scales only) and X[t][k] for the gather.  A
// step is two pair phases of the smoother's pass-1 geometry (rows read at wave-uniform addresses, ffbs_pair.h); the N x N tile
// is recomputed in both and never stored:
//     phase 1  L[n] = log2 sum_k exp2 v[n,k]                        pair_lse: max-shifted, online
//     phase 2  e[k] = exp2(v[n,k] - L[n]);  cdf[k] = e[0] + .. + e[k] (k order, one accumulator);  j = #{k : cdf[k] <= u[n]}
// Phase 2 divides by what phase 1 summed, so the weights it accumulates are normalised and `total` is 1 by construction -- to
// the rounding of L, one fp32 number of the size of the v's themselves (DESIGN.md section 4 has the error budget).  The count
// runs over all rows with a fixed trip count and no early exit.  cdf[N-1] may therefore end a few ulps BELOW u; the count then
// passes the last particle, and it is clamped to the last row with logW > -inf (found once per step), not to N-1.  Rows of
// weight zero add nothing to cdf, so an interior or leading one can never be the first row whose cdf exceeds u: a particle of
// weight zero is never drawn.
// At t = T-1 there is no successor: the rows are staged with zero means, zero scale factors and cst = 0 and the own point is
// zero, so that v[n,k] = a[k] falls out of the same code.
// No atomics; every sum is a per-lane loop in k order, a wave scan or a fold over the <= 8 waves in wave order: the output is
// the same bit for bit on every run.
#include "common.h"
#include "ffbs_pair.h"

namespace psvo {

struct FfbsiArgs {
    int B, T, N;
    const float *X, *Fm, *Fs, *sig_f, *logW, *u;
    const int32_t* idx_in;
    float* Xs;
    int32_t* idx_out;
    float* logq;
    int32_t* distinct;
};

// #{k : cdf[k] <= target} over the n8 staged rows, cdf the running sum in k order of exp2(v[k] - lse) with the pair term v[k]
// of pair_lse (same expression, same read-ahead: four rows, one group ahead of the arithmetic).  Padding rows (sv = -inf) add
// zero, so the count can pass N only when target >= the whole sum; the caller clamps.
template <int DX, bool ROWSCALE>
__device__ __forceinline__ int pair_count(const float* __restrict__ sv, const float* __restrict__ sp,
                                          const float* __restrict__ sr, const f2 (&own)[(DX + 1) / 2],
                                          const f2 (&r)[(DX + 1) / 2], int n8, float lse, float target) {
    constexpr int NP = (DX + 1) / 2;
    float cdf = 0.f;
    int cnt = 0;
    auto fold = [&](const Rows4<DX, ROWSCALE>& R) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f2 acc = f2{0.f, 0.f};
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const f2 z = (R.p[i][q] - own[q]) * (ROWSCALE ? R.rr[i][q] : r[q]);
                acc = pk_fma(z, z, acc);
            }
            const float v = R.v[i] - (acc.x + acc.y);
            cdf += exp2_fast(v - lse);
            cnt += (cdf <= target) ? 1 : 0;
        }
    };
    Rows4<DX, ROWSCALE> even, odd;
    even.load(sv, sp, sr, 0);
    for (int i0 = 0; i0 < n8; i0 += 8) {
        odd.load(sv, sp, sr, i0 + 4);
        fold(even);
        even.load(sv, sp, sr, i0 + 8 < n8 ? i0 + 8 : 0);      // (the last read-ahead wraps to group 0 and is not used)
        fold(odd);
    }
    return cnt;
}

template <int DX, int COV, int MAXT>
__global__ void __launch_bounds__(MAXT) ffbsi_kernel(const FfbsiArgs a) {
    constexpr int DXP = ffbs_dxp(DX);
    constexpr int NP = (DX + 1) / 2;
    constexpr float kHalfLog2e = 0.8493218002880191f;      // sqrt(log2(e) / 2)
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = blockDim.x, nw = NT >> 6;
    const int b = blockIdx.x, B = a.B, T = a.T, N = a.N;
    const bool valid = tid < N;
    const int n = valid ? tid : N - 1;      // clamp so that loads stay in bounds
    const int n8 = (N + 7) & ~7;            // staged rows the pair loops walk (<= NT)
    const float ninf = -__builtin_huge_valf();

    float* sA = smem;                                       // [NT]      rows: a[k] log2(e) + cst[k]
    float* sm = sA + NT;                                    // [NT][DXP] rows: Fm[t][k]
    float* sx = sm + DXP * NT;                              // [NT][DXP] rows: X[t][k], what the draw gathers
    int* flag = reinterpret_cast<int*>(sx + DXP * NT);      // [NT]      1 where some trajectory drew row k
    float* red = reinterpret_cast<float*>(flag + NT);       // [4][8]    per-wave partials: max logW, sum w, last live row, distinct
    int* redi = reinterpret_cast<int*>(red);
    float* sr = red + 4 * 8;                                // [NT][DXP] rows: r[k] (COV only)

    // constant transition scale: r and cst once
    float rc[DX];
    float cstc = -DX * kHalfLog2Pi * kLog2e;
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        rc[d] = 0.f;
        if constexpr (!COV) {
            const float s = a.sig_f[d];
            rc[d] = kHalfLog2e / s;
            cstc -= log2_fast(s);
        }
    }

    // rows of one step: logW[t], X[t], Fm[t], Fs[t] and the step's uniform / teacher-forced index.  No branch in here: row T-1
    // of Fm / Fs is loaded though the recursion has no use for it, and the last step prefetches row 0 again
    // (profiles/ffbs_smoother.md: a branch made hipcc keep the prefetched rows in scratch and wait for them at once)
    auto load_rows = [&](int t, float& lw, float (&x)[DX], float (&fm)[DX], float (&fs)[DX], float& uu, int& ii) {
        const size_t tb = (size_t)t * B + b;
        lw = a.logW[tb * N + n];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            x[d] = a.X[(tb * DX + d) * N + n];
            fm[d] = a.Fm[(tb * DX + d) * N + n];
            if constexpr (COV) fs[d] = a.Fs[(tb * DX + d) * N + n];
        }
        if (a.idx_in) ii = a.idx_in[tb * N + n];
        else uu = a.u[tb * N + n];
    };

    float lw_c, x_c[DX], fm_c[DX], fs_c[DX], u_c = 0.f;
    int idx_c = 0;
#pragma unroll
    for (int d = 0; d < DX; ++d) fs_c[d] = 1.f;
    load_rows(T - 1, lw_c, x_c, fm_c, fs_c, u_c, idx_c);

    float xsucc[DX];        // X[t+1] at the index this trajectory drew there
#pragma unroll
    for (int d = 0; d < DX; ++d) xsucc[d] = 0.f;

    for (int t = T - 1; t >= 0; --t) {
        const size_t tb = (size_t)t * B + b;
        const bool last = t == T - 1;
        float lw_n, x_n[DX], fm_n[DX], fs_n[DX], u_n = 0.f;
        int idx_n = 0;
#pragma unroll
        for (int d = 0; d < DX; ++d) fs_n[d] = 1.f;
        load_rows(max(t - 1, 0), lw_n, x_n, fm_n, fs_n, u_n, idx_n);      // prefetch: consumed one step later

        // ---- a[k] = logW[t][k] - logsumexp logW[t]; the last row of weight > 0 -------------------------------------------
        const float lw = valid ? lw_c : ninf;
        const float wm = wave_max(lw);
        const unsigned long long live = __ballot(lw > ninf);
        if (lane == 0) {
            red[wave] = wm;
            redi[2 * 8 + wave] = live ? wave * 64 + 63 - __builtin_clzll(live) : -1;
        }
        __syncthreads();
        float mx = red[0];
        for (int i = 1; i < nw; ++i) mx = fmaxf(mx, red[i]);
        const float mb = (mx == ninf) ? 0.f : mx;
        const float w = valid ? exp2_fast((lw_c - mb) * kLog2e) : 0.f;
        const float ws = wave_sum(w);
        if (lane == 0) red[8 + wave] = ws;
        // ---- stage the rows ------------------------------------------------------------------------------------------------
        float r[DX], cst = cstc;
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            if constexpr (COV) {
                r[d] = kHalfLog2e / fs_c[d];
                cst -= log2_fast(fs_c[d]);
            } else {
                r[d] = rc[d];
            }
        }
        const bool pairs = valid && !last;      // (padding rows and step T-1: zeros, the pair term is then exactly zero)
        float row_m[DX], row_x[DX], row_r[DX], rl[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            row_m[d] = pairs ? fm_c[d] : 0.f;
            row_x[d] = valid ? x_c[d] : 0.f;
            row_r[d] = pairs ? r[d] : 0.f;
            rl[d] = last ? 0.f : rc[d];
        }
        lds_row_store<DX>(sm + tid * DXP, row_m);
        lds_row_store<DX>(sx + tid * DXP, row_x);
        if constexpr (COV) lds_row_store<DX>(sr + tid * DXP, row_r);
        flag[tid] = 0;
        __syncthreads();
        float tot = 0.f;
        int kmax = redi[2 * 8];
        for (int i = 0; i < nw; ++i) tot += red[8 + i];
        for (int i = 1; i < nw; ++i) kmax = max(kmax, redi[2 * 8 + i]);
        const float a2 = (lw_c - mb) * kLog2e - log2_fast(tot);
        sA[tid] = valid ? a2 + (last ? 0.f : cst) : ninf;
        __syncthreads();

        // ---- phase 1: log2 sum_k exp2 v[n,k];  phase 2: the draw ---------------------------------------------------------
        f2 own2[NP], r2[NP];
        pack_row<DX>(xsucc, own2);
        pack_row<DX>(rl, r2);
        const float lse = pair_lse<DX, COV != 0>(sA, sm, sr, own2, r2, n8);
        int idx;
        if (a.idx_in) idx = idx_c;
        else idx = min(pair_count<DX, COV != 0>(sA, sm, sr, own2, r2, n8, lse, u_c), kmax);
        idx = min(max(idx, 0), N - 1);

        // ---- the drawn row: its pair term once more (logq), its state (the gather, and the own point of step t-1) ----------
        f2 pj[NP], rj[NP], xj[NP];
        lds_row_load2<DX>(sm + idx * DXP, pj);
        lds_row_load2<DX>(sx + idx * DXP, xj);
        if constexpr (COV) lds_row_load2<DX>(sr + idx * DXP, rj);
        f2 acc = f2{0.f, 0.f};
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const f2 z = (pj[q] - own2[q]) * (COV ? rj[q] : r2[q]);
            acc = pk_fma(z, z, acc);
        }
        const float vj = sA[idx] - (acc.x + acc.y);
        if (valid) flag[idx] = 1;
#pragma unroll
        for (int d = 0; d < DX; ++d) xsucc[d] = (d & 1) ? xj[d >> 1].y : xj[d >> 1].x;
        if (valid) {
            if (a.logq) a.logq[tb * N + n] = (vj - lse) * kLn2;
            if (a.idx_out) a.idx_out[tb * N + n] = idx;
            if (a.Xs) {
#pragma unroll
                for (int d = 0; d < DX; ++d) a.Xs[(tb * DX + d) * N + n] = xsucc[d];
            }
        }

        // ---- distinct rows among the N draws: ballot the flags, fold over the waves ----------------------------------------
        __syncthreads();
        const unsigned long long hit = __ballot(valid && flag[tid] != 0);
        if (lane == 0) redi[3 * 8 + wave] = __popcll(hit);
        __syncthreads();
        if (tid == 0 && a.distinct) {
            int c = 0;
            for (int i = 0; i < nw; ++i) c += redi[3 * 8 + i];
            a.distinct[tb] = c;
        }

#pragma unroll
        for (int d = 0; d < DX; ++d) {
            x_c[d] = x_n[d];
            fm_c[d] = fm_n[d];
            fs_c[d] = fs_n[d];
        }
        lw_c = lw_n;
        u_c = u_n;
        idx_c = idx_n;
    }
}

template <int DX, int COV>
static int launch_ffbsi(const FfbsiArgs& a, hipStream_t stream) {
    constexpr int DXP = ffbs_dxp(DX);
    const int NT = (a.N + 63) & ~63;
    const size_t lds = sizeof(float) * ((size_t)(2 + (2 + COV) * DXP) * NT + 4 * 8);
    clear_hip_error();
    if (NT <= 256) hipLaunchKernelGGL((ffbsi_kernel<DX, COV, 256>), dim3(a.B), dim3(NT), lds, stream, a);
    else hipLaunchKernelGGL((ffbsi_kernel<DX, COV, 512>), dim3(a.B), dim3(NT), lds, stream, a);
    return launch_status();
}

}  // namespace psvo

extern "C" int psvo_ffbs_sample(const psvo_desc* desc, const float* X, const float* Fm, const float* Fs, const float* sig_f,
                                const float* logW, const float* u, const int32_t* idx_in, float* Xs, int32_t* idx_out,
                                float* logq, int32_t* distinct, void* stream) {
    using namespace psvo;
    if (!desc || !X || !Fm || !logW) return PSVO_ERR_INVALID;
    if ((Fs != nullptr) == (sig_f != nullptr)) return PSVO_ERR_INVALID;
    if (!u && !idx_in) return PSVO_ERR_INVALID;
    if (!Xs && !idx_out && !logq && !distinct) return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->N > 512) return PSVO_ERR_UNSUPPORTED;

    FfbsiArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N;
    a.X = X; a.Fm = Fm; a.Fs = Fs; a.sig_f = sig_f; a.logW = logW; a.u = u; a.idx_in = idx_in;
    a.Xs = Xs; a.idx_out = idx_out; a.logq = logq; a.distinct = distinct;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return pick_dx(desc->Dx, [&](auto dx) {
        return Fs ? launch_ffbsi<dx(), 1>(a, s) : launch_ffbsi<dx(), 0>(a, s); });
}
