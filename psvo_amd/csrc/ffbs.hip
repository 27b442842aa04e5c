// Marginal particle smoother (forward filtering, backward smoothing) on the particle system a forward filter left in HBM.
// Restates FFBS_reweight_log_Ws of the reference's stale sweep code (not_used/SMC_supreme/SMC.py:451-482, smoothing_perc = 1,
// normalised inputs) and the resampling by the reweighted weights (:87-94) -- see include/psvo_hip.h for the contract.
//
// Work decomposition (MI355X): one persistent workgroup per sequence walks t = T-1 .. 0; lane = particle.  A step is two
// N x N pair phases over the transition density l[j,k] = log N(X[t+1][j]; Fm[t][k], s[t][k]), which is recomputed in both and
// never stored:
//     pass 1  lane = j, loop over k:  den[j] = logsumexp_k(a[k] + l[j,k])          rows k broadcast from LDS
//     pass 2  lane = k, loop over j:  S[k]   = a[k] + logsumexp_j(c[j] + l[j,k])   rows j broadcast from LDS,  c = S[t+1] - den
// Everything in the loops is in the log2 domain (v_exp_f32 / v_log_f32 are base 2): with r = sqrt(log2(e) / 2) / s and
// cst = -sum_d log2 s_d - Dx/2 log2(2 pi) the pair term is  log2(e) l[j,k] = cst[k] - sum_d ((x[j,d] - m[k,d]) r[k,d])^2, and cst[k]
// is folded into the staged a[k] (pass 1) or added after the loop (pass 2).  Both log-sum-exps are max-shifted online, four
// pairs per rescale (5 exponentials per 4 pairs), the squares on packed f32 pairs.  S[t] is renormalised every step, so the weights sum to one to rounding
// however sharp the transitions are.  No atomics; every sum is a per-lane loop, a wave scan or a fold over the <= 8 waves in
// wave order: the output is the same bit for bit on every run.
#include "common.h"
#include "ffbs_pair.h"

namespace psvo {

struct FfbsArgs {
    int B, T, N;
    const float *X, *Fm, *Fs, *sig_f, *logW, *u;
    const int32_t* idx_in;
    float *logWs, *Xmean, *ess, *Xs;
    int32_t* idx_out;
};

template <int DX, int COV, int MAXT>
__global__ void __launch_bounds__(MAXT) ffbs_kernel(const FfbsArgs a) {
    constexpr int DXP = ffbs_dxp(DX);
    constexpr float kHalfLog2e = 0.8493218002880191f;      // sqrt(log2(e) / 2)
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = blockDim.x, nw = NT >> 6;
    const int b = blockIdx.x, B = a.B, T = a.T, N = a.N;
    const bool valid = tid < N;
    const int n = valid ? tid : N - 1;      // clamp so that loads stay in bounds
    const int n8 = (N + 7) & ~7;            // staged rows the pair loops walk (<= NT)
    const float ninf = -__builtin_huge_valf();

    float* sA = smem;                 // [NT]      pass 1 rows: a[k] log2(e) + cst[k]
    float* sc = sA + NT;              // [NT]      pass 2 rows: c[j] (log2 domain)
    float* cdf = sc + NT;             // [NT]      inclusive prefix sums of the smoothed weights
    float* sm = cdf + NT;             // [NT][DXP] pass 1 rows: Fm[t][k]
    float* sx = sm + DXP * NT;        // [NT][DXP] pass 2 rows: X[t+1][j]
    float* red = sx + DXP * NT;       // [5 + DX][8] per-wave partials: max a, sum a, max S, sum S, sum w^2, sum w x_d
    float* sr = red + (5 + DX) * 8;   // [NT][DXP] pass 1 rows: r[k] (COV only)

    const bool draw = (a.u != nullptr || a.idx_in != nullptr) && (a.Xs != nullptr || a.idx_out != nullptr);

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

    // rows of one step: logW[t], X[t], Fm[t], Fs[t] and the step's uniform / teacher-forced draw.  No branch in here: row T-1
    // of Fm / Fs is loaded though the recursion has no use for it, and the last step prefetches row 0 again (a branch made
    // hipcc keep the prefetched rows in scratch and wait for them at once)
    auto load_rows = [&](int t, float& lw, float (&x)[DX], float (&fm)[DX], float (&fs)[DX], float& uu, int& ii) {
        const size_t tb = (size_t)t * B + b;
        lw = a.logW[tb * N + n];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            x[d] = a.X[(tb * DX + d) * N + n];
            fm[d] = a.Fm[(tb * DX + d) * N + n];
            if constexpr (COV) fs[d] = a.Fs[(tb * DX + d) * N + n];
        }
        if (draw) {
            if (a.idx_in) ii = a.idx_in[tb * N + n];
            else uu = a.u[tb * N + n];
        }
    };

    // max and sum over the workgroup, folded over the waves in wave order (slot: which rows of red[])
    auto block_max_of = [&](float v, int slot) {
        v = wave_max(v);
        if (lane == 0) red[slot * 8 + wave] = v;
        __syncthreads();
        float m = red[slot * 8];
        for (int i = 1; i < nw; ++i) m = fmaxf(m, red[slot * 8 + i]);
        return m;
    };

    float lw_c, x_c[DX], fm_c[DX], fs_c[DX], u_c = 0.f;
    int idx_c = 0;
#pragma unroll
    for (int d = 0; d < DX; ++d) fs_c[d] = 1.f;
    load_rows(T - 1, lw_c, x_c, fm_c, fs_c, u_c, idx_c);

    float xnext[DX];        // X[t+1] of this lane's particle
    float Snext = ninf;     // normalised S[t+1] of this lane's particle, log2 domain
#pragma unroll
    for (int d = 0; d < DX; ++d) xnext[d] = 0.f;

    for (int t = T - 1; t >= 0; --t) {
        const size_t tb = (size_t)t * B + b;
        float lw_n, x_n[DX], fm_n[DX], fs_n[DX], u_n = 0.f;
        int idx_n = 0;
#pragma unroll
        for (int d = 0; d < DX; ++d) fs_n[d] = 1.f;
        load_rows(max(t - 1, 0), lw_n, x_n, fm_n, fs_n, u_n, idx_n);      // prefetch: consumed one step later

        // v: what is normalised into S[t] -- the filter's log-weights at t = T-1 (natural log: mult = log2 e), the
        // recursion's S afterwards (log2 domain: mult = 1); outscale turns (v - max) back into natural log
        float v = valid ? lw_c : ninf, mult = kLog2e, outscale = 1.f;
        if (t < T - 1) {
            // ---- a[k] = logW[t][k] - logsumexp logW[t] ----------------------------------------------------------------
            const float mx = block_max_of(v, 0);
            const float mb = (mx == ninf) ? 0.f : mx;
            const float w = valid ? exp2_fast((lw_c - mb) * kLog2e) : 0.f;
            const float ws = wave_sum(w);
            if (lane == 0) red[8 + wave] = ws;
            // ---- stage the rows of both pair phases -------------------------------------------------------------------
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
            float row_m[DX], row_x[DX], row_r[DX];      // (padding rows: zeros, so that their pair term stays -inf)
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                row_m[d] = valid ? fm_c[d] : 0.f;
                row_x[d] = valid ? xnext[d] : 0.f;
                row_r[d] = valid ? r[d] : 0.f;
            }
            lds_row_store<DX>(sm + tid * DXP, row_m);
            lds_row_store<DX>(sx + tid * DXP, row_x);
            if constexpr (COV) lds_row_store<DX>(sr + tid * DXP, row_r);
            __syncthreads();
            float tot = 0.f;
            for (int i = 0; i < nw; ++i) tot += red[8 + i];
            const float a2 = (lw_c - mb) * kLog2e - log2_fast(tot);
            const float A = valid ? a2 + cst : ninf;
            sA[tid] = A;
            __syncthreads();
            // ---- pass 1: lane = j ---------------------------------------------------------------------------------------
            f2 own2[(DX + 1) / 2], r2[(DX + 1) / 2];
            pack_row<DX>(xnext, own2);
            pack_row<DX>(rc, r2);
            const float den = pair_lse<DX, COV != 0>(sA, sm, sr, own2, r2, n8);
            sc[tid] = (valid && Snext != ninf) ? Snext - den : ninf;
            __syncthreads();
            // ---- pass 2: lane = k ---------------------------------------------------------------------------------------
            pack_row<DX>(fm_c, own2);
            pack_row<DX>(r, r2);
            const float L = pair_lse<DX, false>(sc, sx, sr, own2, r2, n8);
            v = valid ? A + L : ninf;
            mult = 1.f;
            outscale = kLn2;
        }

        // ---- normalise S[t]; weights, their prefix sums, effective sample size, smoothed mean ------------------------
        const float mx = block_max_of(v, 2);
        const float mb = (mx == ninf) ? 0.f : mx;
        const float dv = v - mb;
        const float w = valid ? exp2_fast(dv * mult) : 0.f;
        float scan = wave_incl_scan(w, lane);
        const float w2 = wave_sum(w * w);
        float wx[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) wx[d] = wave_sum(w * x_c[d]);
        if (lane == 63) red[3 * 8 + wave] = scan;
        if (lane == 0) {
            red[4 * 8 + wave] = w2;
#pragma unroll
            for (int d = 0; d < DX; ++d) red[(5 + d) * 8 + wave] = wx[d];
        }
        __syncthreads();
        float off = 0.f, total = 0.f;
        for (int i = 0; i < nw; ++i) {
            const float q = red[3 * 8 + i];
            if (i < wave) off += q;
            total += q;
        }
        scan += off;
        const float l2t = log2_fast(total);
        Snext = valid ? fmaf(dv, mult, -l2t) : ninf;
        if (valid) a.logWs[tb * N + n] = fmaf(dv, outscale, -kLn2 * l2t);
        if (tid <= DX && (tid == 0 ? a.ess != nullptr : a.Xmean != nullptr)) {
            float q = 0.f;
            for (int i = 0; i < nw; ++i) q += red[(4 + tid) * 8 + i];
            if (tid == 0) a.ess[tb] = fminf(fmaxf(total * total / q, 1.f), (float)N);      // (1 <= ess <= N holds exactly; rounding may not)
            else a.Xmean[tb * DX + (tid - 1)] = q / total;
        }

        // ---- N multinomial draws from exp S[t] (the filter's draw: cdf[idx-1] <= u total < cdf[idx]) and the gather ----
        if (draw) {
            int idx;
            if (a.idx_in) {
                idx = min(max(idx_c, 0), N - 1);
            } else {
                cdf[tid] = scan;
                __syncthreads();
                // count of cdf entries <= u * total (cdf is non-decreasing)
                const float target = u_c * total;
                int pos = 0;
                for (int s = 1 << (31 - __clz(N)); s > 0; s >>= 1) {
                    const int p = pos + s;
                    if (p <= N && cdf[p - 1] <= target) pos = p;
                }
                idx = min(pos, N - 1);
            }
            if (valid) {
                if (a.idx_out) a.idx_out[tb * N + n] = idx;
                if (a.Xs) {
#pragma unroll
                    for (int d = 0; d < DX; ++d) a.Xs[(tb * DX + d) * N + n] = a.X[(tb * DX + d) * N + idx];
                }
            }
        }

#pragma unroll
        for (int d = 0; d < DX; ++d) {
            xnext[d] = x_c[d];
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
static int launch_ffbs(const FfbsArgs& a, hipStream_t stream) {
    constexpr int DXP = ffbs_dxp(DX);
    const int NT = (a.N + 63) & ~63;
    const size_t lds = sizeof(float) * ((size_t)(3 + (2 + COV) * DXP) * NT + (5 + DX) * 8);
    clear_hip_error();
    if (NT <= 256) hipLaunchKernelGGL((ffbs_kernel<DX, COV, 256>), dim3(a.B), dim3(NT), lds, stream, a);
    else hipLaunchKernelGGL((ffbs_kernel<DX, COV, 512>), dim3(a.B), dim3(NT), lds, stream, a);
    return launch_status();
}

}  // namespace psvo

extern "C" int psvo_ffbs_smooth(const psvo_desc* desc, const float* X, const float* Fm, const float* Fs, const float* sig_f,
                                const float* logW, const float* u, const int32_t* idx_in, float* logWs, float* Xmean,
                                float* ess, float* Xs, int32_t* idx_out, void* stream) {
    using namespace psvo;
    if (!desc || !X || !Fm || !logW || !logWs) return PSVO_ERR_INVALID;
    if ((Fs != nullptr) == (sig_f != nullptr)) return PSVO_ERR_INVALID;
    if ((Xs || idx_out) && !u && !idx_in) return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->N > 512) return PSVO_ERR_UNSUPPORTED;

    FfbsArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N;
    a.X = X; a.Fm = Fm; a.Fs = Fs; a.sig_f = sig_f; a.logW = logW; a.u = u; a.idx_in = idx_in;
    a.logWs = logWs; a.Xmean = Xmean; a.ess = ess; a.Xs = Xs; a.idx_out = idx_out;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return pick_dx(desc->Dx, [&](auto dx) {
        return Fs ? launch_ffbs<dx(), 1>(a, s) : launch_ffbs<dx(), 0>(a, s); });
}
