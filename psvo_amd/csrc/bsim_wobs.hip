// Backward simulation with proposal (PSVO) and its reverse pass for wide observations, 3 <= Dy <= 32
// (include/psvo_hip.h: psvo_bsim_forward_wobs, psvo_bsim_backward_wobs).  Companion of filter_wobs.hip.
//
// Same mathematics and contract as bsim_fwd.hip / bsim_bwd_impl.h (state-independent scales): the N x N transition term is
// recomputed from an LDS-staged tile of (F'_j, W'_j) = (Fm_j rho, (logW_j - lse) log2 e) and never stored, the log-sum-exp is
// online in the log2 domain, the sub-particle pick is the count of CDF entries <= u * total.  What differs is the emission:
// Dy is a RUN-TIME bound and nothing is instantiated per width.  A lane keeps the H hidden activations of MLP_g at its
// sub-particle and walks the outputs e = 0 .. Dy-1 in a rolled loop; row e of the transposed output layer, b2[e], 1 / sig_g[e]
// and y[t,b,e] are read from LDS at wave-uniform addresses, and z_e^2 is added in that order (wobs_common.h: GLds).  The
// step's observation row is loaded once per workgroup, one step ahead, into the other half of a two-row LDS buffer.
//
// Work decomposition: the generic one of bsim_cov.hip, not the tuned quad-blocked / half-split forms -- workgroup = 256 / M
// chains of ONE sequence, lane = (chain, sub-particle m), persistent over the steps (forward: t = T-1 .. 0, reverse:
// t = 0 .. T-1).  Kernels are instantiated per (Dx in {2,3,4}, H in {16,32,64}, M in {4,8,16,32}).
//
// Reverse pass: no float atomics, every sum has one fixed order.
//   * pair phase with j on the lanes of a 16-lane row (bsim_cov.hip): per-item sums (d x~) in registers, reduced over the row
//     with four DPP rotations; per-j sums (d F'_j, d W^_j) reduced over the four rows with two swap-adds and stored, one
//     writer per (wave, q, j), into a wave-private LDS copy; the copies are added in wave order into per-workgroup partials
//     (T,B,nblk,..) in the workspace, which bsim_bwd_fold_finalize (api.hip) adds in workgroup order;
//   * the emission walks the outputs once to write the d G row and the lane's column of d sig_g (LDS, [Dy][lanes], folded in
//     lane order after the time loop), then reads the row back to accumulate d h for 16 or 32 hidden units at a time -- the
//     register remedy of the wide reverse filter;
//   * the other scale sums are per-lane registers folded by block_sum (lanes by the DPP scan, waves in wave order).
//
// Missing observations (PSVO_MS = 1: bsim_wobs_ms.hip is `#define PSVO_MS 1` + `#include "bsim_wobs.hip"`, the kernels of
// psvo_bsim_forward_wobs_missing / psvo_bsim_backward_wobs_missing, 1 <= Dy <= 32): a NaN in obs is an observation that was not
// made, as in filter_wobs_impl.h.  o_e = (y == y) is a broadcast and only feeds selects: log g sums the observed terms in the
// order e = 0 .. Dy - 1 (nothing observed: exactly 0), and the normalising constant of the Gaussian forms is the LDS row
// c_e = -(log sig_g[e] + 1/2 log 2 pi) where the count form has its log-factorials.  Reverse: the d G row entry and the lane's
// d sig_g column entry of a missing output are selected to 0.  Everything that differs sits under `#if PSVO_MS`; the kernels
// live in a namespace of their own (psvo::wbs_ms), so that the two units' instantiations are distinct symbols.
#include "wobs_common.h"

#ifndef PSVO_MS
#define PSVO_MS 0
#endif
#if PSVO_MS
#define PSVO_WBS wbs_ms
#define PSVO_WBS_ENTRY(name) name##_missing
#define PSVO_WBS_MIN_DY 1
#else
#define PSVO_WBS wbs
#define PSVO_WBS_ENTRY(name) name
#define PSVO_WBS_MIN_DY 3
#endif

namespace psvo {
namespace PSVO_WBS {

using wobs::GLds;
using wobs::kMaxDy;

constexpr int kMaxStage = 2;      // forward-tile entries a thread stages per step (N <= 512 with 256 threads)

// workgroup geometry of both kernels: threads, chains per workgroup, workgroups per sequence
struct Geom {
    int ntb, cpb, nblk;
};
static Geom geometry(int N, int M) {
    int NTB = ((N * M + 63) / 64) * 64;
    if (NTB > 256) NTB = 256;
    const int cpb = NTB / M;
    return {NTB, cpb, (N + cpb - 1) / cpb};
}

struct FwdArgs {
    int B, T, N, Dy, emission;
    psvo_mlp f, g, q1inv;
    const float *Fm, *logW, *lse;
    const float *sig_f, *sig_g, *sig_q1inv, *sig_bq2;
    const float *bmu2, *minit, *sig_init, *imean, *isig;
    const float *obs, *eps_b, *u_b;
    const int32_t* sel_in;
    float *bwX, *flp, *glp, *Omega;
    int32_t* sel_out;
    float* score;
    float *lam2_all, *om_all, *mu1_all;
};

// CNT: the count emission (psvo_desc.emission = 2), a compile-time form as in filter_wobs.hip: 1 / sig_g is not used and the
// log-factorial row of a step travels with its observation row
template <int DX, int H, int M, bool CNT>
__global__ void __launch_bounds__(256) bsim_wobs_fwd_kernel(const FwdArgs a) {
    using MQ = MlpLds<DX, H, DX, 1>;
    using MG = GLds<DX, H>;
    constexpr int TS = DX + 1;          // tile slot: F'[DX] | W'
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int NTB = blockDim.x;
    const int B = a.B, T = a.T, N = a.N, Dy = a.Dy;
    const int NP = (N + 7) & ~7;        // tile padded (W' = -inf) to whole blocks of 8
    const int b = blockIdx.y;
    const int cpb = NTB / M;
    const int cl = tid / M, m = tid % M;
    const bool lead = (m == 0);
    const int n_raw = blockIdx.x * cpb + cl;
    const bool valid = n_raw < N;
    const int n = valid ? n_raw : N - 1;
    const int gbase = lane - m;

    float* wf = smem;
    float* wqi = wf + MQ::kSize;
    float* wg = wqi + MQ::kSize;
    float* isg = wg + MG::kSize;        // [kMaxDy] 1 / sig_g
    float* ybuf = isg + kMaxDy;         // [2][kMaxDy] observation rows of step t (t & 1) and t - 1
    float* tile = ybuf + 2 * kMaxDy;    // [2][NP][TS]
    float* lfbuf = tile + 2 * NP * TS;  // CNT: [2][kMaxDy] log Gamma(y + 1) of the rows in ybuf
#if PSVO_MS
    float* cg = tile + 2 * NP * TS;     // !CNT (no lfbuf then): [kMaxDy] -(log sig_g + 1/2 log 2 pi), the constant of one term
#endif

    MQ::load(wf, a.f, tid, NTB);
    MQ::load(wqi, a.q1inv, tid, NTB);
    MG::load(wg, a.g, Dy, tid, NTB);
    if (tid < Dy) {
        if constexpr (!CNT) isg[tid] = 1.f / a.sig_g[tid];
#if PSVO_MS
        if constexpr (!CNT) cg[tid] = -(logf(a.sig_g[tid]) + kHalfLog2Pi);
#endif
        const float y0 = a.obs[((size_t)(T - 1) * B + b) * Dy + tid];
        ybuf[((T - 1) & 1) * kMaxDy + tid] = y0;
        if constexpr (CNT) lfbuf[((T - 1) & 1) * kMaxDy + tid] = wobs::log_factorial(y0);
    }

    // ---- constants (bsim_fwd.hip) --------------------------------------------------------------------------------------
    float isf[DX], rp[DX];
    float kf = -DX * kHalfLog2Pi;
    const float rscale = sqrtf(0.5f * kLog2e);
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        const float s = a.sig_f[d];
        isf[d] = 1.f / s;
        rp[d] = isf[d] * rscale;
        kf -= logf(s);
    }
#if !PSVO_MS
    float lg = -Dy * kHalfLog2Pi;
    if constexpr (!CNT) {
        for (int e = 0; e < Dy; ++e) lg -= logf(a.sig_g[e]);
    }
#endif
    float pc[DX], pic[DX], pi1[DX], pi2[DX];
    float kq = -DX * kHalfLog2Pi;
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        pi1[d] = 1.f / a.sig_q1inv[d];
        pi2[d] = 1.f / a.sig_bq2[d];
        pic[d] = pi1[d] + pi2[d];
        pc[d] = 1.f / pic[d];
        kq -= logf(pc[d]);
    }
    float s_init[DX], is_init[DX], i_isig[DX], im[DX], mi[DX];
    float kinit = -DX * kHalfLog2Pi, kiota = -DX * kHalfLog2Pi;
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        s_init[d] = a.sig_init[d];
        is_init[d] = 1.f / s_init[d];
        kinit -= logf(s_init[d]);
        i_isig[d] = 1.f / a.isig[d];
        kiota -= logf(a.isig[d]);
        im[d] = a.imean[b * DX + d];
        mi[d] = a.minit[b * DX + d];
    }
    const float logM = logf((float)M);
    const float ninf = -__builtin_huge_valf();

    // ---- forward-tile staging: global -> registers at the top of a step, registers -> LDS at its end ---------------------
    float st[kMaxStage][DX + 1], st_l = 0.f;
    auto stage_load = [&](int tt) {
        const size_t tb = (size_t)tt * B + b;
        st_l = a.lse[tb];
#pragma unroll
        for (int r = 0; r < kMaxStage; ++r) {
            const int j = tid + r * NTB;
            if (j < NP) {
                const int jc = j < N ? j : N - 1;
#pragma unroll
                for (int d = 0; d < DX; ++d) st[r][d] = a.Fm[(tb * DX + d) * N + jc];
                st[r][DX] = a.logW[tb * N + jc];
            }
        }
    };
    auto stage_store = [&](float* buf) {
#pragma unroll
        for (int r = 0; r < kMaxStage; ++r) {
            const int j = tid + r * NTB;
            if (j < NP) {
#pragma unroll
                for (int d = 0; d < DX; ++d) buf[j * TS + d] = st[r][d] * rp[d];
                buf[j * TS + DX] = j < N ? (st[r][DX] - st_l) * kLog2e : ninf;
            }
        }
    };
    if (T >= 2) {
        stage_load(T - 2);
        stage_store(tile);
    }

    float eps_c[DX], bmu_c[DX], u_c = 0.f;
    int sel_c = 0;
    auto load_inputs = [&](int t, float (&e)[DX], float (&bm)[DX], float& uu, int& ss) {
        const size_t tb = (size_t)t * B + b;
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            e[d] = a.eps_b[((tb * DX + d) * N + n) * M + m];
            bm[d] = a.bmu2[tb * DX + d];
        }
        if (a.sel_in) ss = a.sel_in[tb * N + n];
        else uu = a.u_b[tb * N + n];
    };
    load_inputs(T - 1, eps_c, bmu_c, u_c, sel_c);
    __syncthreads();      // weights, scales, the first tile and observation row visible

    float xp[DX];   // x_{t+1} of this chain (same in all M lanes)
#pragma unroll
    for (int d = 0; d < DX; ++d) xp[d] = 0.f;
    float score = 0.f;

    for (int t = T - 1; t >= 0; --t) {
        const size_t tb = (size_t)t * B + b;
        const float* cur = tile + ((T - 1 - t) & 1) * NP * TS;
        float* nxt = tile + ((T - t) & 1) * NP * TS;
        const bool last = (t == T - 1), tzero = (t == 0);
        int zo = 0;
        asm volatile("" : "+v"(zo));        // MLP_g is re-read from LDS every step, never hoisted into registers
        const float* wg_t = wg + zo;
        const float* y_t = ybuf + (t & 1) * kMaxDy + zo;

        float eps_n[DX], bmu_n[DX], u_n = 0.f, y_n = 0.f;
        int sel_n = 0;
        if (!tzero) {
            load_inputs(t - 1, eps_n, bmu_n, u_n, sel_n);
            if (tid < Dy) y_n = a.obs[(tb - B) * Dy + tid];     // the next step's row, once per workgroup
        }
        if (t >= 2) stage_load(t - 2);

        // ---- proposal ---------------------------------------------------------------------------------------------------
        float x[DX], q_lp;
        if (last) {
            float mu[DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                mu[d] = mi[d];
                x[d] = fmaf(s_init[d], eps_c[d], mu[d]);
            }
            q_lp = diag_lp<DX>(x, mu, is_init, kinit);
            if (a.mu1_all && valid && lead) {
#pragma unroll
                for (int d = 0; d < DX; ++d) a.mu1_all[(tb * DX + d) * N + n] = 0.f;
            }
        } else {
            float m1[DX], mu[DX];
            MQ::template eval<true>(wqi, xp, m1);
            if (a.mu1_all && valid && lead) {
#pragma unroll
                for (int d = 0; d < DX; ++d) a.mu1_all[(tb * DX + d) * N + n] = m1[d];
            }
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                mu[d] = pc[d] * fmaf(pi1[d], m1[d], pi2[d] * bmu_c[d]);
                x[d] = fmaf(pc[d], eps_c[d], mu[d]);
            }
            q_lp = diag_lp<DX>(x, mu, pic, kq);
        }

        // ---- f(x_{t+1} | x~) ----------------------------------------------------------------------------------------------
        float phi = 0.f;
        if (!last) {
            float fmx[DX];
            MQ::template eval<true>(wf, x, fmx);
            phi = diag_lp<DX>(xp, fmx, isf, kf);
        }
        // ---- g(y_t | x~): Dy terms in the order e = 0 .. Dy - 1 -----------------------------------------------------------
        float g_lp;
        {
            float h[H];
            MG::hidden(wg_t, x, h);
            float acc = 0.f;
#if PSVO_MS
            // observed terms only, constant included, in the order e = 0 .. Dy - 1; nothing observed: exactly 0
            if constexpr (CNT) {
                const float* lf_t = lfbuf + (t & 1) * kMaxDy + zo;
#pragma unroll 1
                for (int e = 0; e < Dy; ++e) {
                    const float y = y_t[e];
                    const float term = wobs::count_term(y, MG::out(wg_t, e, h)) - lf_t[e];
                    acc += (y == y) ? term : 0.f;
                }
            } else {
                const float* cg_t = cg + zo;
#pragma unroll 1
                for (int e = 0; e < Dy; ++e) {
                    float gm = MG::out(wg_t, e, h);
                    if (a.emission) gm = emis_mean(gm);
                    const float y = y_t[e];
                    const float z = (y - gm) * isg[e];
                    const float term = fmaf(-0.5f * z, z, cg_t[e]);
                    acc += (y == y) ? term : 0.f;
                }
            }
            g_lp = acc;
#else
            if constexpr (CNT) {     // y log lam - lam - log Gamma(y + 1), one term per output
                const float* lf_t = lfbuf + (t & 1) * kMaxDy + zo;
#pragma unroll 1
                for (int e = 0; e < Dy; ++e) acc += wobs::count_term(y_t[e], MG::out(wg_t, e, h)) - lf_t[e];
                g_lp = acc;
            } else {
#pragma unroll 1
                for (int e = 0; e < Dy; ++e) {
                    float gm = MG::out(wg_t, e, h);
                    if (a.emission) gm = emis_mean(gm);
                    const float z = (y_t[e] - gm) * isg[e];
                    acc = fmaf(z, z, acc);
                }
                g_lp = fmaf(-0.5f, acc, lg);
            }
#endif
        }

        // ---- filter term: logsumexp_j( log f(x~ | X_{t-1}[j]) + W^_{t-1}[j] ), online in the log2 domain -----------------
        float lam;
        if (!tzero) {
            float xs_[DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) xs_[d] = x[d] * rp[d];
            float mx = ninf, sm = 0.f;
            for (int j0 = 0; j0 < NP; j0 += 8) {
                float v[8], bm = ninf;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float* p = cur + (j0 + c) * TS;
                    float acc = p[DX];
#pragma unroll
                    for (int d = 0; d < DX; ++d) {
                        const float u = xs_[d] - p[d];
                        acc = fmaf(-u, u, acc);
                    }
                    v[c] = acc;
                    bm = fmaxf(bm, acc);
                }
                const float nm = fmaxf(mx, bm);
                const float base = (nm == ninf) ? 0.f : nm;     // (every term so far -inf: keep sm = 0 without NaNs)
                sm *= exp2_fast(mx - base);
#pragma unroll
                for (int c = 0; c < 8; ++c) sm += exp2_fast(v[c] - base);
                mx = nm;
            }
            const float lam2 = mx + log2_fast(sm);
            lam = fmaf(kLn2, lam2, kf);
            if (a.lam2_all && valid) a.lam2_all[(tb * N + n) * M + m] = lam2;
        } else {
            lam = diag_lp<DX>(x, im, i_isig, kiota);   // t = 0: q0 / f density at mu_0 (PSVO.py:169-175)
        }

        // ---- omega, normalise over the M sub-particles, draw one -----------------------------------------------------------
        const float om_raw = lam + phi + g_lp - q_lp;
        const float omx = group_max<M>(om_raw);
        const float pw = exp2_fast((om_raw - omx) * kLog2e);
        const float cdfv = group_incl_scan<M>(pw, m);
        const float total = __shfl(cdfv, gbase + M - 1);
        const float omega = om_raw - fmaf(kLn2, log2_fast(total), omx);
        if (a.om_all && valid) a.om_all[(tb * N + n) * M + m] = omega;
        int sel;
        if (a.sel_in) {
            sel = min(max(sel_c, 0), M - 1);      // (teacher-forced picks are data: keep the shuffle inside the chain)
        } else {
            const unsigned long long bal = __ballot(cdfv <= u_c * total);
            const unsigned long long mask = ((1ull << M) - 1ull) << gbase;
            sel = min((int)__popcll(bal & mask), M - 1);
        }
        const int src = gbase + sel;
        float xs[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) xs[d] = __shfl(x[d], src);
        const float om_s = __shfl(omega, src), phi_s = __shfl(phi, src), g_s = __shfl(g_lp, src), q_s = __shfl(q_lp, src),
                    lam_s = __shfl(lam, src);
        const float Om = om_s + q_s + logM;
        if (valid && lead) {
#pragma unroll
            for (int d = 0; d < DX; ++d) a.bwX[(tb * DX + d) * N + n] = xs[d];
            a.glp[tb * N + n] = g_s;
            a.Omega[tb * N + n] = Om;
            a.sel_out[tb * N + n] = sel;
            if (!last) a.flp[(tb + B) * N + n] = phi_s;     // f_log_probs[t+1]
            if (tzero) a.flp[(size_t)b * N + n] = lam_s;    // f_log_probs[0] = f_init
        }
        score += g_s - Om + (last ? 0.f : phi_s) + (tzero ? lam_s : 0.f);

#pragma unroll
        for (int d = 0; d < DX; ++d) {
            xp[d] = xs[d];
            eps_c[d] = eps_n[d];
            bmu_c[d] = bmu_n[d];
        }
        u_c = u_n;
        sel_c = sel_n;
        if (t >= 2) stage_store(nxt);
        // the prefetched observation row goes to the half of ybuf that step t + 1 read (behind the barrier that ended it)
        if (!tzero && tid < Dy) {
            ybuf[((t - 1) & 1) * kMaxDy + tid] = y_n;
            if constexpr (CNT) lfbuf[((t - 1) & 1) * kMaxDy + tid] = wobs::log_factorial(y_n);
        }
        __syncthreads();
    }
    if (valid && lead) a.score[(size_t)b * N + n] = score;
}

template <int DX, int H>
static size_t fwd_lds_bytes(int N, bool count) {
    const int NP = (N + 7) & ~7;
    // (PSVO_MS: one more row, the per-output constants, where the count form has its log-factorials)
    return sizeof(float) * (2 * MlpLds<DX, H, DX, 1>::kSize + GLds<DX, H>::kSize + 3 * kMaxDy + 2 * (size_t)NP * (DX + 1) +
                            (count ? 2 * kMaxDy : PSVO_MS ? kMaxDy : 0));
}

template <int DX, int H, int M>
static int launch_fwd(const FwdArgs& a, hipStream_t stream) {
    const Geom ge = geometry(a.N, M);
    const bool count = a.emission == 2;
    const size_t lds = fwd_lds_bytes<DX, H>(a.N, count);
    clear_hip_error();
    if (count) hipLaunchKernelGGL((bsim_wobs_fwd_kernel<DX, H, M, true>), dim3(ge.nblk, a.B), dim3(ge.ntb), lds, stream, a);
    else hipLaunchKernelGGL((bsim_wobs_fwd_kernel<DX, H, M, false>), dim3(ge.nblk, a.B), dim3(ge.ntb), lds, stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------
// reverse pass: t = 0 .. T-1, carrying d loss / d bwX[t] of each chain.  With aw = d loss / d score of the chain,
// p_m = exp(omega_m) and s the drawn sub-particle (bsim_bwd_impl.h has the derivation):
//   d g_m = d phi_m = aw p_m,  d q_m = -aw p_m,  d lam_m = aw (p_m - [m == s]) (t >= 1),  aw p_m (t = 0),  d x_m += [m == s] d bwX[t].
// ---------------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
    int B, T, N, Dy, emission;
    psvo_mlp f, g, q1inv;
    const float *Fm, *logW, *lse;
    const float *sig_f, *sig_g, *sig_q1inv, *sig_bq2;
    const float *bmu2, *minit, *sig_init, *imean, *isig;
    const float *obs, *eps_b, *bwX;
    const int32_t* sel;
    const float *lam2_all, *om_all, *mu1_all, *dscore;
    float *xt, *dFt, *dGt, *dmu1;
    float *dbmu2_rows, *dminit_rows, *dimean_rows;
    float *dFm_part, *dlogW_part, *sacc_part;     // workspace: (T,B,nblk,Dx,N), (T,B,nblk,N), (B,nblk,7 Dx + Dy)
};

// CNT: the count emission; its d G rows are d g_m (y / lam - 1) sigmoid(r), there is no d sig_g
template <int DX, int H, int M, bool CNT>
__global__ void __launch_bounds__(256) bsim_wobs_bwd_kernel(const BwdArgs a) {
    using MQ = MlpLds<DX, H, DX, 1>;
    using MG = GLds<DX, H>;
    using AC = BAcc<DX>;
    constexpr int TS = DX + 1;
    constexpr int NA = DX + 1;                // per-j sums: d F' (DX), d W^
    constexpr int NI = DX + 2;                // floats per item of the pair phase: x' (DX), lam2, d lam
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NTB = blockDim.x, nwv = NTB >> 6;
    const int B = a.B, T = a.T, N = a.N, Dy = a.Dy;
    // (the host checked the envelope: the loops over Dy, N and the waves then need no uniform guard masks, which are SGPR pairs)
    __builtin_assume(Dy >= PSVO_WBS_MIN_DY && Dy <= kMaxDy && N >= 1 && N <= 512 && T >= 2 && NTB >= 64 && NTB <= 256 && B >= 1);
    const int NP = (N + 15) & ~15;            // tile padded (W' = -inf: zero weight) to whole tiles of 16
    const int b = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
    const int cpb = NTB / M;
    const int cl = tid / M, m = tid % M;
    const int n_raw = blk * cpb + cl;
    const bool valid = n_raw < N;
    const int n = valid ? n_raw : N - 1;
    const bool lead = valid && (m == 0);
    const int NACC = 7 * DX + Dy;

    float* wf = smem;
    float* wqi = wf + MQ::kSize;
    float* wg = wqi + MQ::kSize;
    float* isg = wg + MG::kSize;              // [kMaxDy]
    float* ybuf = isg + kMaxDy;               // [2][kMaxDy]
    float* red = ybuf + 2 * kMaxDy;           // [16]
    float* kst = red + 16;                    // [12][DX] step constants, see kIsf .. kMi
    float* xch = kst + 12 * DX;               // [4][64][NI] items of each wave
    // (what depends on N, Dy or the workgroup's size comes last: the bases above are compile-time constants, not SGPRs)
    float* tile = xch + 4 * 64 * NI;          // [NP][TS] tile of forward step t - 1
    float* jacc = tile + NP * TS;             // [nwv][NA][NP] per-j sums of the step, one copy per wave
    float* sg = jacc + nwv * NA * NP;         // [Dy][NTB] d sig_g sums, one column per lane

    MQ::load(wf, a.f, tid, NTB);
    MQ::load(wqi, a.q1inv, tid, NTB);
    MG::load(wg, a.g, Dy, tid, NTB);
    if (tid < Dy) {
        if constexpr (!CNT) isg[tid] = 1.f / a.sig_g[tid];
        ybuf[tid] = a.obs[(size_t)b * Dy + tid];
    }
    if constexpr (!CNT) {
        for (int e = 0; e < Dy; ++e) sg[e * NTB + tid] = 0.f;
    }

    // ---- constants (bsim_bwd_impl.h).  Wave-uniform values would live in SGPRs beside some thirty array pointers, more than
    // a wave has: the constants sit in LDS and are read where they are used, the pointers are re-read from the kernel
    // arguments at their point of use (common.h: PSVO_ARG) ----------------------------------------------------------------
    constexpr int kIsf = 0, kRp = DX, kIsfk = 2 * DX, kPc = 3 * DX, kPic = 4 * DX, kPi1 = 5 * DX, kPi2 = 6 * DX,
                  kSinit = 7 * DX, kIsinit = 8 * DX, kIisig = 9 * DX, kIm = 10 * DX, kMi = 11 * DX;
    if (tid < DX) {
        const int d = tid;
        const float kappa = sqrtf(0.5f * kLog2e);
        const float isf_ = 1.f / a.sig_f[d];
        const float i1 = 1.f / a.sig_q1inv[d], i2 = 1.f / a.sig_bq2[d];
        kst[kIsf + d] = isf_;
        kst[kRp + d] = isf_ * kappa;
        kst[kIsfk + d] = isf_ / kappa;
        kst[kPi1 + d] = i1;
        kst[kPi2 + d] = i2;
        kst[kPic + d] = i1 + i2;
        kst[kPc + d] = 1.f / (i1 + i2);
        kst[kSinit + d] = a.sig_init[d];
        kst[kIsinit + d] = 1.f / a.sig_init[d];
        kst[kIisig + d] = 1.f / a.isig[d];
        kst[kIm + d] = a.imean[b * DX + d];
        kst[kMi + d] = a.minit[b * DX + d];
    }
    const float ninf = -__builtin_huge_valf();
    const float aw = valid ? a.dscore[(size_t)b * N + n] : 0.f;   // d loss / d score of this chain

    float acc[7 * DX];
#pragma unroll
    for (int i = 0; i < 7 * DX; ++i) acc[i] = 0.f;
    float dX[DX];   // d loss / d bwX[t] of this chain (same value in its M lanes)
#pragma unroll
    for (int d = 0; d < DX; ++d) dX[d] = 0.f;

    for (int t_ = 0; t_ < T; ++t_) {
        // (the step index is opaque to the optimiser: with a visible induction variable it keeps a running address and a stride
        //  per array in SGPRs across the loop -- some thirty pairs, more than a wave has -- instead of forming addresses per step)
        //  Every section of the step forms its own (t, b) row index from it, so that no address outlives its section.)
        auto row = [&]() {
            int t = t_;
            asm volatile("" : "+s"(t));
            return (size_t)t * B + b;
        };
        auto width = [&]() {            // (N likewise, where the unrolled d * N would otherwise be kept as 64-bit pairs)
            int v = N;
            asm volatile("" : "+s"(v));
            return v;
        };
        const int t = t_;
        const bool last = (t == T - 1), first = (t == 0);
        int zo = 0;
        asm volatile("" : "+v"(zo));        // MLP_g is re-read from LDS every step, never kept in registers
        const float* wg_t = wg + zo;
        const float* y_t = ybuf + (t & 1) * kMaxDy + zo;
        const float* K = kst + zo;          // (the constants too)

        // ---- stage the tile of forward step t - 1 (the pair phase of step t - 1 ended at that step's barrier) -----------------
        if (!first) {
            const size_t pb = row() - B;
            const float* Fm = PSVO_ARG(BwdArgs, Fm);
            const float* logW = PSVO_ARG(BwdArgs, logW);
            const float l = PSVO_ARG(BwdArgs, lse)[pb];
            const int Nn = width();
            for (int j = tid; j < NP; j += NTB) {
                const int jc = j < N ? j : N - 1;
#pragma unroll
                for (int d = 0; d < DX; ++d) tile[j * TS + d] = Fm[(pb * DX + d) * Nn + jc] * K[kRp + d];
                tile[j * TS + DX] = j < N ? (logW[pb * N + jc] - l) * kLog2e : ninf;
            }
        }
        __syncthreads();      // tile (t = 0: weights, scales) and this step's observation row visible

        // ---- recompute the proposal ---------------------------------------------------------------------------------------
        float eps[DX], xp[DX], mu1[DX], bm[DX], mu[DX], x[DX];
        int sel;
        float pi_m;
        {
            const size_t tb = row();
            const int Nn = width();
            const float* eps_b = PSVO_ARG(BwdArgs, eps_b);
            const float* bmu2 = PSVO_ARG(BwdArgs, bmu2);
            const float* bwX = PSVO_ARG(BwdArgs, bwX);
            const float* mu1_all = PSVO_ARG(BwdArgs, mu1_all);
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                eps[d] = eps_b[((tb * DX + d) * Nn + n) * M + m];
                bm[d] = bmu2[tb * DX + d];
                xp[d] = last ? 0.f : bwX[((tb + B) * DX + d) * Nn + n];
                mu1[d] = last ? 0.f : mu1_all[(tb * DX + d) * Nn + n];
                if (!last) {
                    mu[d] = K[kPc + d] * fmaf(K[kPi1 + d], mu1[d], K[kPi2 + d] * bm[d]);
                    x[d] = fmaf(K[kPc + d], eps[d], mu[d]);
                } else {
                    mu[d] = K[kMi + d];
                    x[d] = fmaf(K[kSinit + d], eps[d], mu[d]);
                }
            }
            sel = PSVO_ARG(BwdArgs, sel)[tb * N + n];
            pi_m = valid ? exp2_fast(PSVO_ARG(BwdArgs, om_all)[(tb * N + n) * M + m] * kLog2e) : 0.f;
            if (valid) {
                float* xt = PSVO_ARG(BwdArgs, xt);
#pragma unroll
                for (int d = 0; d < DX; ++d) xt[((tb * DX + d) * Nn + n) * M + m] = x[d];
            }
        }
        const float issel = (m == sel) ? 1.f : 0.f;
        const float dphi = aw * pi_m;                             // = d g_m = -d q_m
        const float dlam = first ? dphi : aw * (pi_m - issel);

        float dx[DX], dxp_part[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            dx[d] = issel * dX[d];
            dxp_part[d] = 0.f;
        }

        // ---- g(y_t | x~): the d G row and the lane's column of d sig_g, outputs in the order o = 0 .. Dy - 1 ------------------
        float* const dGrow = PSVO_ARG(BwdArgs, dGt) + ((row() * Dy) * N + n) * M + m;     // the lane's row, stride N M
        const size_t gstride = (size_t)N * M;
        {
            float h[H];
            MG::hidden(wg_t, x, h);
#if PSVO_MS
            // a missing entry: its d G row entry is written as 0 (it is read back), its d sig_g column entry gets nothing
            if constexpr (CNT) {
#pragma unroll 1
                for (int o = 0; o < Dy; ++o) {
                    const float y = y_t[o];
                    const float dr = dphi * wobs::count_dterm(y, MG::out(wg_t, o, h));
                    if (valid) dGrow[o * gstride] = (y == y) ? dr : 0.f;
                }
            } else {
#pragma unroll 1
                for (int o = 0; o < Dy; ++o) {
                    float gm = MG::out(wg_t, o, h);
                    float dmean = 1.f;
                    if (a.emission) { dmean = emis_dmean(gm); gm = emis_mean(gm); }
                    const float is = isg[o];
                    const float y = y_t[o];
                    const bool ob = (y == y);
                    const float z = (y - gm) * is;
                    sg[o * NTB + tid] += ob ? dphi * (z * z - 1.f) * is : 0.f;
                    if (valid) dGrow[o * gstride] = ob ? dphi * z * is * dmean : 0.f;
                }
            }
#else
            if constexpr (CNT) {
#pragma unroll 1
                for (int o = 0; o < Dy; ++o) {
                    const float dr = dphi * wobs::count_dterm(y_t[o], MG::out(wg_t, o, h));
                    if (valid) dGrow[o * gstride] = dr;
                }
            } else {
#pragma unroll 1
                for (int o = 0; o < Dy; ++o) {
                    float gm = MG::out(wg_t, o, h);
                    float dmean = 1.f;
                    if (a.emission) { dmean = emis_dmean(gm); gm = emis_mean(gm); }
                    const float is = isg[o];
                    const float z = (y_t[o] - gm) * is;
                    sg[o * NTB + tid] += dphi * (z * z - 1.f) * is;
                    if (valid) dGrow[o * gstride] = dphi * z * is * dmean;
                }
            }
#endif
        }
        // (second walk over the outputs: the lane reads its own d G row back, hidden units in chunks)
        MG::template bwd_input<(H >= 64 ? 32 : 16)>(wg_t, Dy, dGrow, gstride, valid, x, dx);

        // ---- f(x_{t+1} | x~) ---------------------------------------------------------------------------------------------------
        {
            float dFo[DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) dFo[d] = 0.f;
            if (!last) {
                float fmx[DX];
                MQ::template eval<true>(wf, x, fmx);
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    const float isf = K[kIsf + d];
                    const float z = (xp[d] - fmx[d]) * isf;
                    dFo[d] = dphi * z * isf;
                    dxp_part[d] = -dFo[d];
                    acc[AC::kSf + d] += dphi * (z * z - 1.f) * isf;
                }
                MQ::template bwd_input<true>(wf, x, dFo, dx);
            }
            if (valid) {
                float* dFt = PSVO_ARG(BwdArgs, dFt);
                const size_t tb = row();
                const int Nn = width();
#pragma unroll
                for (int d = 0; d < DX; ++d) dFt[((tb * DX + d) * Nn + n) * M + m] = dFo[d];
            }
        }

        // ---- filter term ---------------------------------------------------------------------------------------------------------
        float dim_part[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) dim_part[d] = 0.f;
        if (!first) {
            // Pair phase with j ON THE LANES of a 16-lane row (bsim_cov.hip): row g = lane >> 4 works on the 16 items (chain, m)
            // its own lanes own, against forward particle j = 16 jt + j16 of tile jt.  Items travel through wave-private LDS
            // into registers once per step.
            float* const xw = xch + wave * 64 * NI;
#pragma unroll
            for (int d = 0; d < DX; ++d) xw[lane * NI + d] = x[d] * K[kRp + d];
            xw[lane * NI + DX] = PSVO_ARG(BwdArgs, lam2_all)[(row() * N + n) * M + m];
            xw[lane * NI + DX + 1] = dlam;            // (0 for the lanes of a chain past N: aw = 0)
            __builtin_amdgcn_wave_barrier();
            const int g16 = lane & ~15, j16 = lane & 15;
            int own = j16;      // (opaque: the lane masks own == i and lane < 16 would otherwise be kept in SGPR pairs across the time loop)
            asm volatile("" : "+v"(own));
            float ix[16][DX], il[16], idl[16], ixa[16][DX];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    ix[i][d] = xw[(g16 + i) * NI + d];
                    ixa[i][d] = 0.f;
                }
                il[i] = xw[(g16 + i) * NI + DX];
                idl[i] = xw[(g16 + i) * NI + DX + 1];
            }
            float sfl[DX];        // sum over the lane's pairs of c (z^2 - 1): d sigma_f of the filter term, times sigma_f
#pragma unroll
            for (int d = 0; d < DX; ++d) sfl[d] = 0.f;
            float* const ja_w = jacc + wave * NA * NP;
            for (int jt = 0; jt < NP; jt += 16) {
                const int j = jt + j16;
                const float* p = tile + j * TS;
                float Fp[DX];
#pragma unroll
                for (int d = 0; d < DX; ++d) Fp[d] = p[d];
                const float Wp = p[DX];
                float ja[NA];
#pragma unroll
                for (int q = 0; q < NA; ++q) ja[q] = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float e2 = Wp, u[DX];
#pragma unroll
                    for (int d = 0; d < DX; ++d) {
                        u[d] = ix[i][d] - Fp[d];                    // (x~ - F_j) kappa / sigma
                        e2 = fmaf(-u[d], u[d], e2);
                    }
                    const float cj = idl[i] * exp2_fast(e2 - il[i]);    // d lam_i * p_ij
#pragma unroll
                    for (int d = 0; d < DX; ++d) {
                        const float g1 = cj * u[d];
                        ixa[i][d] += g1;
                        ja[d] += g1;
                        sfl[d] += cj * fmaf(u[d] * u[d], 2.f * kLn2, -1.f);
                    }
                    ja[DX] += cj;
                }
#pragma unroll
                for (int q = 0; q < NA; ++q) {      // over the four rows; lanes 0..15 hold (and store) the wave's sum
                    float v = ja[q];
                    v += xor_lane<16>(v);
                    v += xor_lane<32>(v);
                    if (lane == own) ja_w[q * NP + j] = v;      // (lanes 0 .. 15)
                }
            }
            // item sums over the row's 16 lanes; item i of the row is owned by the row's lane i, which keeps the sum
            float mine[DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) mine[d] = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    float v = ixa[i][d];
                    v += dpp_mov<0x128, 0xF, 0xF, true>(v, v);   // row_ror:8
                    v += dpp_mov<0x124, 0xF, 0xF, true>(v, v);   // row_ror:4
                    v += dpp_mov<0x122, 0xF, 0xF, true>(v, v);   // row_ror:2
                    v += dpp_mov<0x121, 0xF, 0xF, true>(v, v);   // row_ror:1
                    mine[d] = (own == i) ? v : mine[d];
                }
            }
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                dx[d] -= mine[d] * K[kIsfk + d];                // (x~ - F) / sigma^2 = u / (sigma kappa)
                acc[AC::kSf + d] += sfl[d] * K[kIsf + d];
            }
        } else {
#pragma unroll
            for (int d = 0; d < DX; ++d) {      // t = 0: lam_m = log N(x~; imean, isig)
                const float iis = K[kIisig + d];
                const float z = (x[d] - K[kIm + d]) * iis;
                const float tz = dphi * z * iis;
                dx[d] -= tz;
                dim_part[d] = tz;
                acc[AC::kSiota + d] += dphi * (z * z - 1.f) * iis;
            }
        }

        // ---- reduce over the chain's M sub-particles; x~ = mu + c eps, -q contributes + sum log c ----------------------------
        float dmu[DX], sce[DX], dxp[DX], dim[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            dmu[d] = group_sum<M>(dx[d]);
            sce[d] = group_sum<M>(dx[d] * eps[d]);
            dxp[d] = group_sum<M>(dxp_part[d]);
            dim[d] = group_sum<M>(dim_part[d]);
        }
        // (the lead lane's sums are selects, not an `if`: see bsim_bwd_impl.h on divergent regions in front of an MLP pass)
        float dmu1[DX], outv[DX];
        if (!last) {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                dmu1[d] = dmu[d] * K[kPc + d] * K[kPi1 + d];
                outv[d] = dmu[d] * K[kPc + d] * K[kPi2 + d];
                acc[AC::kSc + d] += lead ? sce[d] + aw * K[kPic + d] : 0.f;   // -sum_m dq_m / c = a / c
                acc[AC::kSmm1 + d] += lead ? dmu[d] * mu1[d] : 0.f;
                acc[AC::kSmb + d] += lead ? dmu[d] * bm[d] : 0.f;
                acc[AC::kSmm + d] += lead ? dmu[d] * mu[d] : 0.f;
            }
            float dq[DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) dq[d] = 0.f;
            MQ::template bwd_input<true>(wqi, xp, dmu1, dq);         // (the same in the chain's M lanes)
#pragma unroll
            for (int d = 0; d < DX; ++d) dxp[d] += dq[d];
        } else {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                outv[d] = dmu[d];
                dmu1[d] = 0.f;
                acc[AC::kSinit + d] += lead ? sce[d] + aw * K[kIsinit + d] : 0.f;
            }
        }
#pragma unroll
        for (int d = 0; d < DX; ++d) dX[d] = dxp[d];
        if (lead) {
            float* dmu1_o = PSVO_ARG(BwdArgs, dmu1);
            float* dbmu2_rows = PSVO_ARG(BwdArgs, dbmu2_rows);
            const size_t tb = row();
            const int Nn = width();
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                dmu1_o[(tb * DX + d) * Nn + n] = dmu1[d];
                dbmu2_rows[(tb * DX + d) * Nn + n] = last ? 0.f : outv[d];
                if (last) PSVO_ARG(BwdArgs, dminit_rows)[((size_t)b * DX + d) * Nn + n] = outv[d];
                if (first) PSVO_ARG(BwdArgs, dimean_rows)[((size_t)b * DX + d) * Nn + n] = dim[d];
            }
        }
        __syncthreads();      // every wave's copy of the per-j sums is complete; the tile and ybuf[t & 1] are free

        // ---- the workgroup's partials of d Fm / d logW of forward step t - 1: wave copies added in wave order -----------------
        if (!first) {
            float* dFm_part = PSVO_ARG(BwdArgs, dFm_part);
            float* dlogW_part = PSVO_ARG(BwdArgs, dlogW_part);
            const size_t pbk = (row() - B) * nblk + blk;
            for (int i = tid; i < NA * N; i += NTB) {
                const int d = i / N, j = i - d * N;
                float s = 0.f;
                for (int w = 0; w < nwv; ++w) s += jacc[(w * NA + d) * NP + j];
                if (d < DX) dFm_part[(pbk * DX + d) * N + j] = s * K[kIsfk + d];    // d F = d F' rho, and the 1 / (sigma kappa) factor
                else dlogW_part[pbk * N + j] = s;
            }
        }
        if (last) {           // nothing follows forward step T - 1
            float* dFm_part = PSVO_ARG(BwdArgs, dFm_part);
            float* dlogW_part = PSVO_ARG(BwdArgs, dlogW_part);
            const size_t pbk = row() * nblk + blk;
            for (int i = tid; i < NA * N; i += NTB) {
                const int d = i / N, j = i - d * N;
                if (d < DX) dFm_part[(pbk * DX + d) * N + j] = 0.f;
                else dlogW_part[pbk * N + j] = 0.f;
            }
        }
        // the next step's observation row, once per workgroup: it lands in the half of ybuf that step t - 1 read, beside the
        // global loads of the next tile and ahead of the barrier that publishes both
        if (!last && tid < Dy) ybuf[((t + 1) & 1) * kMaxDy + tid] = PSVO_ARG(BwdArgs, obs)[(row() + B) * Dy + tid];
    }

    // ---- per-workgroup scale sums: lanes by the DPP scan, waves in wave order; d sig_g columns in lane order --------------------
    __syncthreads();
    float* dst = PSVO_ARG(BwdArgs, sacc_part) + ((size_t)b * nblk + blk) * NACC;
#pragma unroll
    for (int i = 0; i < 7 * DX; ++i) {
        const float s = block_sum(acc[i], red, wave, lane, nwv);
        if (tid == 0) dst[i] = s;
    }
    __syncthreads();
    if (tid < Dy) {      // (count emission: no scale, zeros)
        float s = 0.f;
        if constexpr (!CNT) {
            for (int i = 0; i < NTB; ++i) s += sg[tid * NTB + i];
        }
        dst[AC::kSg + tid] = s;
    }
}

template <int DX, int H>
static size_t bwd_lds_bytes(int N, int NTB, int Dy) {
    const int NP = (N + 15) & ~15, nwv = NTB / 64;
    return sizeof(float) * (2 * MlpLds<DX, H, DX, 1>::kSize + GLds<DX, H>::kSize + 3 * kMaxDy + 16 + (size_t)NP * (DX + 1) +
                            (size_t)nwv * (DX + 1) * NP + 4 * 64 * (DX + 2) + (size_t)Dy * NTB + 12 * DX);
}

struct BwdOut {
    float *dFm, *dlogW, *dlse, *dsig_f, *dsig_g, *dsig_q1inv, *dsig_bq2, *dsig_init, *disig;
};

template <int DX, int H, int M>
static int launch_bwd(const BwdArgs& a, const BwdOut& o, hipStream_t stream) {
    const Geom ge = geometry(a.N, M);
    const size_t lds = bwd_lds_bytes<DX, H>(a.N, ge.ntb, a.Dy);
    if (lds > 160 * 1024) return PSVO_ERR_UNSUPPORTED;
    clear_hip_error();
    if (a.emission == 2) hipLaunchKernelGGL((bsim_wobs_bwd_kernel<DX, H, M, true>), dim3(ge.nblk, a.B), dim3(ge.ntb), lds, stream, a);
    else hipLaunchKernelGGL((bsim_wobs_bwd_kernel<DX, H, M, false>), dim3(ge.nblk, a.B), dim3(ge.ntb), lds, stream, a);
    // (DX is a template value inside the envelope: the status can only be PSVO_OK)
    (void)launch_bsim_bwd_fold_finalize(DX, {a.dFm_part, a.dlogW_part, a.T, a.B, ge.nblk, a.N, a.Dy, o.dFm, o.dlogW, o.dlse, a.sacc_part,
                                       a.B * ge.nblk, a.sig_q1inv, a.sig_bq2, o.dsig_f, o.dsig_g, o.dsig_q1inv, o.dsig_bq2,
                                       o.dsig_init, o.disig}, stream);
    return launch_status();
}

// the envelope of both entry points (host only); T >= 2 as for psvo_bsim_forward
static int check_shape(const psvo_desc* d) {
    if (d->B <= 0 || d->T < 2 || d->N <= 0) return PSVO_ERR_INVALID;
    const bool dx = d->Dx >= 2 && d->Dx <= 4, h = d->H == 16 || d->H == 32 || d->H == 64;
    const bool m = d->M == 4 || d->M == 8 || d->M == 16 || d->M == 32;
    if (d->Dy < PSVO_WBS_MIN_DY || d->Dy > kMaxDy || !dx || !h || !m || d->N > 512 || d->B > 65535 || d->layers < 0 || d->layers > 1)
        return PSVO_ERR_UNSUPPORTED;
    return PSVO_OK;
}

template <class F>
static int dispatch(const psvo_desc* d, F&& f) {
    return pick_dx(d->Dx, [&](auto dx) {
        return pick_h(d->H, [&](auto h) { return pick_m(d->M, [&](auto m) { return f(dx, h, m); }); });
    });
}

struct WsLayout {
    size_t dFm_part, dlogW_part, sacc;
};
static WsLayout ws_layout(int B, int T, int N, int M, int Dx, int Dy) {
    const size_t nblk = geometry(N, M).nblk;
    return {(size_t)T * B * nblk * Dx * N, (size_t)T * B * nblk * N, (size_t)B * nblk * (7 * Dx + Dy)};
}

}  // namespace PSVO_WBS (wbs, or wbs_ms)
}  // namespace psvo

#if !PSVO_MS     // (the geometry and the workspace are those of the static pair: one definition, in its unit)
extern "C" int psvo_bsim_wobs_blocks(int N, int M) {
    if (N <= 0 || M <= 0) return 0;
    return psvo::PSVO_WBS::geometry(N, M).nblk;
}

extern "C" long long psvo_bsim_wobs_ws_floats(int B, int T, int N, int M, int Dx, int Dy) {
    if (B <= 0 || T <= 0 || N <= 0 || M <= 0 || Dx <= 0 || Dy <= 0) return 0;
    const psvo::PSVO_WBS::WsLayout l = psvo::PSVO_WBS::ws_layout(B, T, N, M, Dx, Dy);
    return (long long)(l.dFm_part + l.dlogW_part + l.sacc);
}
#endif

extern "C" int PSVO_WBS_ENTRY(psvo_bsim_forward_wobs)(const psvo_desc* desc, const float* X, const float* Fm, const float* logW,
                                      const float* lse, const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                                      const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
                                      const float* bmu2, const float* minit, const float* sig_init, const float* imean,
                                      const float* isig, const float* obs, const float* eps_b, const float* u_b,
                                      const int32_t* sel_in, float* bwX, float* flp, float* glp, float* Omega,
                                      int32_t* sel_out, float* score, float* lam2_all, float* om_all, float* mu1_all,
                                      void* stream) {
    using namespace psvo;
    using namespace psvo::PSVO_WBS;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!desc || !Fm || !logW || !lse || !f || !g || !q1_inv || !sig_f || !sig_g || !sig_q1inv || !sig_bq2 || !bmu2 ||
        !minit || !sig_init || !imean || !isig || !obs || !eps_b || !bwX || !flp || !glp || !Omega || !sel_out || !score)
        return PSVO_ERR_INVALID;
    if (!u_b && !sel_in) return PSVO_ERR_INVALID;
    const int st = check_shape(desc);
    if (st != PSVO_OK) return st;
    (void)X;

    FwdArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy; a.emission = desc->emission;
    a.f = *f; a.g = *g; a.q1inv = *q1_inv;
    a.Fm = Fm; a.logW = logW; a.lse = lse;
    a.sig_f = sig_f; a.sig_g = sig_g; a.sig_q1inv = sig_q1inv; a.sig_bq2 = sig_bq2;
    a.bmu2 = bmu2; a.minit = minit; a.sig_init = sig_init; a.imean = imean; a.isig = isig;
    a.obs = obs; a.eps_b = eps_b; a.u_b = u_b; a.sel_in = sel_in;
    a.bwX = bwX; a.flp = flp; a.glp = glp; a.Omega = Omega; a.sel_out = sel_out; a.score = score;
    a.lam2_all = lam2_all; a.om_all = om_all; a.mu1_all = mu1_all;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch(desc, [&](auto dx, auto h, auto m) { return launch_fwd<dx(), h(), m()>(a, s); });
}

extern "C" int PSVO_WBS_ENTRY(psvo_bsim_backward_wobs)(
    const psvo_desc* desc, const float* Fm, const float* logW, const float* lse, const psvo_mlp* f, const psvo_mlp* g,
    const psvo_mlp* q1_inv, const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
    const float* bmu2, const float* minit, const float* sig_init, const float* imean, const float* isig, const float* obs,
    const float* eps_b, const float* bwX, const int32_t* sel, const float* lam2_all, const float* om_all,
    const float* mu1_all, const float* dscore, float* xt, float* dFt, float* dGt, float* dmu1, float* dbmu2_rows,
    float* dminit_rows, float* dimean_rows, float* dFm, float* dlogW, float* dlse, float* dsig_f, float* dsig_g,
    float* dsig_q1inv, float* dsig_bq2, float* dsig_init, float* disig, float* ws, void* stream) {
    using namespace psvo;
    using namespace psvo::PSVO_WBS;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!desc || !Fm || !logW || !lse || !f || !g || !q1_inv || !sig_f || !sig_g || !sig_q1inv || !sig_bq2 || !bmu2 ||
        !minit || !sig_init || !imean || !isig || !obs || !eps_b || !bwX || !sel || !lam2_all || !om_all || !mu1_all ||
        !dscore || !xt || !dFt || !dGt || !dmu1 || !dbmu2_rows || !dminit_rows || !dimean_rows || !dFm || !dlogW || !dlse ||
        !dsig_f || !dsig_g || !dsig_q1inv || !dsig_bq2 || !dsig_init || !disig || !ws)
        return PSVO_ERR_INVALID;
    const int st = check_shape(desc);
    if (st != PSVO_OK) return st;

    BwdArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy; a.emission = desc->emission;
    a.f = *f; a.g = *g; a.q1inv = *q1_inv;
    a.Fm = Fm; a.logW = logW; a.lse = lse;
    a.sig_f = sig_f; a.sig_g = sig_g; a.sig_q1inv = sig_q1inv; a.sig_bq2 = sig_bq2;
    a.bmu2 = bmu2; a.minit = minit; a.sig_init = sig_init; a.imean = imean; a.isig = isig;
    a.obs = obs; a.eps_b = eps_b; a.bwX = bwX; a.sel = sel;
    a.lam2_all = lam2_all; a.om_all = om_all; a.mu1_all = mu1_all; a.dscore = dscore;
    a.xt = xt; a.dFt = dFt; a.dGt = dGt; a.dmu1 = dmu1;
    a.dbmu2_rows = dbmu2_rows; a.dminit_rows = dminit_rows; a.dimean_rows = dimean_rows;
    const WsLayout l = ws_layout(desc->B, desc->T, desc->N, desc->M, desc->Dx, desc->Dy);
    a.dFm_part = ws; a.dlogW_part = ws + l.dFm_part; a.sacc_part = a.dlogW_part + l.dlogW_part;
    BwdOut o{dFm, dlogW, dlse, dsig_f, dsig_g, dsig_q1inv, dsig_bq2, dsig_init, disig};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch(desc, [&](auto dx, auto h, auto m) { return launch_bwd<dx(), h(), m()>(a, o, s); });
}
