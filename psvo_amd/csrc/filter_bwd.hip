// Reverse-mode pass of the forward particle filter (gradient of anything computed from the
// filter's logW / lse / Fm outputs w.r.t. its inputs).  The reference gets this from TensorFlow
// autodiff through tf.while_loop (reference src/trainer.py:115-118, no stop_gradient anywhere,
// SURVEY.md Appendix B); here it is one persistent workgroup per sequence walking t = T-1 .. 0.
//
// What flows (Appendix B): samples are reparameterised (x = mu + c*eps), ancestor indices are
// constants, the gather of resampled particles back-propagates as a scatter-add into the
// pre-resampling particles.  In this formulation a resampled particle only enters step t+1
// through the gathered MLP outputs P1_t[a] (proposal mean) and Fm_t[a] (transition mean), so the
// scatter-add targets are d P1_t / d Fm_t, kept in LDS (float atomics), double-buffered over t.
//
// Nothing is stored by the forward pass beyond its own outputs; hidden activations are
// recomputed.  MLP *weight* gradients are not formed here: the kernel writes, for every MLP
// evaluation, the gradient w.r.t. that evaluation's output (rows dP, dF, dG) and psvo_mlp_wgrad
// reduces rows to weights in a fully parallel launch.
#include "common.h"

namespace psvo {
extern int g_tune_deterministic;   // PSVO_TUNE_DETERMINISTIC (psvo_set_tuning, bsim_bwd.hip)
inline namespace PSVO_LNS {   // l1 / l2: hidden layers of the per-particle MLPs (common.h)
PSVO_TIMERS_DEFINE(filter_bwd)


struct FilterBwdArgs {
    int B, T, N;
    int resample, two_q, bootstrap, emission;
    psvo_mlp q1, f, g;
    const float *sig_q1, *sig_q2, *sig_f, *sig_g;
    const float *mu2, *m0, *sig0, *fm0, *fsig0, *obs, *eps;
    const float *X, *Fm, *P1, *logW, *lse;
    const int32_t* idx;
    const float* dlse;       // (T,B) or null
    int nparts;              // leading "parts" dimension of the external gradients (bsim blocks per sequence)
    const float* dFm_ext;    // (T,B,nparts,Dx,N) or null
    const float* dlogW_ext;  // (T,B,nparts,N) or null
    float *dP, *dF, *dG, *dmu2, *dm0, *dfm0;
    float* sacc;             // (B, NACC) per-sequence scalar accumulators (see finalize)
    float* dm2_rows;         // (T,B,Dx,N) per-particle d mu2 rows, summed over N by row_sum_kernel (api.hip) afterwards
    int wave_copies;         // filter_bwd_kernel: one scatter-target copy per wave (set by the launcher when LDS has room)
    float* scanAB;           // affine-scan path: (T,B,N,REC) records (16-byte aligned); part: (T,B,NACC) per-step partial sums
    float* scanPart;
    int det_copies;          // filter_bwd_kernel<.., DET = true>: scatter-target copies, 1 .. waves (see there)
};

// Adaptive resampling (psvo_filter_backward_adaptive): the static arguments plus the forward pass's decisions rs (T,B), 1 =
// the sequence resampled at that step.  A type of its own, so that the static kernels keep their argument block.
struct FilterBwdArgsAd : FilterBwdArgs {
    const int32_t* rs;
};
template <bool AD>
using FilterBwdArgsT = std::conditional_t<AD, FilterBwdArgsAd, FilterBwdArgs>;
// a decision word read through the constant address space (uniform address: a scalar load)
typedef const __attribute__((address_space(4))) int32_t rs_word_t;

// floats of one affine-scan record (ScanRec<DX>::REC): A (Dx x Dx) | b (Dx) | ext (Dx) | ancestor, padded to float4s
constexpr int scan_rec_floats(int Dx) { return (Dx * Dx + 2 * Dx + 1 + 3) & ~3; }

// The reverse pass's workspace (psvo_filter_ws_floats), offsets and size in floats: per-sequence sums (at 0) | d mu2 rows |
// (16-byte aligned) affine-scan records (T,B,N,REC) | per-step partial sums (T,B,NACC).  The size allows 4 floats for the alignment.
struct FilterWsLayout {
    long long dm2, rec, part, total;
};
static FilterWsLayout filter_ws_layout(int B, int T, int N, int Dx, int Dy) {
    const long long nacc = psvo_filter_acc_size(Dx, Dy), sums = B * nacc, rows = (long long)T * B * Dx * N;
    const long long recs = (long long)T * B * scan_rec_floats(Dx) * N, end = sums + rows, rec = (end + 3) & ~3LL;
    return {sums, rec, rec + recs, end + 4 + recs + (long long)T * B * nacc};
}

// the persistent kernels (filter_bwd_impl.h): the static pair, then the adaptive pair
#define PSVO_AD 0
#include "filter_bwd_impl.h"
#undef PSVO_AD
#define PSVO_AD 1
#include "filter_bwd_impl.h"
#undef PSVO_AD

#if PSVO_L == 1
// ---------------------------------------------------------------------------------------------
// The reverse filter as an AFFINE SCAN (round 3; bootstrap wiring with resampling, one hidden layer).
//
// With resampling the gradient w.r.t. logW_t[n] does not depend on later steps, and the only thing the reverse pass carries
// from step t+1 to step t is D_t[n] = d loss / d MLP_q1(x_t[n]) (Dx values per particle): the children of particle n scatter
//     kappa (dx0_c + J_c^T D_{t+1}[c]) + tf_c        into D_t[n]   (c: particles of step t+1 with ancestor n)
// where J_c = d MLP_q1 / d x at x_{t+1}[c], dx0_c and tf_c the parts of the step that do not depend on D, kappa = c / s1 the
// product-of-Gaussians factor.  The recurrence is AFFINE in D:  D_t[n] = ext_t[n] + sum_c (A_c D_{t+1}[c] + b_c)  with a
// Dx x Dx matrix A_c = diag(kappa) J_c^T and a vector b_c per particle and step.  So the time loop splits into
//   A. fbs_coeff_kernel : A and b of EVERY (t, b, n) -- the MLP_g forward + input gradient, the densities and Dx input-gradient
//      passes of MLP_q1 on unit vectors -- one workgroup per (t, sequence): T B workgroups on all CUs, no dependence between them;
//   B. fbs_scan_kernel  : ONE WAVE per sequence walks t = T-1 .. 0 doing nothing but D <- ext + scatter(A D + b): a Dx x Dx
//      matrix-vector product and Dx LDS adds per particle and step, no MLP, no barrier (a single wave: LDS operations are in
//      order), coefficients requested a step ahead; it writes the rows D_t[n] (= the dP rows of psvo_mlp_wgrad);
//   C. fbs_rows_kernel  : everything else the persistent kernel produces, from D -- dG rows, d mu2 rows, the scale sums, d m0 --
//      again one workgroup per (t, sequence).
// The persistent kernel spends 7 800 cycles per step on ONE workgroup per sequence (32 of 256 CUs at C*, 8 at C5) and only a
// quarter of that is MLP arithmetic; here the serial part is ~10 instructions per particle and step.
// Sums are fixed-order (per-step partials folded over t by step_fold_kernel; LDS adds of one wave are applied in lane order).
// ---------------------------------------------------------------------------------------------
// One record per (t, sequence, particle), stored as float4 planes [(t, sequence), float4 index, particle] so that the scan reads it
// with 16-byte loads that are contiguous over the lanes:
//   [ A (Dx x Dx, row-major) | b (Dx) | ext (Dx) = the upstream gradient w.r.t. Fm_t[n] | ancestor (int bits) ], padded to float4s.
// (The first layout was (T,B,coefficient,N) read with one dword load per value: 25 loads per particle and step at Dx = 4 --
//  a wave can have 64 vector-memory operations outstanding, so the scan ran ONE step ahead whatever its ring depth.)
template <int DX>
struct ScanRec {
    static constexpr int NC = DX * DX + DX;
    static constexpr int kExt = NC, kAnc = NC + DX;
    static constexpr int REC = scan_rec_floats(DX);
};

template <int DX, int DY, int H>
__global__ void __launch_bounds__(512) fbs_coeff_kernel(const FilterBwdArgs a) {
    using MQ = MlpLds<DX, H, DX, 1>;
    using MG = MlpLds<DX, H, DY, 1>;
    using SR = ScanRec<DX>;
    constexpr bool kRolled = true;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, NT = blockDim.x;
    const int t = blockIdx.x, b = blockIdx.y, B = a.B, N = a.N;
    const bool valid = tid < N;
    const int n = valid ? tid : N - 1;
    const size_t tb = (size_t)t * B + b;
    float rec[SR::REC];
#pragma unroll
    for (int i = 0; i < SR::REC; ++i) rec[i] = 0.f;
#pragma unroll
    for (int d = 0; d < DX; ++d) rec[SR::kExt + d] = a.dFm_ext ? a.dFm_ext[(tb * DX + d) * N + n] : 0.f;
    if (t >= 1) {       // (t = 0 has no parent: only the upstream gradient)
        float* wq1 = smem;
        float* wg = wq1 + MQ::kSize;
        MQ::load(wq1, a.q1, tid, NT);
        MG::load(wg, a.g, tid, NT);
        float x[DX], fmean[DX], y[DY];
        const int anc = a.idx[(tb - B) * N + n];
        rec[SR::kAnc] = __int_as_float(anc);
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            x[d] = a.X[(tb * DX + d) * N + n];
            fmean[d] = a.Fm[((tb - B) * DX + d) * N + anc];
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) y[k] = a.obs[tb * DY + k];
        const float sm = exp2_fast((a.logW[tb * N + n] - a.lse[tb]) * kLog2e);
        const float dlw = (a.dlse ? a.dlse[tb] : 0.f) * sm + (a.dlogW_ext ? a.dlogW_ext[tb * N + n] : 0.f);
        float kap[DX], ifs[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float i1 = 1.f / a.sig_q1[d];
            kap[d] = a.two_q ? i1 / (i1 + 1.f / a.sig_q2[d]) : 1.f;     // c / s1
            ifs[d] = i1;                                                // bootstrap: the transition scale is sigma_q1
        }
        __syncthreads();
        float dxg[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) dxg[d] = 0.f;
        {
            float gm[DY], dgm[DY];
            MG::template eval<kRolled>(wg, x, gm);
#pragma unroll
            for (int k = 0; k < DY; ++k) {
                float dmean = 1.f;
                if (a.emission) { dmean = emis_dmean(gm[k]); gm[k] = emis_mean(gm[k]); }
                const float isg = 1.f / a.sig_g[k];
                dgm[k] = dlw * (y[k] - gm[k]) * isg * isg * dmean;
            }
            MG::template bwd_input<kRolled>(wg, x, dgm, dxg);
        }
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float tf = dlw * (x[d] - fmean[d]) * ifs[d] * ifs[d];
            rec[DX * DX + d] = fmaf(kap[d], dxg[d] - tf, tf);
        }
#pragma unroll
        for (int k = 0; k < DX; ++k) {
            float ek[DX], col[DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) { ek[d] = (d == k) ? 1.f : 0.f; col[d] = 0.f; }
            MQ::template bwd_input<kRolled>(wq1, x, ek, col);          // J^T e_k
#pragma unroll
            for (int d = 0; d < DX; ++d) rec[d * DX + k] = kap[d] * col[d];
        }
    }
    if (valid) {
        // float4 i of the record at [(tb R4 + i) N + n]: a wave's accesses are 16 bytes per lane AND contiguous over the lanes
        // (particle-major records -- 112 bytes apart at Dx = 4 -- cost 64 cache lines per access: C5 67.0 -> 69.1 ms)
        float4* dst = reinterpret_cast<float4*>(a.scanAB) + (tb * (SR::REC / 4)) * N + n;
#pragma unroll
        for (int i = 0; i < SR::REC / 4; ++i) dst[(size_t)i * N] = make_float4(rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]);
    }
}

// NWV waves per sequence (1: no barrier at all -- LDS operations of one wave are in order; 4: one barrier per step), PPL particles
// per lane (N <= 64 NWV PPL), DEPTH steps of coefficients in flight: a step takes ~0.2 us and HBM ~2 us, so the loads of step
// t - DEPTH are issued when step t is consumed (a ring of DEPTH register sets, the step loop unrolled DEPTH times so that every
// index into it is static).
template <int DX, int NWV, int PPL, int DEPTH, int NCP = NWV>
__global__ void __launch_bounds__(64 * NWV) fbs_scan_kernel(const FilterBwdArgs a) {
    using SR = ScanRec<DX>;
    constexpr int NTS = 64 * NWV, R4 = SR::REC / 4;
    // NCP = NWV: one scatter copy per wave (fixed summation order; the launcher's choice at every N).  NCP = 1: one shared copy
    // and LDS float atomics across the waves -- measured at C5 (N = 512, Dx = 4): 68.4 against 68.3 ms, the copies are not what
    // the step waits for
    // scatter targets: one copy per wave, summed by the parent in wave order (LDS adds of ONE wave are applied in lane order,
    // adds of several waves in arrival order: with the copies every sum has a fixed order, as in filter_bwd_lpp_kernel)
    extern __shared__ __attribute__((aligned(16))) float acc[];      // [2][NWV][DX][N]
    const int tid = threadIdx.x, b = blockIdx.x, B = a.B, T = a.T, N = a.N;
    const int CPY = DX * N, mine = (NCP > 1 ? (tid >> 6) : 0) * CPY;
    for (int i = tid; i < 2 * NCP * CPY; i += NTS) acc[i] = 0.f;
    float4 rec[DEPTH][PPL][R4];
    auto load = [&](int t, float4 (&r)[PPL][R4]) {
        const size_t tb = (size_t)t * B + b;
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
            const int n = min(tid + NTS * p, N - 1);
            const float4* src = reinterpret_cast<const float4*>(a.scanAB) + (tb * R4) * N + n;
#pragma unroll
            for (int i = 0; i < R4; ++i) r[p][i] = src[(size_t)i * N];
        }
    };
#pragma unroll
    for (int s = 0; s < DEPTH; ++s)
        if (T - 1 - s >= 0) load(T - 1 - s, rec[s]);
    if (NWV > 1) __syncthreads();
    for (int t0 = T - 1; t0 >= 0; t0 -= DEPTH) {
#pragma unroll
        for (int s = 0; s < DEPTH; ++s) {
            const int t = t0 - s;
            if (t < 0) break;
            const size_t tb = (size_t)t * B + b;
            float* cur = acc + (t & 1) * NCP * CPY;
            float* nxt = acc + ((t + 1) & 1) * NCP * CPY + mine;
            float D[PPL][DX];
            float cf[PPL][SR::REC];
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
#pragma unroll
                for (int i = 0; i < R4; ++i) {
                    cf[p][4 * i] = rec[s][p][i].x; cf[p][4 * i + 1] = rec[s][p][i].y;
                    cf[p][4 * i + 2] = rec[s][p][i].z; cf[p][4 * i + 3] = rec[s][p][i].w;
                }
            }
            if (t - DEPTH >= 0) load(t - DEPTH, rec[s]);      // refill the slot just consumed
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
                const int n = tid + NTS * p;
                if (n < N) {
#pragma unroll
                    for (int d = 0; d < DX; ++d) {
                        float v = 0.f;
#pragma unroll
                        for (int w = 0; w < NCP; ++w) {
                            v += cur[w * CPY + d * N + n];
                            cur[w * CPY + d * N + n] = 0.f;
                        }
                        D[p][d] = v + cf[p][SR::kExt + d];
                        a.dP[(tb * DX + d) * N + n] = D[p][d];
                    }
                }
            }
            if (t >= 1) {
#pragma unroll
                for (int p = 0; p < PPL; ++p) {
                    const int n = tid + NTS * p;
                    if (n < N) {
                        const int an = __float_as_int(cf[p][SR::kAnc]);
#pragma unroll
                        for (int d = 0; d < DX; ++d) {
                            float v = cf[p][DX * DX + d];
#pragma unroll
                            for (int k = 0; k < DX; ++k) v = fmaf(cf[p][d * DX + k], D[p][k], v);
                            atomicAdd(&nxt[d * N + an], v);
                        }
                    }
                }
            }
            if (NWV > 1) {
                // a workgroup barrier that orders the LDS traffic of the step ONLY: __syncthreads() also waits for every
                // outstanding global access (s_waitcnt vmcnt(0)), i.e. for the record loads just issued for DEPTH steps ahead
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            } else {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
    }
}

template <int DX, int DY, int H>
__global__ void __launch_bounds__(512) fbs_rows_kernel(const FilterBwdArgs a) {
    using MQ = MlpLds<DX, H, DX, 1>;
    using MG = MlpLds<DX, H, DY, 1>;
    using AC = FAcc<DX>;
    constexpr int kN = AC::kSg + DY;
    constexpr bool kRolled = true;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = blockDim.x, nw = NT >> 6;
    const int t = blockIdx.x, b = blockIdx.y, B = a.B, N = a.N;
    const bool valid = tid < N, first = (t == 0);
    const int n = valid ? tid : N - 1;
    float* wq1 = smem;
    float* wg = wq1 + MQ::kSize;
    float* red = wg + MG::kSize;     // [nw][kN] + 16
    MQ::load(wq1, a.q1, tid, NT);
    MG::load(wg, a.g, tid, NT);
    const size_t tb = (size_t)t * B + b;
    float s1[DX], s2[DX], fs[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        s1[d] = first ? a.sig0[d] : a.sig_q1[d];
        s2[d] = a.two_q ? a.sig_q2[d] : 1.f;
        fs[d] = first ? a.fsig0[d] : a.sig_q1[d];
    }
    const StepKR<DX> K = make_stepkr<DX>(s1, s2, fs, a.two_q != 0);
    float x[DX], e[DX], m2[DX], y[DY], mean1[DX], fmean[DX], dPn[DX];
    const int anc = first ? n : a.idx[(tb - B) * N + n];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        x[d] = a.X[(tb * DX + d) * N + n];
        e[d] = a.eps[(tb * DX + d) * N + n];
        m2[d] = a.two_q ? a.mu2[tb * DX + d] : 0.f;
        fmean[d] = first ? a.fm0[b * DX + d] : a.Fm[((tb - B) * DX + d) * N + anc];
        mean1[d] = first ? a.m0[b * DX + d] : fmean[d];
        dPn[d] = valid ? a.dP[(tb * DX + d) * N + n] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < DY; ++k) y[k] = a.obs[tb * DY + k];
    const float sm = valid ? exp2_fast((a.logW[tb * N + n] - a.lse[tb]) * kLog2e) : 0.f;
    float dlw = (a.dlse ? a.dlse[tb] : 0.f) * sm + (a.dlogW_ext ? a.dlogW_ext[tb * N + n] : 0.f);
    if (!valid) dlw = 0.f;
    float mu[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) mu[d] = a.two_q ? K.c[d] * fmaf(K.i1[d], mean1[d], K.i2[d] * m2[d]) : mean1[d];
    __syncthreads();

    float acc[kN];
#pragma unroll
    for (int i = 0; i < kN; ++i) acc[i] = 0.f;
    float inc[AC::kSet];
#pragma unroll
    for (int i = 0; i < AC::kSet; ++i) inc[i] = 0.f;
    float dx[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) dx[d] = 0.f;
    {
        float gm[DY], dgm[DY];
        MG::template eval<kRolled>(wg, x, gm);
#pragma unroll
        for (int k = 0; k < DY; ++k) {
            float dmean = 1.f;
            if (a.emission) { dmean = emis_dmean(gm[k]); gm[k] = emis_mean(gm[k]); }
            const float isg = 1.f / a.sig_g[k];
            const float z = (y[k] - gm[k]) * isg;
            dgm[k] = dlw * z * isg * dmean;
            acc[AC::kSg + k] += dlw * (z * z - 1.f) * isg;
            if (valid) a.dG[(tb * DY + k) * N + n] = dgm[k];
        }
        MG::template bwd_input<kRolled>(wg, x, dgm, dx);
    }
    float dfmean[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        const float z = (x[d] - fmean[d]) * K.ifs[d];
        const float tf = dlw * z * K.ifs[d];
        dx[d] -= tf;
        dfmean[d] = tf;
        inc[AC::kSfs + d] += dlw * (z * z - 1.f) * K.ifs[d];
        inc[AC::kSc + d] += dlw * K.ic[d];
    }
    MQ::template bwd_input<kRolled>(wq1, x, dPn, dx);
    float dmean1[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        const float dmu = dx[d];
        inc[AC::kSc + d] += dmu * e[d];
        if (a.two_q) {
            dmean1[d] = dmu * K.c[d] * K.i1[d];
            inc[AC::kSmm1 + d] += dmu * mean1[d];
            inc[AC::kSmb + d] += dmu * m2[d];
            inc[AC::kSmm + d] += dmu * mu[d];
            if (valid) a.dm2_rows[(tb * DX + d) * N + n] = dmu * K.c[d] * K.i2[d];
        } else {
            dmean1[d] = dmu;
        }
    }
#pragma unroll
    for (int i = 0; i < AC::kSet; ++i) acc[(first ? 0 : AC::kSet) + i] = inc[i];
    // ---- this step's partial of the per-sequence sums (fixed order: lanes, then waves) ----------------------------------
#pragma unroll
    for (int i = 0; i < kN; ++i) {
        const float v = wave_sum(acc[i]);
        if (lane == 0) red[wave * kN + i] = v;
    }
    if (first) {
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float v1 = wave_sum(dmean1[d]), v2 = wave_sum(dfmean[d]);
            if (lane == 0) {
                red[nw * kN + wave * 2 * DX + d] = v1;
                red[nw * kN + wave * 2 * DX + DX + d] = v2;
            }
        }
    }
    __syncthreads();
    if (tid < kN) {
        float v = 0.f;
        for (int w = 0; w < nw; ++w) v += red[w * kN + tid];
        a.scanPart[tb * kN + tid] = v;
    }
    if (first && tid < DX) {
        float v1 = 0.f, v2 = 0.f;
        for (int w = 0; w < nw; ++w) {
            v1 += red[nw * kN + w * 2 * DX + tid];
            v2 += red[nw * kN + w * 2 * DX + DX + tid];
        }
        const bool same0 = (a.fm0 == a.m0);
        a.dm0[b * DX + tid] = same0 ? v1 + v2 : v1;
        a.dfm0[b * DX + tid] = same0 ? 0.f : v2;
    }
}

template <int DX, int DY, int H>
static void launch_filter_bwd_scan(const FilterBwdArgs& a, hipStream_t stream) {
    using MQ = MlpLds<DX, H, DX, 1>;
    using MG = MlpLds<DX, H, DY, 1>;
    using AC = FAcc<DX>;
    constexpr int kN = AC::kSg + DY;
    const int NT = (a.N + 63) & ~63;
    const size_t ldsw = sizeof(float) * (MQ::kSize + MG::kSize);
    hipLaunchKernelGGL((fbs_coeff_kernel<DX, DY, H>), dim3(a.T, a.B), dim3(NT), ldsw, stream, a);
    const size_t ldss = sizeof(float) * 2 * DX * a.N * (a.N <= 128 ? 1 : 4);
    // registers of the record ring: DEPTH x PPL x REC (12 / 16 / 28 floats) -- <= ~250 of the 512 a lone wave per SIMD may use
    constexpr int D1 = (DX == 2) ? 16 : (DX == 3) ? 12 : 8, D2 = D1 / 2;
    if (a.N <= 64) hipLaunchKernelGGL((fbs_scan_kernel<DX, 1, 1, D1>), dim3(a.B), dim3(64), ldss, stream, a);
    else if (a.N <= 128) hipLaunchKernelGGL((fbs_scan_kernel<DX, 1, 2, D2>), dim3(a.B), dim3(64), ldss, stream, a);
    else if (a.N <= 256) hipLaunchKernelGGL((fbs_scan_kernel<DX, 4, 1, D1>), dim3(a.B), dim3(256), ldss, stream, a);
    else hipLaunchKernelGGL((fbs_scan_kernel<DX, 4, 2, D2>), dim3(a.B), dim3(256), ldss, stream, a);
    const size_t ldsr = ldsw + sizeof(float) * ((NT / 64) * (kN + 2 * DX) + 16);
    hipLaunchKernelGGL((fbs_rows_kernel<DX, DY, H>), dim3(a.T, a.B), dim3(NT), ldsr, stream, a);
    launch_step_fold(a.scanPart, a.T, a.B, kN, a.sacc, stream);
}
#endif   // PSVO_L == 1

struct FilterBwdOut {
    float *dsig_q1, *dsig_q2, *dsig_f, *dsig_g, *dsig0, *dfsig0;
};

template <int DX, int DY, int H, bool AD = false>
static int launch_filter_bwd(const FilterBwdArgsT<AD>& a, const FilterBwdOut& o, hipStream_t stream) {
    using MQ = MlpLds<DX, H, DX, PSVO_L>;
    using MG = MlpLds<DX, H, DY, PSVO_L>;
    const int NT = (a.N + 63) & ~63;
    FilterBwdArgsT<AD> aw = a;
    const size_t arrays = a.bootstrap ? 2 : 4;       // d P1 (+ d Fm) double-buffered; the d Fm pair only without bootstrap
    size_t lds = sizeof(float) * (2 * MQ::kSize + MG::kSize + arrays * (size_t)(NT / 64) * DX * NT + 16);
    // (N <= 256 only: at N = 512 the eight copies cost 3 % of the C5 step -- 32 reads and clears per particle and step at
    //  Dx = 4 -- and C5 is the configuration that can least afford it; there the scatter keeps its float atomics)
    aw.wave_copies = a.N <= 256 && lds <= 150 * 1024;
    if (!aw.wave_copies) lds = sizeof(float) * (2 * MQ::kSize + MG::kSize + arrays * DX * NT + 16);
    clear_hip_error();
    constexpr bool kLppOk = (H % 16 == 0) && (PSVO_L == 2 || (H <= 32 && DX <= 3));   // (two layers: as in filter_fwd.hip)
    bool lpp = false;
#if PSVO_L == 1
    // Used where the reverse filter IS the tail of the step: the filter-only objectives (no upstream gradient from a backward
    // simulation: C2 0.90 -> 0.67 ms) and N > 256 (one workgroup per sequence on 8 CUs at C5: 71.2 -> 66.7 ms).  Behind a
    // backward simulation at N <= 256 the tail is bound by the weight gradients that run beside it -- C* 3.45 -> 3.42, C4
    // unchanged -- and the persistent kernel stays (psvo_set_tuning(PSVO_TUNE_FILTER_BWD, 2) forces the scan everywhere).
    const bool scan_pays = (!a.dFm_ext && !a.dlogW_ext) || a.N > 256 || g_tune_filter_bwd_scan == 2;
    // (never for an adaptive call: the scan's recurrence assumes a gather at every step)
    if (!AD && g_tune_filter_bwd_scan && scan_pays && a.bootstrap && a.resample && a.nparts <= 1 && a.scanAB && a.scanPart) {
        launch_filter_bwd_scan<DX, DY, H>(a, stream);
        lpp = true;      // (the persistent kernels are skipped)
    } else
#endif
    if constexpr (kLppOk) {
        if (a.N <= 128) {   // latency-bound regime: four lanes per particle
            const int NT4 = (4 * a.N + 63) & ~63;
            const size_t lds4 = sizeof(float) * (2 * MQ::kSize + MG::kSize + 4 * (NT4 / 64) * DX * (NT4 / 4) + 16);
            if constexpr (AD)
                hipLaunchKernelGGL((filter_bwd_lpp_ad_kernel<DX, DY, H>), dim3(a.B), dim3(NT4), lds4, stream, a);
            else
                hipLaunchKernelGGL((filter_bwd_lpp_kernel<DX, DY, H>), dim3(a.B), dim3(NT4), lds4, stream, a);
            lpp = true;
        }
    }
    if (lpp) {
    } else if (g_tune_deterministic && !aw.wave_copies) {
        // fixed-order scatter (see filter_bwd_kernel): the most copies, down to one, whose single buffer fits
        const size_t arrays1 = a.bootstrap ? 1 : 2;
        auto lds_det = [&](int nc) { return sizeof(float) * (2 * MQ::kSize + MG::kSize + arrays1 * nc * DX * (size_t)NT + 16); };
        int nc = NT / 64;
        while (nc > 1 && lds_det(nc) > 150 * 1024) --nc;
        aw.det_copies = nc;
        if constexpr (AD) {
            if (NT <= 256)
                hipLaunchKernelGGL((filter_bwd_ad_kernel<DX, DY, H, 256, true>), dim3(a.B), dim3(NT), lds_det(nc), stream, aw);
            else
                hipLaunchKernelGGL((filter_bwd_ad_kernel<DX, DY, H, 512, true>), dim3(a.B), dim3(NT), lds_det(nc), stream, aw);
        } else if (NT <= 256)
            hipLaunchKernelGGL((filter_bwd_kernel<DX, DY, H, 256, true>), dim3(a.B), dim3(NT), lds_det(nc), stream, aw);
        else
            hipLaunchKernelGGL((filter_bwd_kernel<DX, DY, H, 512, true>), dim3(a.B), dim3(NT), lds_det(nc), stream, aw);
    } else if constexpr (AD) {
        if (NT <= 256)
            hipLaunchKernelGGL((filter_bwd_ad_kernel<DX, DY, H, 256>), dim3(a.B), dim3(NT), lds, stream, aw);
        else
            hipLaunchKernelGGL((filter_bwd_ad_kernel<DX, DY, H, 512>), dim3(a.B), dim3(NT), lds, stream, aw);
    } else if (NT <= 256)
        hipLaunchKernelGGL((filter_bwd_kernel<DX, DY, H, 256>), dim3(a.B), dim3(NT), lds, stream, aw);
    else
        hipLaunchKernelGGL((filter_bwd_kernel<DX, DY, H, 512>), dim3(a.B), dim3(NT), lds, stream, aw);
    if (a.two_q) {
        launch_row_sum(a.dm2_rows, (long long)a.T * a.B * DX, a.N, a.dmu2, stream);
    }
    // (DX is a template value inside the envelope: the status can only be PSVO_OK)
    (void)launch_filter_bwd_finalize(DX, {a.sacc, a.B, DY, a.two_q, a.bootstrap, a.sig_q1, a.sig_q2, a.sig0, (int)(a.fsig0 == a.sig0),
                                    o.dsig_q1, o.dsig_q2, o.dsig_f, o.dsig_g, o.dsig0, o.dfsig0}, stream);
    return launch_status();
}

}  // inline namespace PSVO_LNS
}  // namespace psvo

#if PSVO_L == 1   // (sizing helpers: independent of the number of hidden layers)
extern "C" int psvo_filter_acc_size(int Dx, int Dy) { return 10 * Dx + Dy; }

extern "C" long long psvo_filter_ws_floats(int B, int T, int N, int Dx, int Dy) {
    return psvo::filter_ws_layout(B, T, N, Dx, Dy).total;
}
#endif

namespace psvo {
inline namespace PSVO_LNS {
// the checks and the launch behind psvo_filter_backward (rs == nullptr) and psvo_filter_backward_adaptive
static int filter_backward_checked(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, int nparts,
    const float* dFm_ext, const float* dlogW_ext, float* dP, float* dF, float* dG, float* dmu2, float* dm0,
    float* dfm0, float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
    float* sacc, const int32_t* rs, void* stream) {
    if (!mlp_layers_ok(q1) || !mlp_layers_ok(f) || !mlp_layers_ok(g)) return PSVO_ERR_INVALID;
    if (!desc || !q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X || !Fm ||
        !logW || !lse || !dP || !dG || !dm0 || !dfm0 || !dsig_q1 || !dsig_q2 || !dsig_f || !dsig_g || !dsig0 ||
        !dfsig0 || !sacc)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2 || !dmu2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f || !P1 || !dF)) return PSVO_ERR_INVALID;
    if (desc->resample && !idx) return PSVO_ERR_INVALID;
    if ((dFm_ext || dlogW_ext) && nparts <= 0) return PSVO_ERR_INVALID;
    if (desc->N > 512) return PSVO_ERR_UNSUPPORTED;

    FilterBwdArgs a;
    a.wave_copies = 0;
    a.det_copies = 1;
    a.B = desc->B; a.T = desc->T; a.N = desc->N;
    a.resample = desc->resample; a.two_q = desc->two_q; a.bootstrap = desc->bootstrap; a.emission = desc->emission;
    a.q1 = *q1; a.f = desc->bootstrap ? *q1 : *f; a.g = *g;
    a.sig_q1 = sig_q1; a.sig_q2 = sig_q2; a.sig_f = sig_f; a.sig_g = sig_g;
    a.mu2 = mu2; a.m0 = m0; a.sig0 = sig0; a.fm0 = fm0; a.fsig0 = fsig0; a.obs = obs; a.eps = eps;
    a.X = X; a.Fm = Fm; a.P1 = P1; a.logW = logW; a.lse = lse; a.idx = idx;
    a.dlse = dlse; a.nparts = nparts; a.dFm_ext = dFm_ext; a.dlogW_ext = dlogW_ext;
    a.dP = dP; a.dF = dF; a.dG = dG; a.dmu2 = dmu2; a.dm0 = dm0; a.dfm0 = dfm0; a.sacc = sacc;
    const FilterWsLayout l = filter_ws_layout(desc->B, desc->T, desc->N, desc->Dx, desc->Dy);
    const bool scan = (reinterpret_cast<uintptr_t>(sacc + l.rec) & 15) == 0;      // (a misaligned workspace: the persistent kernel)
    a.dm2_rows = sacc + l.dm2;
    a.scanAB = scan ? sacc + l.rec : nullptr; a.scanPart = scan ? sacc + l.part : nullptr;
    FilterBwdOut o{dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rs) {
        FilterBwdArgsAd aa;
        static_cast<FilterBwdArgs&>(aa) = a;
        aa.rs = rs;
        return dispatch_shape(desc->Dx, desc->Dy, desc->H, [&](auto dx, auto dy, auto h) {
            return launch_filter_bwd<dx(), dy(), h(), true>(aa, o, s); });
    }
    return dispatch_shape(desc->Dx, desc->Dy, desc->H, [&](auto dx, auto dy, auto h) {
        return launch_filter_bwd<dx(), dy(), h()>(a, o, s); });
}
}  // inline namespace PSVO_LNS
}  // namespace psvo

PSVO_L2_DECL(psvo_filter_backward)
PSVO_ENTRY(psvo_filter_backward)(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, int nparts,
    const float* dFm_ext, const float* dlogW_ext, float* dP, float* dF, float* dG, float* dmu2, float* dm0,
    float* dfm0, float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
    float* sacc, void* stream) {
    using namespace psvo;
    if (!desc_layers_ok(desc) || !desc_emission_ok(desc)) return PSVO_ERR_UNSUPPORTED;
#if PSVO_L == 1
    if (desc && desc->layers == 2)
        return psvo_filter_backward_l2(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0,
            obs, eps, X, Fm, P1, logW, lse, idx, dlse, nparts, dFm_ext, dlogW_ext, dP, dF, dG, dmu2, dm0, dfm0,
            dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, sacc, stream);
#endif
    return filter_backward_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0,
            obs, eps, X, Fm, P1, logW, lse, idx, dlse, nparts, dFm_ext, dlogW_ext, dP, dF, dG, dmu2, dm0, dfm0,
            dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, sacc, nullptr, stream);
}

PSVO_L2_DECL(psvo_filter_backward_adaptive)
PSVO_ENTRY(psvo_filter_backward_adaptive)(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, int nparts,
    const float* dFm_ext, const float* dlogW_ext, float* dP, float* dF, float* dG, float* dmu2, float* dm0,
    float* dfm0, float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
    float* sacc, const int32_t* rs, void* stream) {
    using namespace psvo;
    // the adaptive contract first: a filter that resamples at all, its decisions; no backward simulation behind it (yet)
    if (!desc || !desc->resample || !rs) return PSVO_ERR_INVALID;
    if (nparts > 1 || dFm_ext || dlogW_ext) return PSVO_ERR_UNSUPPORTED;
    if (!desc_layers_ok(desc) || !desc_emission_ok(desc)) return PSVO_ERR_UNSUPPORTED;
#if PSVO_L == 1
    if (desc->layers == 2)
        return psvo_filter_backward_adaptive_l2(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0,
            obs, eps, X, Fm, P1, logW, lse, idx, dlse, nparts, dFm_ext, dlogW_ext, dP, dF, dG, dmu2, dm0, dfm0,
            dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, sacc, rs, stream);
#endif
    return filter_backward_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0,
            obs, eps, X, Fm, P1, logW, lse, idx, dlse, nparts, dFm_ext, dlogW_ext, dP, dF, dG, dmu2, dm0, dfm0,
            dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, sacc, rs, stream);
}
