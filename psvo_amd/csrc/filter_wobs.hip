// Wide observations ("wobs"): the forward particle filter, its reverse pass and the weight gradient of MLP_g for
// 3 <= Dy <= 32 (include/psvo_hip.h: psvo_filter_forward_wobs, psvo_filter_backward_wobs, psvo_mlp_wgrad_wobs).
//
// The plain kernels (filter_fwd.hip, filter_bwd.hip, mlp_grad.hip) are templated on Dy in {1, 2}: the emission mean, its
// gradient and the per-output sums are registers indexed by a compile-time Dy.  That does not scale to 32 outputs (and 30
// instantiations per shape), so here Dy is a RUN-TIME bound and nothing is instantiated per width:
//   * a lane (= particle) keeps the H hidden activations of MLP_g in registers and walks the outputs e = 0 .. Dy-1 in a
//     rolled loop; row e of the transposed output layer W2T[e][:], b2[e], 1 / sig_g[e] and the step's observation y[t,b,e]
//     are read from LDS at wave-uniform addresses (broadcasts).  The emission log-density is accumulated in that order;
//   * the observation row of step t+1 is requested by the first Dy lanes while step t computes and lands in the other
//     half of a two-row LDS buffer behind the barrier that ends the step;
//   * the reverse kernel writes the rows d g_e in that loop and reads them back for the input gradient, hidden units in
//     chunks of 16 or 32 (H + H live values per lane would not fit a 512-lane workgroup); the Dy sums of d sig_g live in LDS, one column per lane (owner lanes), folded in lane order after the time loop;
//   * the gather of resampled particles back-propagates as a scatter-add into the parents.  Every parent collects its
//     children itself, in child order, from a staged (ancestor, value) list in LDS: no atomics, one fixed order.
// Kernels are instantiated for Dx in {2,3,4} x H in {16,32,64} (9 forward; 18 reverse: with and without the upstream gradients of Fm / logW, template flag EXT), the weight gradient for Din in {1..4} x
// H in {16,32,64} x one or two 16-wide output tiles (24).
#include "wobs_common.h"

namespace psvo {
namespace wobs {

struct FwdArgs {
    int B, T, N, Dy;
    int resample, two_q, bootstrap, emission;
    psvo_mlp q1, f, g;
    const float *sig_q1, *sig_q2, *sig_f, *sig_g;
    const float *mu2, *m0, *sig0, *fm0, *fsig0, *obs, *eps, *u;
    const int32_t* idx_in;
    float *X, *Xanc, *Fm, *P1, *logW;
    int32_t* idx_out;
    float* lse;
};

// ---------------------------------------------------------------------------------------------
// Forward filter: lane = particle, workgroup = sequence, t in-kernel (filter_fwd.hip's lane-per-particle kernel with the
// emission walked over a run-time Dy).  Same outputs and draw rule: idx = #{k : cdf[k] <= u * total}, clamped to N - 1.
// ---------------------------------------------------------------------------------------------
// CNT: the count emission (psvo_desc.emission = 2), a compile-time form so that the Gaussian / unit-normal instantiations keep
// their code and registers.  1 / sig_g is not used; the log-factorial row of a step travels with its observation row.
template <int DX, int H, bool CNT>
__global__ void __launch_bounds__(512) filter_fwd_wobs_kernel(const FwdArgs a) {
    using MQ = MlpLds<DX, H, DX, 1>;
    using MG = GLds<DX, H>;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = blockDim.x, nw = NT >> 6;
    const int b = blockIdx.x, B = a.B, T = a.T, N = a.N, Dy = a.Dy;
    const bool valid = tid < N;
    const int n = valid ? tid : N - 1;  // clamp so that loads stay in bounds

    float* wq1 = smem;
    float* wf = wq1 + MQ::kSize;
    float* wg = wf + MQ::kSize;
    float* isg = wg + MG::kSize;        // [kMaxDy] 1 / sig_g
    float* ybuf = isg + kMaxDy;         // [2][kMaxDy] observation rows of step t (t & 1) and t + 1
    float* cdf = ybuf + 2 * kMaxDy;     // [NT]
    float* sx = cdf + NT;               // [DX][NT] staged X_t
    float* sp = sx + DX * NT;           // [DX][NT] staged MLP_q1(X_t)
    float* sf = sp + DX * NT;           // [DX][NT] staged MLP_f(X_t) (unused when bootstrap)
    float* red = sf + DX * NT;          // 48 floats scratch
    float* lfbuf = red + 48;            // CNT: [2][kMaxDy] log Gamma(y + 1) of the rows in ybuf

    MQ::load(wq1, a.q1, tid, NT);
    if (!a.bootstrap) MQ::load(wf, a.f, tid, NT);
    MG::load(wg, a.g, Dy, tid, NT);
    const float* wfm = a.bootstrap ? wq1 : wf;
    if (tid < Dy) {
        if constexpr (!CNT) isg[tid] = 1.f / a.sig_g[tid];
        const float y0 = a.obs[(size_t)b * Dy + tid];
        ybuf[tid] = y0;
        if constexpr (CNT) lfbuf[tid] = log_factorial(y0);
    }

    float sq1[DX], sq2[DX], sfv[DX], s0[DX], fs0[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        sq1[d] = a.sig_q1[d];
        sq2[d] = a.two_q ? a.sig_q2[d] : 1.f;
        sfv[d] = a.bootstrap ? a.sig_q1[d] : a.sig_f[d];
        s0[d] = a.sig0[d];
        fs0[d] = a.fsig0[d];
    }
    float lg = -Dy * kHalfLog2Pi;
    if constexpr (!CNT) {
        for (int e = 0; e < Dy; ++e) lg -= logf(a.sig_g[e]);
    }
    const StepK<DX> K0 = make_stepk<DX>(s0, sq2, fs0, a.two_q != 0);
    const StepK<DX> K1 = make_stepk<DX>(sq1, sq2, sfv, a.two_q != 0);
    const float neg_logN = -logf((float)N);
    const float ninf = -__builtin_huge_valf();

    float mean1[DX], fmean[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        mean1[d] = a.m0[b * DX + d];
        fmean[d] = a.fm0[b * DX + d];
    }
    float lnw = neg_logN;

    // software prefetch of the next step's inputs
    float eps_c[DX], mu2_c[DX], u_c = 0.f;
    int idx_c = 0;
    auto load_inputs = [&](int t, float (&e)[DX], float (&m)[DX], float& uu, int& ii) {
        const size_t tb = (size_t)t * B + b;
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            e[d] = a.eps[(tb * DX + d) * N + n];
            m[d] = a.two_q ? a.mu2[tb * DX + d] : 0.f;
        }
        if (a.resample) {
            if (a.idx_in) ii = a.idx_in[tb * N + n];
            else uu = a.u[tb * N + n];
        }
    };
    load_inputs(0, eps_c, mu2_c, u_c, idx_c);
    __syncthreads();  // weights, scales, first observation row visible

    for (int t = 0; t < T; ++t) {
        const size_t tb = (size_t)t * B + b;
        const StepK<DX> K = (t == 0) ? K0 : K1;
        int zo = 0;
        asm volatile("" : "+v"(zo));        // weights are re-read from LDS every step, never hoisted into registers
        const float* wq1_t = wq1 + zo;
        const float* wfm_t = wfm + zo;
        const float* wg_t = wg + zo;
        const float* y_t = ybuf + (t & 1) * kMaxDy + zo;

        float eps_n[DX], mu2_n[DX], u_n = 0.f, y_n = 0.f;
        int idx_n = 0;
        if (t + 1 < T) {
            load_inputs(t + 1, eps_n, mu2_n, u_n, idx_n);
            if (tid < Dy) y_n = a.obs[(tb + B) * Dy + tid];
        }

        // ---- proposal: product of two diagonal Gaussians on *scales* (SVO.py:186-197) ----------
        float mu[DX], x[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            mu[d] = a.two_q ? K.c[d] * fmaf(K.i1[d], mean1[d], K.i2[d] * mu2_c[d]) : mean1[d];
            x[d] = fmaf(K.c[d], eps_c[d], mu[d]);
        }
        const float q_lp = diag_lp<DX>(x, mu, K.ic, K.lq);
        const float f_lp = diag_lp<DX>(x, fmean, K.ifs, K.lf);

        // ---- emission: Dy terms in the order e = 0 .. Dy - 1 ---------------------------------------
        float g_lp;
        {
            float h[H];
            MG::hidden(wg_t, x, h);
            float acc = 0.f;
            if constexpr (CNT) {     // y log lam - lam - log Gamma(y + 1), one term per output
                const float* lf_t = lfbuf + (t & 1) * kMaxDy + zo;
#pragma unroll 1
                for (int e = 0; e < Dy; ++e) acc += count_term(y_t[e], MG::out(wg_t, e, h)) - lf_t[e];
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
        }
        float lw = f_lp + g_lp - q_lp + lnw;
        if (!valid) lw = ninf;

        // ---- next-step proposal / transition means of every pre-resampling particle -----------
        float p1[DX], fm[DX];
        MQ::template eval<true>(wq1_t, x, p1);
        if (a.bootstrap) {
#pragma unroll
            for (int d = 0; d < DX; ++d) fm[d] = p1[d];
        } else {
            MQ::template eval<true>(wfm_t, x, fm);
        }
        if (valid) {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                a.X[(tb * DX + d) * N + n] = x[d];
                a.Fm[(tb * DX + d) * N + n] = fm[d];
                if (a.P1) a.P1[(tb * DX + d) * N + n] = p1[d];
            }
            a.logW[tb * N + n] = lw;
        }

        // ---- log-sum-exp over particles and multinomial ancestors (SVO.py:266-300) -------------
        const float mx = block_max(lw, red, 0, wave, lane, nw);
        const float w = valid ? exp2_fast((lw - mx) * kLog2e) : 0.f;
        float sc = wave_incl_scan(w, lane);
        float total;
        if (nw > 1) {
            float* wt = red + 32;
            if (lane == 63) wt[wave] = sc;
            __syncthreads();
            float off = 0.f, tot = 0.f;
            for (int i = 0; i < nw; ++i) {
                const float v = wt[i];
                if (i < wave) off += v;
                tot += v;
            }
            sc += off;
            total = tot;
        } else {
            total = lane_bcast(sc, 63);
        }
        const float lse_t = fmaf(kLn2, log2_fast(total), mx);
        if (tid == 0) a.lse[tb] = lse_t;

        if (a.resample) {
            cdf[tid] = sc;
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                sx[d * NT + tid] = x[d];
                sp[d * NT + tid] = p1[d];
                if (!a.bootstrap) sf[d * NT + tid] = fm[d];
            }
            __syncthreads();
            int idx;
            if (a.idx_in) {
                idx = idx_c;
            } else {
                // count of cdf entries <= u * total (cdf is non-decreasing)
                const float target = u_c * total;
                int pos = 0;
                for (int s = 1 << (31 - __clz(N)); s > 0; s >>= 1) {
                    const int p = pos + s;
                    if (p <= N && cdf[p - 1] <= target) pos = p;
                }
                idx = min(pos, N - 1);
            }
            idx = min(max(idx, 0), N - 1);      // (teacher-forced indices are data: keep the gather inside the staged tiles)
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                x[d] = sx[d * NT + idx];
                mean1[d] = sp[d * NT + idx];
                fmean[d] = a.bootstrap ? mean1[d] : sf[d * NT + idx];
            }
            if (valid) {
                a.idx_out[tb * N + n] = idx;
#pragma unroll
                for (int d = 0; d < DX; ++d) a.Xanc[(tb * DX + d) * N + n] = x[d];
            }
            lnw = neg_logN;
        } else {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                mean1[d] = p1[d];
                fmean[d] = fm[d];
            }
            if (valid) {
                a.idx_out[tb * N + n] = n;
#pragma unroll
                for (int d = 0; d < DX; ++d) a.Xanc[(tb * DX + d) * N + n] = x[d];
            }
            lnw = lw - lse_t;
        }
        // the prefetched observation row goes to the half of ybuf that step t - 1 read (behind the barrier that ended it)
        if (t + 1 < T && tid < Dy) {
            ybuf[((t + 1) & 1) * kMaxDy + tid] = y_n;
            if constexpr (CNT) lfbuf[((t + 1) & 1) * kMaxDy + tid] = log_factorial(y_n);
        }
        __syncthreads();  // staged tiles / red[] are rewritten next step; the next observation row is visible

#pragma unroll
        for (int d = 0; d < DX; ++d) {
            eps_c[d] = eps_n[d];
            mu2_c[d] = mu2_n[d];
        }
        u_c = u_n;
        idx_c = idx_n;
    }
}

template <int DX, int H>
static size_t fwd_lds_bytes(int NT, bool count) {
    return sizeof(float) * (2 * MlpLds<DX, H, DX, 1>::kSize + GLds<DX, H>::kSize + 3 * kMaxDy + NT + 3 * DX * NT + 48 +
                            (count ? 2 * kMaxDy : 0));
}

template <int DX, int H>
static int launch_fwd(const FwdArgs& a, hipStream_t stream) {
    const int NT = (a.N + 63) & ~63;
    const bool count = a.emission == 2;
    const size_t lds = fwd_lds_bytes<DX, H>(NT, count);
    clear_hip_error();
    if (count) hipLaunchKernelGGL((filter_fwd_wobs_kernel<DX, H, true>), dim3(a.B), dim3(NT), lds, stream, a);
    else hipLaunchKernelGGL((filter_fwd_wobs_kernel<DX, H, false>), dim3(a.B), dim3(NT), lds, stream, a);
    return launch_status();
}

// ---------------------------------------------------------------------------------------------
// Reverse filter (filter_bwd.hip's persistent kernel; upstream gradients: d lse and, through the _ext entry point, d Fm / d logW).  One workgroup per sequence walks
// t = T-1 .. 0.  What step t leaves for step t-1 is D[n] = d loss / d (MLP_q1(x_{t-1}[n]), MLP_f(x_{t-1}[n])), carried in the
// parent's own registers: the children stage (ancestor, values) in LDS and every parent adds its children in child order.
// Per-sequence sums (common.h: FAcc): [2 sets x 5 Dx | Dy].
// ---------------------------------------------------------------------------------------------
struct BwdArgs {
    int B, T, N, Dy;
    int resample, two_q, bootstrap, emission;
    psvo_mlp q1, f, g;
    const float *sig_q1, *sig_q2, *sig_f, *sig_g;
    const float *mu2, *m0, *sig0, *fm0, *fsig0, *obs, *eps;
    const float *X, *Fm, *P1, *logW, *lse;
    const int32_t* idx;
    const float* dlse;
    float *dP, *dF, *dG, *dmu2, *dm0, *dfm0;
    float* sacc;             // (B, 10 Dx + Dy) per-sequence sums
    float* dm2_rows;         // (T,B,Dx,N) per-particle d mu2 rows, summed over N afterwards
    // psvo_filter_backward_wobs_ext (kernel instantiated with EXT = true; the plain form never reads these).  They sit behind
    // everything else and are fetched from the kernel arguments where they are used (common.h: PSVO_ARG): held in SGPRs across
    // the time loop they pushed the kernel into scratch.
    const float* dFm_ext;    // (T,B,nparts,Dx,N) or null: d loss / d Fm from a backward simulation behind the filter
    const float* dlogW_ext;  // (T,B,nparts,N) or null: d loss / d logW, likewise
    int nparts;              // leading "parts" axis of the two
};

// nparts of the launch, re-read from the kernel arguments at its point of use (arg_ptr of common.h for an int)
__device__ __forceinline__ int arg_nparts() {
    unsigned off = (unsigned)offsetof(BwdArgs, nparts);
    asm volatile("" : "+s"(off));
    typedef const char __attribute__((address_space(4))) * kptr;
    typedef const int __attribute__((address_space(4))) * iptr;
    return *(iptr)((kptr)__builtin_amdgcn_kernarg_segment_ptr() + off);
}

// CNT: the count emission (as in the forward kernel); its d G rows are dlw (y / lam - 1) sigmoid(r), there is no d sig_g
template <int DX, int H, bool EXT, bool CNT>
__global__ void __launch_bounds__(512) filter_bwd_wobs_kernel(const BwdArgs a) {
    using MQ = MlpLds<DX, H, DX, 1>;
    using MG = GLds<DX, H>;
    using AC = FAcc<DX>;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = blockDim.x, nw = NT >> 6;
    const int b = blockIdx.x, B = a.B, T = a.T, N = a.N, Dy = a.Dy;
    const bool valid = tid < N;
    const int n = valid ? tid : N - 1;
    const int NV = a.bootstrap ? DX : 2 * DX;     // values a child hands to its parent

    float* wq1 = smem;
    float* wf = wq1 + MQ::kSize;
    float* wg = wf + MQ::kSize;
    float* isg = wg + MG::kSize;        // [kMaxDy]
    float* ybuf = isg + kMaxDy;         // [2][kMaxDy]
    float* red = ybuf + 2 * kMaxDy;     // [16]
    int* sa = reinterpret_cast<int*>(red + 16);   // [NT] staged ancestors (-1: no particle)
    float* sv = red + 16 + NT;          // [NV][NT] staged values
    float* sg = sv + NV * NT;           // [Dy][NT] d sig_g sums, one column per lane
    float* kst = sg + Dy * NT;          // [2][5 DX] step constants c | 1/c | 1/s1 | 1/s2 | 1/fs of t = 0 and of t >= 1

    MQ::load(wq1, a.q1, tid, NT);
    if (!a.bootstrap) MQ::load(wf, a.f, tid, NT);
    MG::load(wg, a.g, Dy, tid, NT);
    const float* wfm = a.bootstrap ? wq1 : wf;
    if (tid < Dy) {
        if constexpr (!CNT) isg[tid] = 1.f / a.sig_g[tid];
        ybuf[((T - 1) & 1) * kMaxDy + tid] = a.obs[((size_t)(T - 1) * B + b) * Dy + tid];
    }
    if constexpr (!CNT) {
        for (int e = 0; e < Dy; ++e) sg[e * NT + tid] = 0.f;
    }
    if (tid == 0) {
        float sq1[DX], sq2[DX], sfv[DX], s0[DX], fs0[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            sq1[d] = a.sig_q1[d];
            sq2[d] = a.two_q ? a.sig_q2[d] : 1.f;
            sfv[d] = a.bootstrap ? a.sig_q1[d] : a.sig_f[d];
            s0[d] = a.sig0[d];
            fs0[d] = a.fsig0[d];
        }
        const StepK<DX> K0 = make_stepk<DX>(s0, sq2, fs0, a.two_q != 0);
        const StepK<DX> K1 = make_stepk<DX>(sq1, sq2, sfv, a.two_q != 0);
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            kst[d] = K0.c[d]; kst[DX + d] = K0.ic[d]; kst[2 * DX + d] = K0.i1[d]; kst[3 * DX + d] = K0.i2[d];
            kst[4 * DX + d] = K0.ifs[d];
            kst[5 * DX + d] = K1.c[d]; kst[6 * DX + d] = K1.ic[d]; kst[7 * DX + d] = K1.i1[d]; kst[8 * DX + d] = K1.i2[d];
            kst[9 * DX + d] = K1.ifs[d];
        }
    }

    // (registers carried over the time loop are kept few: the emission loop below holds 2 H values per lane)
    float acc[AC::kSet];            // sums of the steps t >= 1; the t = 0 set goes out from its own step
#pragma unroll
    for (int i = 0; i < AC::kSet; ++i) acc[i] = 0.f;
    float dlnw = 0.f;  // IWAE: gradient w.r.t. the normalised log-weight carried into step t+1
    float carryP[DX], carryF[DX];   // gradients w.r.t. MLP_q1(x_t[n]) / MLP_f(x_t[n]) collected from step t + 1
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        carryP[d] = 0.f;
        carryF[d] = 0.f;
    }
    const int NACC = 2 * AC::kSet + Dy;
    __syncthreads();

    for (int t = T - 1; t >= 0; --t) {
        const size_t tb = (size_t)t * B + b;
        const size_t tp = (t == 0) ? tb : tb - B;              // (t = 0 has no parent: values replaced below)
        const bool first = (t == 0);
        int zo = 0;
        asm volatile("" : "+v"(zo));        // weights and constants are re-read from LDS every step, never kept in registers
        const float* wq1_t = wq1 + zo;
        const float* wfm_t = wfm + zo;
        const float* wg_t = wg + zo;
        const float* y_t = ybuf + (t & 1) * kMaxDy + zo;
        const float* K = kst + (first ? 0 : 5 * DX) + zo;

        float y_n = 0.f;
        if (t >= 1 && tid < Dy) {       // next step's observation row, in flight during this one
            if constexpr (CNT) y_n = PSVO_ARG(BwdArgs, obs)[(tb - B) * Dy + tid];      // (see dlse below)
            else y_n = a.obs[(tb - B) * Dy + tid];
        }

        float x[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) x[d] = a.X[(tb * DX + d) * N + n];
        const float lw_t = a.logW[tb * N + n], lse_t = a.lse[tb];
        float dlse_t;
        if constexpr (CNT) {    // (dlse and obs re-read from the kernel arguments where they are used, as the _ext pointers are:
            // held across the time loop they left a dead 64-byte spill slot, i.e. a scratch allocation, in five EXT forms)
            const float* dlse = PSVO_ARG(BwdArgs, dlse);
            dlse_t = dlse ? dlse[tb] : 0.f;
        } else {
            dlse_t = a.dlse ? a.dlse[tb] : 0.f;
        }

        // ---- gradient w.r.t. logW_t[n] ------------------------------------------------------------
        const float sm = valid ? exp2_fast((lw_t - lse_t) * kLog2e) : 0.f;
        float dlw = dlse_t * sm;
        if constexpr (EXT) {    // parts added in part order
            const float* dlogW_ext = PSVO_ARG(BwdArgs, dlogW_ext);
            if (dlogW_ext) {
                const int np = arg_nparts();
                float ext = 0.f;
                for (int p = 0; p < np; ++p) ext += dlogW_ext[(tb * np + p) * N + n];
                dlw += ext;
            }
        }
        if (!a.resample) {
            const float tot = block_sum(dlnw, red, wave, lane, nw);
            dlw += dlnw - sm * tot;
        }
        if (!valid) dlw = 0.f;
        dlnw = first ? 0.f : dlw;

        // ---- emission: outputs in the order o = 0 .. Dy - 1 -----------------------------------------------
        float dx[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) dx[d] = 0.f;
        {
            float h[H];
            MG::hidden(wg_t, x, h);
            if constexpr (CNT) {
#pragma unroll 1
                for (int o = 0; o < Dy; ++o) {
                    const float dr = dlw * count_dterm(y_t[o], MG::out(wg_t, o, h));
                    if (valid) a.dG[(tb * Dy + o) * N + n] = dr;
                }
            } else {
#pragma unroll 1
                for (int o = 0; o < Dy; ++o) {
                    float gm = MG::out(wg_t, o, h);
                    float dmean = 1.f;
                    if (a.emission) { dmean = emis_dmean(gm); gm = emis_mean(gm); }
                    const float is = isg[o];
                    const float z = (y_t[o] - gm) * is;
                    sg[o * NT + tid] += dlw * (z * z - 1.f) * is;
                    if (valid) a.dG[(tb * Dy + o) * N + n] = dlw * z * is * dmean;
                }
            }
        }
        // (second walk over the outputs: the lane reads its own d G rows back -- H partial sums beside the H activations
        //  would not fit the 256 registers of a 512-lane workgroup)
        MG::template bwd_input<(H >= 64 ? 32 : 16)>(wg_t, Dy, a.dG + (tb * Dy) * N + n, (size_t)N, valid, x, dx);
        // ---- the rest of the step's forward quantities (loaded here: not live across the emission loop) ------
        int anc = n;
        if (t >= 1 && a.resample) anc = min(max(a.idx[tp * N + n], 0), N - 1);
        float e[DX], m2[DX], mean1[DX], fmean[DX], mu[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            e[d] = a.eps[(tb * DX + d) * N + n];
            m2[d] = a.two_q ? a.mu2[tb * DX + d] : 0.f;
            if (first) {
                fmean[d] = a.fm0[b * DX + d];
                mean1[d] = a.m0[b * DX + d];
            } else {
                fmean[d] = a.Fm[(tp * DX + d) * N + anc];
                mean1[d] = a.bootstrap ? fmean[d] : a.P1[(tp * DX + d) * N + anc];
            }
            mu[d] = a.two_q ? K[d] * fmaf(K[2 * DX + d], mean1[d], K[3 * DX + d] * m2[d]) : mean1[d];
        }
        // ---- transition and proposal densities ------------------------------------------------------
        float inc[AC::kSet];
#pragma unroll
        for (int i = 0; i < AC::kSet; ++i) inc[i] = 0.f;
        float dfmean[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float ifs = K[4 * DX + d];
            const float z = (x[d] - fmean[d]) * ifs;
            const float tf = dlw * z * ifs;
            dx[d] -= tf;
            dfmean[d] = tf;
            inc[AC::kSfs + d] += dlw * (z * z - 1.f) * ifs;
            inc[AC::kSc + d] += dlw * K[DX + d];  // -dq/dc = +dlw / c
        }
        // ---- MLP_q1(x_t), MLP_f(x_t): gradients collected from step t+1 -------------------------------------
        float dPn[DX], dFn[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            dPn[d] = valid ? carryP[d] : 0.f;
            dFn[d] = (valid && !a.bootstrap) ? carryF[d] : 0.f;
        }
        if constexpr (EXT) {    // Fm is MLP_f(x_t), i.e. MLP_q1(x_t) when bootstrap; parts added in part order
            const float* dFm_ext = PSVO_ARG(BwdArgs, dFm_ext);
            if (dFm_ext) {
                const int np = arg_nparts();
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    float ext = 0.f;
                    for (int p = 0; p < np; ++p) ext += dFm_ext[((tb * np + p) * DX + d) * N + n];
                    // (two plain adds: a conditional lvalue would take the arrays' addresses and put them in scratch)
                    if (valid && a.bootstrap) dPn[d] += ext;
                    if (valid && !a.bootstrap) dFn[d] += ext;
                }
            }
        }
        if (valid) {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                a.dP[(tb * DX + d) * N + n] = dPn[d];
                if (!a.bootstrap) a.dF[(tb * DX + d) * N + n] = dFn[d];
            }
        }
        MQ::template bwd_input<true>(wq1_t, x, dPn, dx);
        if (!a.bootstrap) MQ::template bwd_input<true>(wfm_t, x, dFn, dx);

        // ---- x = mu + c eps, mu = c (mean1/s1 + mu2/s2) ----------------------------------------------------
        float dmean1[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float dmu = dx[d];
            inc[AC::kSc + d] += dmu * e[d];
            if (a.two_q) {
                dmean1[d] = dmu * K[d] * K[2 * DX + d];
                inc[AC::kSmm1 + d] += dmu * mean1[d];
                inc[AC::kSmb + d] += dmu * m2[d];
                inc[AC::kSmm + d] += dmu * mu[d];
                if (valid) a.dm2_rows[(tb * DX + d) * N + n] = dmu * K[d] * K[3 * DX + d];
            } else {
                dmean1[d] = dmu;
            }
        }
        // ---- gather backward: every parent adds its children, in child order (SVO.py:255-257) ---------------
        if (!first) {
#pragma unroll
            for (int i = 0; i < AC::kSet; ++i) acc[i] += valid ? inc[i] : 0.f;
            if (a.resample) {
                sa[tid] = valid ? anc : -1;
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    if (a.bootstrap) {
                        sv[d * NT + tid] = dmean1[d] + dfmean[d];
                    } else {
                        sv[d * NT + tid] = dmean1[d];
                        sv[(DX + d) * NT + tid] = dfmean[d];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    carryP[d] = 0.f;
                    carryF[d] = 0.f;
                }
                for (int c = 0; c < N; ++c) {
                    if (sa[c] == tid) {
#pragma unroll
                        for (int d = 0; d < DX; ++d) {
                            carryP[d] += sv[d * NT + c];
                            if (!a.bootstrap) carryF[d] += sv[(DX + d) * NT + c];
                        }
                    }
                }
            } else {
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    carryP[d] = a.bootstrap ? dmean1[d] + dfmean[d] : dmean1[d];
                    carryF[d] = dfmean[d];
                }
            }
        } else {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                const float s1 = block_sum(valid ? dmean1[d] : 0.f, red, wave, lane, nw);
                const float s2 = block_sum(valid ? dfmean[d] : 0.f, red, wave, lane, nw);
                if (tid == 0) {   // (fm0 aliasing m0: ONE tensor feeds both, its gradient is the sum -- see psvo_hip.h)
                    const bool same0 = (a.fm0 == a.m0);
                    a.dm0[b * DX + d] = same0 ? s1 + s2 : s1;
                    a.dfm0[b * DX + d] = same0 ? 0.f : s2;
                }
            }
#pragma unroll
            for (int i = 0; i < AC::kSet; ++i) {      // set 0: the sums of t = 0
                const float s = block_sum(valid ? inc[i] : 0.f, red, wave, lane, nw);
                if (tid == 0) a.sacc[(size_t)b * NACC + i] = s;
            }
        }
        if (t >= 1 && tid < Dy) ybuf[((t - 1) & 1) * kMaxDy + tid] = y_n;
        __syncthreads();   // the staged list is rewritten next step; the next observation row is visible
    }

    // ---- per-sequence sums of t >= 1 (set 1) and of d sig_g -----------------------------------------------------
#pragma unroll
    for (int i = 0; i < AC::kSet; ++i) {
        const float s = block_sum(acc[i], red, wave, lane, nw);
        if (tid == 0) a.sacc[(size_t)b * NACC + AC::kSet + i] = s;
    }
    __syncthreads();
    if (tid < Dy) {      // lane columns of d sig_g, in lane order (count emission: no scale, zeros)
        float s = 0.f;
        if constexpr (!CNT) {
            for (int i = 0; i < N; ++i) s += sg[tid * NT + i];
        }
        a.sacc[(size_t)b * NACC + AC::kSg + tid] = s;
    }
}

struct BwdOut {
    float *dsig_q1, *dsig_q2, *dsig_f, *dsig_g, *dsig0, *dfsig0;
};

template <int DX, int H>
static size_t bwd_lds_bytes(int NT, int Dy, bool bootstrap) {
    return sizeof(float) * (2 * MlpLds<DX, H, DX, 1>::kSize + GLds<DX, H>::kSize + 3 * kMaxDy + 16 + (size_t)NT
                            + (size_t)(bootstrap ? DX : 2 * DX) * NT + (size_t)Dy * NT + 10 * DX);
}

template <int DX, int H>
static int launch_bwd(const BwdArgs& a, const BwdOut& o, hipStream_t stream) {
    const int NT = (a.N + 63) & ~63;
    const size_t lds = bwd_lds_bytes<DX, H>(NT, a.Dy, a.bootstrap != 0);
    clear_hip_error();
    const bool ext = a.dFm_ext || a.dlogW_ext;
    if (a.emission == 2) {
        if (ext) hipLaunchKernelGGL((filter_bwd_wobs_kernel<DX, H, true, true>), dim3(a.B), dim3(NT), lds, stream, a);
        else hipLaunchKernelGGL((filter_bwd_wobs_kernel<DX, H, false, true>), dim3(a.B), dim3(NT), lds, stream, a);
    } else {
        if (ext) hipLaunchKernelGGL((filter_bwd_wobs_kernel<DX, H, true, false>), dim3(a.B), dim3(NT), lds, stream, a);
        else hipLaunchKernelGGL((filter_bwd_wobs_kernel<DX, H, false, false>), dim3(a.B), dim3(NT), lds, stream, a);
    }
    if (a.two_q) {
        launch_row_sum(a.dm2_rows, (long long)a.T * a.B * DX, a.N, a.dmu2, stream);
    }
    // (DX is a template value inside the envelope: the status can only be PSVO_OK)
    (void)launch_filter_bwd_finalize(DX, {a.sacc, a.B, a.Dy, a.two_q, a.bootstrap, a.sig_q1, a.sig_q2, a.sig0, (int)(a.fsig0 == a.sig0),
                                    o.dsig_q1, o.dsig_q2, o.dsig_f, o.dsig_g, o.dsig0, o.dfsig0}, stream);
    return launch_status();
}

// the envelope of the two filter entry points (host only): 3 <= Dy <= 32, one hidden layer, N <= 512; Dx and H by dispatch
static bool filter_shape_ok(const psvo_desc* d) {
    return d->Dy >= 3 && d->Dy <= kMaxDy && d->layers >= 0 && d->layers <= 1 && d->N <= 512 && d->B <= 65535;
}

template <class F>
static int dispatch_dx_h(int Dx, int H, F&& f) {
    return pick_dx(Dx, [&](auto dx) { return pick_h(H, [&](auto h) { return f(dx, h); }); });
}

// ---------------------------------------------------------------------------------------------
// Weight gradient of a one-hidden-layer MLP with 3 .. 32 outputs from per-row output gradients (mlp_grad.hip's contract):
//     dW2 += h^T dOut (H x Dout, K = rows),  dh = dOut W2^T (rows x H, K = Dout)  on v_mfma_f32_16x16x4_f32,
//     db2 += dOut, d pre = [h > 0] dh, dW1 += x^T d pre, db1 += d pre           on the VALU.
// A workgroup of four waves walks chunks of 64 rows:
//   A (VALU)  thread = (row, quarter of the units / of the outputs): h -> Hs[64][H], dOut -> Ds[64][DP] (zero beyond Dout and
//             beyond the last row: such rows and columns contribute nothing), x -> xs, db2 in registers;
//   1 (MFMA)  wave w: dh of rows 16 w .. 16 w + 15 = Ds W2s (K = DP); in the accumulator layout: mask, db1, dW1 (registers);
//   2 (MFMA)  dW2 tiles (16 units x 16 outputs, K = the 64 rows), dealt round-robin to the waves, accumulators persistent.
// One partial per workgroup, folded in block order by reduce_rows_kernel (api.hip).
// MFMA operand layout (lane = 16 lg + li): A[i = li][k = lg], B[k = lg][j = li], D[i = 4 lg + r][j = li].
// ---------------------------------------------------------------------------------------------
struct WgradArgs {
    long long S;
    int L, Dout;
    const float* X;      // [S][DIN][L]
    const float* dOut;   // [S][Dout][L]
    psvo_mlp w;
    float* partial;      // [gridDim.x][NP]
};

typedef float wf4 __attribute__((ext_vector_type(4)));

template <int DIN, int H, int NOT>
struct WgradLds {
    static constexpr int DP = 16 * NOT;       // padded output width
    static constexpr int LDH = H + 1, LDD = DP + 1;
    static constexpr int oW2 = 0;                     // W2s [DP][LDH]: W2s[o][k] = W2[k][o]
    static constexpr int oHs = oW2 + DP * LDH;        // [64][LDH]
    static constexpr int oDs = oHs + 64 * LDH;        // [64][LDD]
    static constexpr int oXs = oDs + 64 * LDD;        // [64][DIN]
    static constexpr int oW1 = oXs + 64 * DIN;        // W1 [DIN][H] | b1 [H]
    static constexpr int kTiles = oW1 + (DIN + 1) * H;
    static constexpr int kRed = 16 * (DIN + 1) * H;   // the final reduction reuses the buffers from 0
    static constexpr int kSize = kTiles > kRed ? kTiles : kRed;
};

template <int DIN, int H, int NOT>
__global__ void __launch_bounds__(256) mlp_wgrad_wobs_kernel(const WgradArgs a) {
    using LY = WgradLds<DIN, H, NOT>;
    constexpr int DP = LY::DP, LDH = LY::LDH, LDD = LY::LDD;
    constexpr int NCT = H / 16;                       // 16-wide tiles of the hidden units
    constexpr int NTILE = NCT * NOT;                  // dW2 tiles
    constexpr int TPW = (NTILE + 3) / 4;              // ... per wave
    constexpr int OPW = DP / 4;                       // outputs a wave stages in phase A
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* W2s = sm + LY::oW2;
    float* Hs = sm + LY::oHs;
    float* Ds = sm + LY::oDs;
    float* xs = sm + LY::oXs;
    float* w1s = sm + LY::oW1;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int Dout = a.Dout;
    const int oB1 = DIN * H, oGW2 = oB1 + H, oGB2 = oGW2 + H * Dout, NP = oGB2 + Dout;

    for (int i = tid; i < DP * H; i += 256) {
        const int o = i / H, k = i - o * H;
        W2s[o * LDH + k] = o < Dout ? a.w.W2[k * Dout + o] : 0.f;
    }
    for (int i = tid; i < DIN * H; i += 256) w1s[i] = a.w.W1[i];
    for (int i = tid; i < H; i += 256) w1s[DIN * H + i] = a.w.b1[i];

    wf4 accW2[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) accW2[t] = wf4{0.f, 0.f, 0.f, 0.f};
    float gW1[NCT][DIN], gb1[NCT], gb2[OPW];
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
        gb1[c] = 0.f;
#pragma unroll
        for (int d = 0; d < DIN; ++d) gW1[c][d] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < OPW; ++j) gb2[j] = 0.f;
    __syncthreads();

    const long long R = a.S * a.L;
    const long long nchunk = (R + 63) / 64;
    for (long long ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
        // ---- A: rows of the chunk ----------------------------------------------------------------------
        {
            const long long r = ch * 64 + lane;
            const bool in = r < R;
            const long long sgm = in ? r / a.L : 0;
            const int l = in ? (int)(r - sgm * a.L) : 0;
            float x[DIN];
#pragma unroll
            for (int d = 0; d < DIN; ++d) x[d] = in ? a.X[(sgm * DIN + d) * a.L + l] : 0.f;
            if (wave == 0) {
#pragma unroll
                for (int d = 0; d < DIN; ++d) xs[lane * DIN + d] = x[d];
            }
#pragma unroll
            for (int j = 0; j < OPW; ++j) {
                const int o = wave + 4 * j;
                const float g = (in && o < Dout) ? a.dOut[(sgm * Dout + o) * a.L + l] : 0.f;
                Ds[lane * LDD + o] = g;
                gb2[j] += g;
            }
#pragma unroll
            for (int kk = 0; kk < H / 4; ++kk) {
                const int k = wave * (H / 4) + kk;
                float pre = w1s[DIN * H + k];
#pragma unroll
                for (int d = 0; d < DIN; ++d) pre = fmaf(x[d], w1s[d * H + k], pre);
                Hs[lane * LDH + k] = fmaxf(pre, 0.f);
            }
        }
        __syncthreads();
        // ---- 1: dh = dOut W2^T for rows 16 wave .. + 15 --------------------------------------------------
        {
            wf4 acc[NCT];
#pragma unroll
            for (int c = 0; c < NCT; ++c) acc[c] = wf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k0 = 0; k0 < DP; k0 += 4) {
                const float av = Ds[(wave * 16 + li) * LDD + k0 + lg];
#pragma unroll
                for (int c = 0; c < NCT; ++c) {
                    const float bv = W2s[(k0 + lg) * LDH + c * 16 + li];
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[c], 0, 0, 0);
                }
            }
            // accumulator layout: row i = 16 wave + 4 lg + r, unit j = 16 c + li
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = wave * 16 + 4 * lg + r;
                float x[DIN];
#pragma unroll
                for (int d = 0; d < DIN; ++d) x[d] = xs[i * DIN + d];
#pragma unroll
                for (int c = 0; c < NCT; ++c) {
                    const float dpre = Hs[i * LDH + c * 16 + li] > 0.f ? acc[c][r] : 0.f;
                    gb1[c] += dpre;
#pragma unroll
                    for (int d = 0; d < DIN; ++d) gW1[c][d] = fmaf(x[d], dpre, gW1[c][d]);
                }
            }
        }
        // ---- 2: dW2 += h^T dOut over the 64 rows ----------------------------------------------------------
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int tl = wave + 4 * t;
            if (tl < NTILE) {
                const int rt = tl / NOT, ct = tl % NOT;
#pragma unroll 4
                for (int k0 = 0; k0 < 64; k0 += 4) {
                    const float av = Hs[(k0 + lg) * LDH + rt * 16 + li];      // A[i][k] = h[row k][unit i]
                    const float bv = Ds[(k0 + lg) * LDD + ct * 16 + li];
                    accW2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, accW2[t], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- the workgroup's partial ------------------------------------------------------------------------
    float* dst = a.partial + (size_t)blockIdx.x * NP;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int tl = wave + 4 * t;
        if (tl < NTILE) {
            const int rt = tl / NOT, ct = tl % NOT;
            const int o = ct * 16 + li;
            if (o < Dout) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[oGW2 + (rt * 16 + 4 * lg + r) * Dout + o] = accW2[t][r];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < OPW; ++j) {       // (uniform over the wave: the scan runs under the full mask)
        const float v = wave_sum(gb2[j]);
        const int o = wave + 4 * j;
        if (lane == 0 && o < Dout) dst[oGB2 + o] = v;
    }
    float* red = sm;     // [16 groups][DIN + 1][H]: every column sum exists once per (wave, lane group)
    const int grp = wave * 4 + lg;
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
        const int j = c * 16 + li;
        float* rg = red + (size_t)grp * (DIN + 1) * H;
#pragma unroll
        for (int d = 0; d < DIN; ++d) rg[d * H + j] = gW1[c][d];
        rg[DIN * H + j] = gb1[c];
    }
    __syncthreads();
    for (int p = tid; p < (DIN + 1) * H; p += 256) {
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) v += red[(size_t)g * (DIN + 1) * H + p];
        dst[p] = v;       // ([dW1 (DIN,H) | db1 (H)] is the layout of the first (DIN + 1) H outputs)
    }
}

template <int DIN, int H, int NOT>
static int launch_wgrad(const WgradArgs& a, int nblk, float* out, int accumulate, hipStream_t s) {
    const int NP = DIN * H + H + H * a.Dout + a.Dout;
    const size_t lds = sizeof(float) * WgradLds<DIN, H, NOT>::kSize;
    clear_hip_error();
    hipLaunchKernelGGL((mlp_wgrad_wobs_kernel<DIN, H, NOT>), dim3(nblk), dim3(256), lds, s, a);
    launch_reduce_rows(a.partial, nblk, NP, NP, out, accumulate, s);      // (workgroups in order)
    return launch_status();
}

}  // namespace wobs
}  // namespace psvo

extern "C" int psvo_filter_forward_wobs(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                        const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                                        const float* mu2, const float* m0, const float* sig0, const float* fm0,
                                        const float* fsig0, const float* obs, const float* eps, const float* u,
                                        const int32_t* idx_in, float* X, float* Xanc, float* Fm, float* P1, float* logW,
                                        int32_t* idx_out, float* lse, void* stream) {
    using namespace psvo;
    using namespace psvo::wobs;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!desc || !q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X || !Xanc || !Fm ||
        !logW || !idx_out || !lse)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f)) return PSVO_ERR_INVALID;
    if (desc->resample && !u && !idx_in) return PSVO_ERR_INVALID;
    if (!filter_shape_ok(desc)) return PSVO_ERR_UNSUPPORTED;

    FwdArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy;
    a.resample = desc->resample; a.two_q = desc->two_q; a.bootstrap = desc->bootstrap; a.emission = desc->emission;
    a.q1 = *q1; a.f = desc->bootstrap ? *q1 : *f; a.g = *g;
    a.sig_q1 = sig_q1; a.sig_q2 = sig_q2; a.sig_f = sig_f; a.sig_g = sig_g;
    a.mu2 = mu2; a.m0 = m0; a.sig0 = sig0; a.fm0 = fm0; a.fsig0 = fsig0;
    a.obs = obs; a.eps = eps; a.u = u; a.idx_in = idx_in;
    a.X = X; a.Xanc = Xanc; a.Fm = Fm; a.P1 = P1; a.logW = logW; a.idx_out = idx_out; a.lse = lse;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_fwd<dx(), h()>(a, s); });
}

extern "C" long long psvo_filter_wobs_ws_floats(int B, int T, int N, int Dx, int Dy) {
    return (long long)B * (10 * Dx + Dy) + (long long)T * B * Dx * N;
}

extern "C" int psvo_filter_backward_wobs_ext(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, int nparts,
    const float* dFm_ext, const float* dlogW_ext, float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
    float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0, float* ws, void* stream) {
    using namespace psvo;
    using namespace psvo::wobs;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!desc || !q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X || !Fm || !logW ||
        !lse || !dP || !dG || !dm0 || !dfm0 || !dsig_q1 || !dsig_q2 || !dsig_f || !dsig_g || !dsig0 || !dfsig0 || !ws)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2 || !dmu2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f || !P1 || !dF)) return PSVO_ERR_INVALID;
    if (desc->resample && !idx) return PSVO_ERR_INVALID;
    if ((dFm_ext || dlogW_ext) && nparts <= 0) return PSVO_ERR_INVALID;
    if (!filter_shape_ok(desc)) return PSVO_ERR_UNSUPPORTED;

    BwdArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy;
    a.resample = desc->resample; a.two_q = desc->two_q; a.bootstrap = desc->bootstrap; a.emission = desc->emission;
    a.q1 = *q1; a.f = desc->bootstrap ? *q1 : *f; a.g = *g;
    a.sig_q1 = sig_q1; a.sig_q2 = sig_q2; a.sig_f = sig_f; a.sig_g = sig_g;
    a.mu2 = mu2; a.m0 = m0; a.sig0 = sig0; a.fm0 = fm0; a.fsig0 = fsig0; a.obs = obs; a.eps = eps;
    a.X = X; a.Fm = Fm; a.P1 = P1; a.logW = logW; a.lse = lse; a.idx = idx; a.dlse = dlse;
    a.nparts = nparts; a.dFm_ext = dFm_ext; a.dlogW_ext = dlogW_ext;
    a.dP = dP; a.dF = dF; a.dG = dG; a.dmu2 = dmu2; a.dm0 = dm0; a.dfm0 = dfm0;
    a.sacc = ws;
    a.dm2_rows = ws + (long long)desc->B * (10 * desc->Dx + desc->Dy);
    BwdOut o{dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_bwd<dx(), h()>(a, o, s); });
}

extern "C" int psvo_filter_backward_wobs(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, float* dP, float* dF,
    float* dG, float* dmu2, float* dm0, float* dfm0, float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g,
    float* dsig0, float* dfsig0, float* ws, void* stream) {
    return psvo_filter_backward_wobs_ext(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, X, Fm,
                                         P1, logW, lse, idx, dlse, 0, nullptr, nullptr, dP, dF, dG, dmu2, dm0, dfm0, dsig_q1,
                                         dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, ws, stream);
}

extern "C" int psvo_mlp_wgrad_wobs_blocks(long long rows) {
    long long nb = (rows + 64 * 4 - 1) / (64 * 4);   // >= 4 chunks of 64 rows per workgroup amortise the final reduction
    if (nb < 1) nb = 1;
    if (nb > 512) nb = 512;
    return (int)nb;
}

extern "C" int psvo_mlp_wgrad_wobs(long long S, int L, int Din, int H, int Dout, const float* X, const float* dOut,
                                   const psvo_mlp* w, float* partial, float* grad, int accumulate, void* stream) {
    using namespace psvo;
    using namespace psvo::wobs;
    if (!X || !dOut || !w || !partial || !grad || S <= 0 || L <= 0) return PSVO_ERR_INVALID;
    if (Dout < 3 || Dout > kMaxDy) return PSVO_ERR_UNSUPPORTED;
    WgradArgs a{S, L, Dout, X, dOut, *w, partial};
    const int nblk = psvo_mlp_wgrad_wobs_blocks(S * L);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return pick<1, 2, 3, 4>(Din, [&](auto din) {
        return pick_h(H, [&](auto h) {
            return Dout <= 16 ? launch_wgrad<din(), h(), 1>(a, nblk, grad, accumulate, s)
                              : launch_wgrad<din(), h(), 2>(a, nblk, grad, accumulate, s);
        });
    });
}
