// The two wide-observation filter kernels.  filter_wobs.hip includes this file four times: PSVO_AD = 0 (and PSVO_MS = 0) gives
// filter_fwd_wobs_kernel and filter_bwd_wobs_kernel, text and code as they always were; PSVO_AD = 1 gives filter_fwd_wobs_ad_kernel
// and filter_bwd_wobs_ad_kernel, the kernels of psvo_filter_forward_wobs_adaptive / psvo_filter_backward_wobs_adaptive; PSVO_MS = 1
// gives the missing-observation pair, and both together the adaptive missing-observation pair (below).  filter_wobs_in.hip includes it
// a fifth time: PSVO_IN = 1 on top of PSVO_MS = 1, the input-driven pair (below).
//
// Adaptive resampling (filter_fwd_impl.h / filter_bwd_impl.h have the definition; it is the same here): the draw is made and
// written every step, and the sequence INHERITS it only when ESS = (sum w)^2 / sum w^2 has fallen below ess_frac N (or when
// rs_in says so).  Forward: sum w^2 is one more per-wave sum beside the scan's wave totals, behind the same barrier; every lane
// adds the same LDS words in the same order, and the decision only feeds selects.  Reverse: the decisions rs (T,B) are constants
// like the indices, read as scalars; the ancestor of particle n at step t is rs[t-1] ? idx[t-1][n] : n, and the term of the
// carried normalised weight (`!a.resample` in the static kernel) is applied at exactly the steps with rs[t] == 0.
//
// Missing observations (PSVO_MS = 1, PSVO_AD = 0: filter_fwd_wobs_ms_kernel / filter_bwd_wobs_ms_kernel, the kernels of
// psvo_filter_forward_wobs_missing / psvo_filter_backward_wobs_missing): a NaN in obs is an observation that was not made, and its
// term is left out of log g.  y_t[e] is a broadcast, so o_e = (y == y) is the same in every lane; it only feeds selects.  The
// normalising constant of the Gaussian forms is no longer one number per launch: c_e = -(log sig_g[e] + 1/2 log 2 pi) is an LDS row
// beside 1 / sig_g and a step adds the c_e of what it observed.  Reverse: the d G row of a missing entry is written as 0 (the
// weight gradient and bwd_input read it back) and the d sig_g column receives nothing.  Same argument blocks as the static pair.
//
// Both (PSVO_AD = 1 and PSVO_MS = 1: filter_fwd_wobs_msad_kernel / filter_bwd_wobs_msad_kernel, the kernels of
// psvo_filter_forward_wobs_missing_adaptive / psvo_filter_backward_wobs_missing_adaptive): the two sets of lines do not touch each
// other, and the semantics are the intersection of the two definitions above -- ESS is taken from the weights as the observed
// terms left them, so a step with nothing observed (log g = 0 exactly) that follows a resampled step of a bootstrap filter
// without q2 has ESS = N and is kept.  The adaptive argument blocks; the LDS of the missing-observation form: the adaptive form's
// red[40 + wave], wave <= 7, ends at red[47], the last of the 48 floats ahead of the cg row (the log-factorial rows for counts).
//
// Exogenous inputs (PSVO_IN = 1 on top of PSVO_MS = 1, PSVO_AD = 0; filter_wobs_in.hip: filter_fwd_wobs_in_kernel /
// filter_bwd_wobs_in_kernel, the kernels of psvo_filter_forward_wobs_input / psvo_filter_backward_wobs_input): the first layer of
// MLP_q1 / MLP_f is applied to concat[x_t, v_t], and the input's share hb[t,b,:] = v[b,t,:] W1[Dx:] of the hidden pre-activation is
// the same for every particle.  The kernels keep the EFFECTIVE bias row b1 + hb[t,b,:] of the step (one fp32 add, made by the lane
// that stages the word) in a two-row LDS buffer hbuf[2][2 H] (q1 | f), the pattern of ybuf: the words of the next step's row are
// requested while this step computes -- lane tid takes word tid and, where a single wave stages 2 H = 128 words, word tid + NT --
// and land in the half that the step BEFORE this one read, ahead of the step's own stores and of the barrier that ends it.  Nothing of step t reads
// that half, so neither the IWAE reverse step (no barrier between bwd_input and the end of the step) nor a one-wave forward
// step (block_max has no barrier at nw == 1) can see a row replaced under it; no barrier is added.  Every MQ::eval<true> /
// MQ::bwd_input<true> of step t reads the row of step t (RowBias in row_bias.h: the same operations, the bias words
// taken from the row).
//
// All three (PSVO_IN = 1, PSVO_MS = 1 and PSVO_AD = 1; filter_wobs_inad.hip: filter_fwd_wobs_inad_kernel / filter_bwd_wobs_inad_kernel,
// the kernels of psvo_filter_forward_wobs_input_adaptive / psvo_filter_backward_wobs_input_adaptive): a sixth compilation and no new
// line.  The two sets of lines do not touch: the adaptive form's red[40 + wave] ends at red[47] and hbuf starts behind
// red + 48 + 2 kMaxDy (forward), behind the d sig_g columns (reverse); the decision feeds selects and, in the reverse pass, scalar
// branches around the gather, none of which holds a read or a store of hbuf; and every barrier of the input form is taken at
// every step of the adaptive form too (block_sum's under `!rs_here` by every wave or by none).  The semantics are the
// intersection of the two definitions: ESS from the weights as they are, the draw made and written every step, rs a constant of
// the reverse pass, the rows d P / d F left for psvo_mlp_wgrad_rowbias.  The argument blocks are the adaptive ones with the bias
// rows behind them (filter_wobs_args.h).
#if PSVO_IN && PSVO_AD
#define PSVO_WOBS_FWD_KERNEL filter_fwd_wobs_inad_kernel
#define PSVO_WOBS_BWD_KERNEL filter_bwd_wobs_inad_kernel
#define PSVO_WOBS_FWD_ARGS FwdArgsInAd
#define PSVO_WOBS_BWD_ARGS BwdArgsInAd
#elif PSVO_IN
#define PSVO_WOBS_FWD_KERNEL filter_fwd_wobs_in_kernel
#define PSVO_WOBS_BWD_KERNEL filter_bwd_wobs_in_kernel
#define PSVO_WOBS_FWD_ARGS FwdArgsIn
#define PSVO_WOBS_BWD_ARGS BwdArgsIn
#elif PSVO_AD && PSVO_MS
#define PSVO_WOBS_FWD_KERNEL filter_fwd_wobs_msad_kernel
#define PSVO_WOBS_BWD_KERNEL filter_bwd_wobs_msad_kernel
#define PSVO_WOBS_FWD_ARGS FwdArgsAd
#define PSVO_WOBS_BWD_ARGS BwdArgsAd
#elif PSVO_AD
#define PSVO_WOBS_FWD_KERNEL filter_fwd_wobs_ad_kernel
#define PSVO_WOBS_BWD_KERNEL filter_bwd_wobs_ad_kernel
#define PSVO_WOBS_FWD_ARGS FwdArgsAd
#define PSVO_WOBS_BWD_ARGS BwdArgsAd
#elif PSVO_MS
#define PSVO_WOBS_FWD_KERNEL filter_fwd_wobs_ms_kernel
#define PSVO_WOBS_BWD_KERNEL filter_bwd_wobs_ms_kernel
#define PSVO_WOBS_FWD_ARGS FwdArgs
#define PSVO_WOBS_BWD_ARGS BwdArgs
#else
#define PSVO_WOBS_FWD_KERNEL filter_fwd_wobs_kernel
#define PSVO_WOBS_BWD_KERNEL filter_bwd_wobs_kernel
#define PSVO_WOBS_FWD_ARGS FwdArgs
#define PSVO_WOBS_BWD_ARGS BwdArgs
#endif

// ---------------------------------------------------------------------------------------------
// Forward filter: lane = particle, workgroup = sequence, t in-kernel (filter_fwd.hip's lane-per-particle kernel with the
// emission walked over a run-time Dy).  Same outputs and draw rule: idx = #{k : cdf[k] <= u * total}, clamped to N - 1.
// ---------------------------------------------------------------------------------------------
// CNT: the count emission (psvo_desc.emission = 2), a compile-time form so that the Gaussian / unit-normal instantiations keep
// their code and registers.  1 / sig_g is not used; the log-factorial row of a step travels with its observation row.
template <int DX, int H, bool CNT>
__global__ void __launch_bounds__(512) PSVO_WOBS_FWD_KERNEL(const PSVO_WOBS_FWD_ARGS a) {
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
#if PSVO_MS
    float* cg = red + 48;               // !CNT (no lfbuf then): [kMaxDy] -(log sig_g + 1/2 log 2 pi), the constant of one term
#endif
#if PSVO_IN
    using RB = RowBias<DX, H>;
    float* hbuf = red + 48 + 2 * kMaxDy;        // [2][2 H] effective bias rows (q1 | f) of step t (t & 1) and t + 1; 16-byte aligned
    const int NB = a.bootstrap ? H : 2 * H;     // words of a row that are staged
#endif

    MQ::load(wq1, a.q1, tid, NT);
    if (!a.bootstrap) MQ::load(wf, a.f, tid, NT);
    MG::load(wg, a.g, Dy, tid, NT);
    const float* wfm = a.bootstrap ? wq1 : wf;
    if (tid < Dy) {
        if constexpr (!CNT) isg[tid] = 1.f / a.sig_g[tid];
#if PSVO_MS
        if constexpr (!CNT) cg[tid] = -(logf(a.sig_g[tid]) + kHalfLog2Pi);
#endif
        const float y0 = a.obs[(size_t)b * Dy + tid];
        ybuf[tid] = y0;
        if constexpr (CNT) lfbuf[tid] = log_factorial(y0);
    }
#if PSVO_IN
    for (int i = tid; i < NB; i += NT) {        // the row of step 0, b1 from HBM (the images are not visible yet)
        const int k = i & (H - 1);
        hbuf[i] = i >= H ? a.f.b1[k] + a.hb_f[(size_t)b * H + k] : a.q1.b1[k] + a.hb_q1[(size_t)b * H + k];
    }
#endif

    float sq1[DX], sq2[DX], sfv[DX], s0[DX], fs0[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        sq1[d] = a.sig_q1[d];
        sq2[d] = a.two_q ? a.sig_q2[d] : 1.f;
        sfv[d] = a.bootstrap ? a.sig_q1[d] : a.sig_f[d];
        s0[d] = a.sig0[d];
        fs0[d] = a.fsig0[d];
    }
#if !PSVO_MS
    float lg = -Dy * kHalfLog2Pi;
    if constexpr (!CNT) {
        for (int e = 0; e < Dy; ++e) lg -= logf(a.sig_g[e]);
    }
#endif
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
#if PSVO_AD
        // (the four adaptive arguments are plain fields: re-read from the kernel arguments at their point of use -- common.h:
        //  PSVO_ARG -- they halve the scalar spills but put three count instantiations into scratch)
        int rs_f = 0;         // the teacher-forced decision of this step, requested ahead of its use
        if (a.rs_in) rs_f = a.rs_in[tb];
#endif
        int zo = 0;
        asm volatile("" : "+v"(zo));        // weights are re-read from LDS every step, never hoisted into registers
        const float* wq1_t = wq1 + zo;
        const float* wfm_t = wfm + zo;
        const float* wg_t = wg + zo;
        const float* y_t = ybuf + (t & 1) * kMaxDy + zo;

        float eps_n[DX], mu2_n[DX], u_n = 0.f, y_n = 0.f;
        int idx_n = 0;
#if PSVO_IN
        float hb_n[2] = {0.f, 0.f};         // words tid and tid + NT of the next step's row (NT >= 64, 2 H <= 128)
#endif
        if (t + 1 < T) {
            load_inputs(t + 1, eps_n, mu2_n, u_n, idx_n);
            if (tid < Dy) y_n = a.obs[(tb + B) * Dy + tid];
#if PSVO_IN
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = tid + j * NT;
                if (i < NB) hb_n[j] = (i >= H ? a.hb_f : a.hb_q1)[(tb + B) * H + (i & (H - 1))];
            }
#endif
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
#if PSVO_MS
            // observed terms only, constant included, in the order e = 0 .. Dy - 1; nothing observed: exactly 0
            if constexpr (CNT) {
                const float* lf_t = lfbuf + (t & 1) * kMaxDy + zo;
#pragma unroll 1
                for (int e = 0; e < Dy; ++e) {
                    const float y = y_t[e];
                    const float term = count_term(y, MG::out(wg_t, e, h)) - lf_t[e];
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
#endif
        }
        float lw = f_lp + g_lp - q_lp + lnw;
        if (!valid) lw = ninf;

        // ---- next-step proposal / transition means of every pre-resampling particle -----------
        float p1[DX], fm[DX];
#if PSVO_IN
        const float* hb_t = hbuf + (t & 1) * 2 * H + zo;        // b1 + hb[t] of MLP_q1, then of MLP_f
        RB::eval(wq1_t, hb_t, x, p1);
        if (a.bootstrap) {
#pragma unroll
            for (int d = 0; d < DX; ++d) fm[d] = p1[d];
        } else {
            RB::eval(wfm_t, hb_t + H, x, fm);
        }
        // the prefetched bias row: b1 (the image's word) + hb, into the half that step t - 1 read.  Here, ahead of the step's
        // stores: the words were requested before the emission loop and have landed, and a wait for them placed behind the
        // stores would wait for the stores as well (vmcnt counts both, and the count is not exact across the branches below)
        if (t + 1 < T) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = tid + j * NT;
                if (i < NB) hbuf[((t + 1) & 1) * 2 * H + i] = (i >= H ? wf : wq1)[MQ::kB1 + (i & (H - 1))] + hb_n[j];
            }
        }
#else
        MQ::template eval<true>(wq1_t, x, p1);
        if (a.bootstrap) {
#pragma unroll
            for (int d = 0; d < DX; ++d) fm[d] = p1[d];
        } else {
            MQ::template eval<true>(wfm_t, x, fm);
        }
#endif
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
#if PSVO_AD
        float tot2 = wave_sum(w * w);       // (w is relative to the workgroup's maximum already)
#endif
        if (nw > 1) {
            float* wt = red + 32;
            if (lane == 63) wt[wave] = sc;
#if PSVO_AD
            if (lane == 63) red[40 + wave] = tot2;      // (nw <= 8: block_max has red[0..7], the wave totals red[32..39])
#endif
            __syncthreads();
            float off = 0.f, tot = 0.f;
            for (int i = 0; i < nw; ++i) {
                const float v = wt[i];
                if (i < wave) off += v;
                tot += v;
            }
            sc += off;
            total = tot;
#if PSVO_AD
            tot2 = 0.f;
            for (int i = 0; i < nw; ++i) tot2 += red[40 + i];          // wave order, the same in every lane
#endif
        } else {
            total = lane_bcast(sc, 63);
        }
        const float lse_t = fmaf(kLn2, log2_fast(total), mx);
        if (tid == 0) a.lse[tb] = lse_t;
#if PSVO_AD
        const float ess = total * total / tot2;
        const bool inherit = a.rs_in ? (rs_f != 0) : !(ess >= a.ess_frac * (float)N);      // (a NaN ESS resamples)
        if (tid == 0) {
            a.ess_out[tb] = ess;
            a.rs_out[tb] = inherit ? 1 : 0;
        }
#endif

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
#if PSVO_AD
            // balanced weights: the particle keeps its own means and carries its normalised weight into the next step
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                mean1[d] = inherit ? mean1[d] : p1[d];
                fmean[d] = inherit ? fmean[d] : fm[d];
            }
            lnw = inherit ? neg_logN : lw - lse_t;
#endif
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

// ---------------------------------------------------------------------------------------------
// Reverse filter (filter_bwd.hip's persistent kernel; upstream gradients: d lse and, through the _ext entry point, d Fm / d logW).  One workgroup per sequence walks
// t = T-1 .. 0.  What step t leaves for step t-1 is D[n] = d loss / d (MLP_q1(x_{t-1}[n]), MLP_f(x_{t-1}[n])), carried in the
// parent's own registers: the children stage (ancestor, values) in LDS and every parent adds its children in child order.
// Per-sequence sums (common.h: FAcc): [2 sets x 5 Dx | Dy].
// ---------------------------------------------------------------------------------------------
// CNT: the count emission (as in the forward kernel); its d G rows are dlw (y / lam - 1) sigmoid(r), there is no d sig_g
template <int DX, int H, bool EXT, bool CNT>
__global__ void __launch_bounds__(512) PSVO_WOBS_BWD_KERNEL(const PSVO_WOBS_BWD_ARGS a) {
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
#if PSVO_IN
    using RB = RowBias<DX, H>;
    float* hbuf = sg + Dy * NT;         // [2][2 H] effective bias rows (q1 | f) of step t (t & 1) and t - 1; 16-byte aligned
    float* kst = hbuf + 4 * H;          // [2][5 DX] step constants, as below
    const int NB = a.bootstrap ? H : 2 * H;
#else
    float* kst = sg + Dy * NT;          // [2][5 DX] step constants c | 1/c | 1/s1 | 1/s2 | 1/fs of t = 0 and of t >= 1
#endif

    MQ::load(wq1, a.q1, tid, NT);
    if (!a.bootstrap) MQ::load(wf, a.f, tid, NT);
    MG::load(wg, a.g, Dy, tid, NT);
    const float* wfm = a.bootstrap ? wq1 : wf;
    if (tid < Dy) {
        if constexpr (!CNT) isg[tid] = 1.f / a.sig_g[tid];
        ybuf[((T - 1) & 1) * kMaxDy + tid] = a.obs[((size_t)(T - 1) * B + b) * Dy + tid];
    }
#if PSVO_IN
    for (int i = tid; i < NB; i += NT) {        // the row of step T - 1, b1 from HBM (the images are not visible yet)
        const int k = i & (H - 1);
        const size_t r = ((size_t)(T - 1) * B + b) * H + k;
        hbuf[((T - 1) & 1) * 2 * H + i] = i >= H ? a.f.b1[k] + a.hb_f[r] : a.q1.b1[k] + a.hb_q1[r];
    }
#endif
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
#if PSVO_AD
        // the decisions of this step and of the one before it, read through the constant address space at a wave-uniform address:
        // scalar loads into SGPRs, the same word in every wave of the workgroup.  The pointer is re-read from the kernel
        // arguments (as the _ext pointers are) and not held across the time loop.
        const rs_word_t* rs_seq = (const rs_word_t*)arg_rs() + b;
        const bool rs_here = __builtin_amdgcn_readfirstlane(rs_seq[(size_t)t * B]) != 0;
        const bool rs_prev = first || __builtin_amdgcn_readfirstlane(rs_seq[(size_t)(t - 1) * B]) != 0;
#endif

        float y_n = 0.f;
        if (t >= 1 && tid < Dy) {       // next step's observation row, in flight during this one
            if constexpr (CNT) y_n = PSVO_ARG(BwdArgs, obs)[(tb - B) * Dy + tid];      // (see dlse below)
            else y_n = a.obs[(tb - B) * Dy + tid];
        }
#if PSVO_IN
        float hb_n[2] = {0.f, 0.f};         // words tid and tid + NT of the row of step t - 1, in flight during this step
        if (t >= 1) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = tid + j * NT;
                if (i < NB) hb_n[j] = (i >= H ? a.hb_f : a.hb_q1)[(tb - B) * H + (i & (H - 1))];
            }
        }
#endif

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
#if PSVO_AD
        if (!rs_here) {         // lnw[t+1] = lw[t] - lse[t]; a scalar: block_sum's barriers are taken by every wave or by none
#else
        if (!a.resample) {
#endif
            const float tot = block_sum(dlnw, red, wave, lane, nw);
            dlw += dlnw - sm * tot;
        }
        if (!valid) dlw = 0.f;
        dlnw = first ? 0.f : dlw;
#if PSVO_IN
        // the row of step t - 1 goes to the half that step t + 1 read: an IWAE step has no barrier between bwd_input and the end
        // of the step, and waves still inside this step's bwd_input read the other half.  Here, ahead of the step's first store:
        // the words were requested before x and logW, which have just been waited for, and a wait placed behind the stores of
        // the emission loop would wait for those as well
        if (t >= 1) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = tid + j * NT;
                if (i < NB) hbuf[((t - 1) & 1) * 2 * H + i] = (i >= H ? wf : wq1)[MQ::kB1 + (i & (H - 1))] + hb_n[j];
            }
        }
#endif

        // ---- emission: outputs in the order o = 0 .. Dy - 1 -----------------------------------------------
        float dx[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) dx[d] = 0.f;
        {
            float h[H];
            MG::hidden(wg_t, x, h);
#if PSVO_MS
            // a missing entry: its d G row is written as 0 (it is read back), its d sig_g column gets nothing
            if constexpr (CNT) {
#pragma unroll 1
                for (int o = 0; o < Dy; ++o) {
                    const float y = y_t[o];
                    const float dr = dlw * count_dterm(y, MG::out(wg_t, o, h));
                    if (valid) a.dG[(tb * Dy + o) * N + n] = (y == y) ? dr : 0.f;
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
                    sg[o * NT + tid] += ob ? dlw * (z * z - 1.f) * is : 0.f;
                    if (valid) a.dG[(tb * Dy + o) * N + n] = ob ? dlw * z * is * dmean : 0.f;
                }
            }
#else
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
#endif
        }
        // (second walk over the outputs: the lane reads its own d G rows back -- H partial sums beside the H activations
        //  would not fit the 256 registers of a 512-lane workgroup)
        MG::template bwd_input<(H >= 64 ? 32 : 16)>(wg_t, Dy, a.dG + (tb * Dy) * N + n, (size_t)N, valid, x, dx);
        // ---- the rest of the step's forward quantities (loaded here: not live across the emission loop) ------
        int anc = n;
#if PSVO_AD
        if (t >= 1 && rs_prev) anc = min(max(a.idx[tp * N + n], 0), N - 1);      // (a kept step: the particle is its own parent)
#else
        if (t >= 1 && a.resample) anc = min(max(a.idx[tp * N + n], 0), N - 1);
#endif
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
#if PSVO_IN
        {
            const float* hb_t = hbuf + (t & 1) * 2 * H + zo;        // the relu masks of step t: b1 + hb[t]
            RB::bwd_input(wq1_t, hb_t, x, dPn, dx);
            if (!a.bootstrap) RB::bwd_input(wfm_t, hb_t + H, x, dFn, dx);
        }
#else
        MQ::template bwd_input<true>(wq1_t, x, dPn, dx);
        if (!a.bootstrap) MQ::template bwd_input<true>(wfm_t, x, dFn, dx);
#endif

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
#if PSVO_AD
            // (a kept step has no gather to reverse: it skips the staging and the O(N) walk over the children, on a scalar
            //  branch; the barrier between the two stays outside it, taken at every step)
            if (rs_prev) {
#else
            if (a.resample) {
#endif
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
#if PSVO_AD
            }
            __syncthreads();
            if (rs_prev) {
#else
                __syncthreads();
#endif
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

#undef PSVO_WOBS_FWD_KERNEL
#undef PSVO_WOBS_BWD_KERNEL
#undef PSVO_WOBS_FWD_ARGS
#undef PSVO_WOBS_BWD_ARGS
