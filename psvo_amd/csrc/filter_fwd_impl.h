// The two forward-filter kernels.  filter_fwd.hip includes this file twice: PSVO_AD = 0 gives filter_fwd_kernel and
// filter_fwd_lpp_kernel, text and code as they always were; PSVO_AD = 1 gives filter_fwd_ad_kernel and filter_fwd_lpp_ad_kernel,
// the kernels of psvo_filter_forward_adaptive.
//
// Adaptive resampling (not in the reference): the draw is made and written every step, and the sequence INHERITS it only when its
// effective sample size ESS = (sum w)^2 / sum w^2 has fallen below ess_frac N (or when rs_in says so).  sum w^2 is one more per-wave
// sum beside the scan's wave totals, through the same LDS exchange and barrier; every lane adds the same LDS words in the same
// order, so the decision is the same in the whole workgroup -- and it only feeds selects: the barriers of the step are taken by
// every lane whatever it is.
#if PSVO_AD
#define PSVO_FWD_KERNEL filter_fwd_ad_kernel
#define PSVO_FWD_LPP_KERNEL filter_fwd_lpp_ad_kernel
#define PSVO_FWD_ARGS FilterArgsAd
#else
#define PSVO_FWD_KERNEL filter_fwd_kernel
#define PSVO_FWD_LPP_KERNEL filter_fwd_lpp_kernel
#define PSVO_FWD_ARGS FilterArgs
#endif

// EM: emission variant fixed at compile time (0 / 1) or read from the arguments (2).  The one-wave-per-SIMD build
// (MAXT = 256) keeps every MLP weight in VGPRs only without the extra branch in its time loop, so it is compiled both ways.
template <int DX, int DY, int H, int MAXT, int EM = 2>
__global__ void __launch_bounds__(MAXT) PSVO_FWD_KERNEL(const PSVO_FWD_ARGS a) {
    using MQ = MlpLds<DX, H, DX, PSVO_L>;
    using MG = MlpLds<DX, H, DY, PSVO_L>;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = blockDim.x, nw = NT >> 6;
    const int b = blockIdx.x, B = a.B, T = a.T, N = a.N;
    const bool valid = tid < N;
    const int n = valid ? tid : N - 1;  // clamp so that loads stay in bounds

    float* wq1 = smem;
    float* wf = wq1 + MQ::kSize;
    float* wg = wf + MQ::kSize;
    float* cdf = wg + MG::kSize;
    float* sx = cdf + NT;          // [DX][NT] staged X_t
    float* sp = sx + DX * NT;      // [DX][NT] staged MLP_q1(X_t)
    float* sf = sp + DX * NT;      // [DX][NT] staged MLP_f(X_t) (== sp when bootstrap)
    float* red = sf + DX * NT;     // 48 floats scratch

    MQ::load(wq1, a.q1, tid, NT);
    if (!a.bootstrap) MQ::load(wf, a.f, tid, NT);
    MG::load(wg, a.g, tid, NT);
    const float* wfm = a.bootstrap ? wq1 : wf;

    // step constants: t = 0 uses (q0, sigma_q0) for the first proposal term
    float sq1[DX], sq2[DX], sfv[DX], s0[DX], fs0[DX], isg[DY];
    float lg = -DY * kHalfLog2Pi;
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        sq1[d] = a.sig_q1[d];
        sq2[d] = a.two_q ? a.sig_q2[d] : 1.f;
        sfv[d] = a.bootstrap ? a.sig_q1[d] : a.sig_f[d];
        s0[d] = a.sig0[d];
        fs0[d] = a.fsig0[d];
    }
#pragma unroll
    for (int e = 0; e < DY; ++e) {
        const float s = a.sig_g[e];
        isg[e] = 1.f / s;
        lg -= logf(s);
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
    float eps_c[DX], mu2_c[DX], obs_c[DY], u_c = 0.f;
    int idx_c = 0;
    auto load_inputs = [&](int t, float (&e)[DX], float (&m)[DX], float (&o)[DY], float& uu, int& ii) {
        const size_t tb = (size_t)t * B + b;
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            e[d] = a.eps[(tb * DX + d) * N + n];
            m[d] = a.two_q ? a.mu2[tb * DX + d] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) o[k] = a.obs[tb * DY + k];
        if (a.resample) {
            if (a.idx_in) ii = a.idx_in[tb * N + n];
            else uu = a.u[tb * N + n];
        }
    };
    load_inputs(0, eps_c, mu2_c, obs_c, u_c, idx_c);
    __syncthreads();  // weights visible

    // Weights are loop-invariant LDS reads: when they fit the register budget the compiler keeps
    // them all resident in VGPRs (no LDS traffic in the MLPs); otherwise make the LDS offset
    // opaque per step so they are re-read as broadcasts instead of being spilled to scratch.
    constexpr int kWeights = MQ::kSize + MG::kSize;
    constexpr bool kOpaque = (MAXT > 256) ? (kWeights > 120) : (kWeights > 330);

    SEC_INIT(filter_fwd)
    for (int t = 0; t < T; ++t) {
        SEC(0);
        const size_t tb = (size_t)t * B + b;
        const StepK<DX> K = (t == 0) ? K0 : K1;
#if PSVO_AD
        int rs_f = 0;         // the teacher-forced decision of this step, requested ahead of its use
        if (a.rs_in) rs_f = a.rs_in[tb];
#endif
        int zo = 0;
        if (kOpaque) asm volatile("" : "+v"(zo));
        const float* wq1_t = wq1 + zo;
        const float* wfm_t = wfm + zo;
        const float* wg_t = wg + zo;

        float eps_n[DX], mu2_n[DX], obs_n[DY], u_n = 0.f;
        int idx_n = 0;
        if (t + 1 < T) load_inputs(t + 1, eps_n, mu2_n, obs_n, u_n, idx_n);

        SEC(1);   // issue of the prefetch loads
        // ---- proposal: product of two diagonal Gaussians on *scales* (SVO.py:186-197) ----------
        float mu[DX], x[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            mu[d] = a.two_q ? K.c[d] * fmaf(K.i1[d], mean1[d], K.i2[d] * mu2_c[d]) : mean1[d];
            x[d] = fmaf(K.c[d], eps_c[d], mu[d]);
        }
        const float q_lp = diag_lp<DX>(x, mu, K.ic, K.lq);
        const float f_lp = diag_lp<DX>(x, fmean, K.ifs, K.lf);

        SEC(2);   // proposal, q / f densities
        // ---- emission ------------------------------------------------------------------------
        float gm[DY];
        MG::template eval<kOpaque>(wg_t, x, gm);
        if (EM == 2 ? (a.emission != 0) : (EM == 1)) {
#pragma unroll
            for (int k = 0; k < DY; ++k) gm[k] = emis_mean(gm[k]);
        }
        const float g_lp = diag_lp<DY>(obs_c, gm, isg, lg);

        float lw = f_lp + g_lp - q_lp + lnw;
        if (!valid) lw = ninf;

        SEC(3);   // MLP_g, weight
        // ---- next-step proposal / transition means of every pre-resampling particle -----------
        float p1[DX], fm[DX];
        MQ::template eval<kOpaque>(wq1_t, x, p1);
        if (a.bootstrap) {
#pragma unroll
            for (int d = 0; d < DX; ++d) fm[d] = p1[d];
        } else {
            MQ::template eval<kOpaque>(wfm_t, x, fm);
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

        SEC(4);   // MLP_q1 (/ MLP_f), history stores
        // ---- log-sum-exp over particles and multinomial ancestors (SVO.py:266-300) -------------
        const float mx = block_max(lw, red, 0, wave, lane, nw);
        const float w = valid ? exp2_fast((lw - mx) * kLog2e) : 0.f;
        float sc = wave_incl_scan(w, lane);
        float total;
#if PSVO_AD
        float tot2 = wave_sum(w * w);
#endif
        if (nw > 1) {
            float* wt = red + 32;
            if (lane == 63) wt[wave] = sc;
#if PSVO_AD
            if (lane == 63) red[16 + wave] = tot2;      // (the second slot of block_max: not used by this kernel)
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
            for (int i = 0; i < nw; ++i) tot2 += red[16 + i];          // wave order, the same in every lane
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

        SEC(5);   // block max, exp, scan, total
        if (a.resample) {
            cdf[tid] = sc;
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                sx[d * NT + tid] = x[d];
                sp[d * NT + tid] = p1[d];
                if (!a.bootstrap) sf[d * NT + tid] = fm[d];
            }
            __syncthreads();
            SEC(6);   // stage particles / CDF in LDS + barrier
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
            SEC(7);   // CDF search, gather, ancestor stores
            __syncthreads();  // staged tiles are rewritten next step
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
            if (nw > 1) __syncthreads();  // red[] reuse
        }

#pragma unroll
        for (int d = 0; d < DX; ++d) {
            eps_c[d] = eps_n[d];
            mu2_c[d] = mu2_n[d];
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) obs_c[k] = obs_n[k];
        u_c = u_n;
        idx_c = idx_n;
    }
}

// ---------------------------------------------------------------------------------------------
// Four lanes per particle (N <= 256).  The filter runs ONE workgroup per sequence, so a step is a pure
// latency chain; with lane = particle the two dependent MLP evaluations were > 40 % of it.  Here particle
// n owns the quad of lanes 4n..4n+3: lane p evaluates hidden units [p*H/4, (p+1)*H/4) of every MLP and the
// outputs are summed over the quad with two DPP adds.  With one hidden layer the lane's slice of the weights is
// read from LDS ONCE, behind the barrier that makes the weights visible, into registers (MlpLds::Slice): read
// through the LDS pointer inside the time loop it was re-read every step -- the image shares the LDS array the
// step stores into, and across a barrier hipcc cannot take it for unchanged (18 ds_read_b128 per step at C*).
// MLP_f's slice joins the other two where the three fit (kSliceBudget); the two-layer MLP reads LDS.
// Everything else is computed redundantly in the four lanes; the multinomial search is a
// two-round 16-ary search in which the quad reads 16 CDF pivots / 16 CDF entries as four float4 per round.
// The per-sequence log-sum-exp and CDF use per-wave maxima and ONE barrier.
// ---------------------------------------------------------------------------------------------
template <int DX, int DY, int H, int MAXT>
__global__ void __launch_bounds__(MAXT) PSVO_FWD_LPP_KERNEL(const PSVO_FWD_ARGS a) {
    using MQ = MlpLds<DX, H, DX, PSVO_L>;
    using MG = MlpLds<DX, H, DY, PSVO_L>;
    constexpr int P = 4;
    using SG = typename MlpLds<DX, H, DY, 1>::template Slice<P>;
    using SQ = typename MlpLds<DX, H, DX, 1>::template Slice<P>;
    // which slices are held in registers (one hidden layer only: the H x H layer of two reads its operands from LDS as the
    // matrix instructions want them).  MLP_g and MLP_q1 wherever the build stays within 256 VGPRs, without scratch and without
    // one more spilled register than it had: that leaves out Dx = 4 and the adaptive kernels at Dy = 2, which gain spilled
    // SGPRs -- their slices stay in LDS and are read there each step, as before.  MLP_f, evaluated without bootstrap only,
    // joins where all three stay inside kSliceBudget floats (above it: more than the 256 registers of two waves per SIMD).
    constexpr int kSliceBudget = 120;
    constexpr bool kRegGQ = PSVO_L == 1 && DX <= 3 && !(PSVO_AD && DY == 2);
    constexpr bool kRegF = kRegGQ && SG::kFloats + 2 * SQ::kFloats <= kSliceBudget;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = blockDim.x, nw = NT >> 6;
    const int NPT = NT / P;                       // particle slots, a multiple of 16
    const int b = blockIdx.x, B = a.B, T = a.T, N = a.N;
    const int pn = tid >> 2, p = tid & 3;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);   // wave index as a scalar
    const bool valid = pn < N;
    const int n = valid ? pn : N - 1;

    float* wq1 = smem;
    float* wf = wq1 + MQ::kSize;
    float* wg = wf + MQ::kSize;
    float* cdf = wg + MG::kSize;   // [NPT]
    float* piv = cdf + NPT;        // [16] cdf[16 i + 15], +inf beyond the last block
    float* sx = piv + 16;          // [DX][NPT] staged X_t
    float* sp = sx + DX * NPT;     // [DX][NPT] staged MLP_q1(X_t)
    float* sf = sp + DX * NPT;     // [DX][NPT] staged MLP_f(X_t) (unused when bootstrap)
    float* red = sf + DX * NPT;    // [2][16] per-wave (max, sum); adaptive: [3][16], + the sum of squares

    MQ::load(wq1, a.q1, tid, NT);
    if (!a.bootstrap) MQ::load(wf, a.f, tid, NT);
    MG::load(wg, a.g, tid, NT);
    const float* wfm = a.bootstrap ? wq1 : wf;
    if (tid < 16) piv[tid] = __builtin_huge_valf();

    float sq1[DX], sq2[DX], sfv[DX], s0[DX], fs0[DX], isg[DY];
    float lg = -DY * kHalfLog2Pi;
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        sq1[d] = a.sig_q1[d];
        sq2[d] = a.two_q ? a.sig_q2[d] : 1.f;
        sfv[d] = a.bootstrap ? a.sig_q1[d] : a.sig_f[d];
        s0[d] = a.sig0[d];
        fs0[d] = a.fsig0[d];
    }
#pragma unroll
    for (int e = 0; e < DY; ++e) {
        const float s = a.sig_g[e];
        isg[e] = 1.f / s;
        lg -= logf(s);
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

    // Per-step inputs: the quad fetches each of them ONCE.  The scalar inputs of a particle and of its sequence form one
    // field list -- eps[DX] | u (or the teacher-forced index) | mu2[DX] | obs[DY] -- and lane p of the quad loads fields
    // p, p + 4, ..: kSlots loads per lane and step instead of one per field.  Every array is (T, B, ., N)-major, so a
    // slot's pointer advances by a constant per step; pointer and stride are set up here, once.  The loaded words stay
    // raw until the register rotation that ends the step, which hands them to the quad (quad_field: one v_mov_dpp each).
    constexpr int kFU = DX, kFM2 = DX + 1, kFY = 2 * DX + 1, kFields = 2 * DX + 1 + DY, kSlots = (kFields + 3) / 4;
    const in_word_t* in_ptr[kSlots];
    int in_str[kSlots];                           // floats per time step
    // (the field of a lane is picked by selects over the slot's four candidates, each a compile-time field: an if / else chain
    //  on the lane's own field number would be a divergent branch per field)
    auto field_ptr = [&](int f, const in_word_t*& q, int& st) {
        q = a.eps + (size_t)b * DX * N + n;       // a field that is absent re-reads this word (never used)
        st = 0;
        if (f < kFU) {
            q = a.eps + ((size_t)b * DX + f) * N + n;
            st = B * DX * N;
        } else if (f == kFU) {
            if (a.resample) {
                q = (a.idx_in ? reinterpret_cast<const in_word_t*>(a.idx_in) : static_cast<const in_word_t*>(a.u)) + (size_t)b * N + n;
                st = B * N;
            }
        } else if (f < kFY) {
            if (a.two_q) {
                q = a.mu2 + (size_t)b * DX + (f - kFM2);
                st = B * DX;
            }
        } else if (f < kFields) {
            q = a.obs + (size_t)b * DY + (f - kFY);
            st = B * DY;
        }
    };
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        field_ptr(4 * s, in_ptr[s], in_str[s]);
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            const in_word_t* q;
            int st;
            field_ptr(4 * s + j, q, st);
            in_ptr[s] = (p == j) ? q : in_ptr[s];
            in_str[s] = (p == j) ? st : in_str[s];
        }
    }
    float eps_c[DX], mu2_c[DX], obs_c[DY], u_c = 0.f;
    int idx_c = 0;
    float raw_n[kSlots];
    auto issue_inputs = [&]() {    // issues the loads of the slots' next time step, nothing else
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            raw_n[s] = *in_ptr[s];
            in_ptr[s] += in_str[s];
        }
    };
    auto take_inputs = [&]() {     // quad broadcast of the loaded fields (all 64 lanes active)
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            eps_c[d] = quad_field(raw_n, d);
            const float m = quad_field(raw_n, kFM2 + d);
            mu2_c[d] = a.two_q ? m : 0.f;
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) obs_c[k] = quad_field(raw_n, kFY + k);
        u_c = quad_field(raw_n, kFU);
        idx_c = __builtin_bit_cast(int, u_c);
    };
    issue_inputs();
    take_inputs();
    __syncthreads();  // weights visible

    // the lane's weight slices, read from LDS here and nowhere else (see the kernel's header)
    SG rg;
    SQ rq, rf;
    if constexpr (kRegGQ) {
        MlpLds<DX, H, DY, 1>::template load_slice<P>(wg, p, rg);
        MlpLds<DX, H, DX, 1>::template load_slice<P>(wq1, p, rq);
    }
    if constexpr (kRegF) MlpLds<DX, H, DX, 1>::template load_slice<P>(wfm, p, rf);

    SEC_INIT(filter_fwd)
    // t = 0 (its own proposal constants) is peeled: the loop proper then carries one set of step constants
    // instead of selecting between two every step (scalar-register pressure: spills cost v_readlane + s_nop)
    auto step = [&](auto first_tag, const int t) {
        SEC(0);   // (lpp) loop overhead
        const size_t tb = (size_t)t * B + b;
        const StepK<DX> K = decltype(first_tag)::value ? K0 : K1;
#if PSVO_AD
        int rs_f = 0;         // the teacher-forced decision of this step, requested ahead of its use
        if (a.rs_in) rs_f = a.rs_in[tb];
#endif
        if (t + 1 < T) issue_inputs();

        SEC(1);   // (lpp) issue of the prefetch loads
        // ---- proposal (SVO.py:186-197), densities: the same in the four lanes of the particle --------
        float mu[DX], x[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            mu[d] = a.two_q ? K.c[d] * fmaf(K.i1[d], mean1[d], K.i2[d] * mu2_c[d]) : mean1[d];
            x[d] = fmaf(K.c[d], eps_c[d], mu[d]);
        }
        const float q_lp = diag_lp<DX>(x, mu, K.ic, K.lq);
        const float f_lp = diag_lp<DX>(x, fmean, K.ifs, K.lf);

        SEC(2);   // (lpp) proposal, q / f densities
        // ---- the MLPs of the step, hidden units split over the quad ------------------------------------
        float gm[DY], p1[DX], fm[DX];
        if constexpr (kRegGQ) {
            MlpLds<DX, H, DY, 1>::template eval_part<P>(rg, x, gm);
            MlpLds<DX, H, DX, 1>::template eval_part<P>(rq, x, p1);
        } else {
            MG::template eval_part<P>(wg, p, x, gm);
            MQ::template eval_part<P>(wq1, p, x, p1);
        }
        if (!a.bootstrap) {
            if constexpr (kRegF) MlpLds<DX, H, DX, 1>::template eval_part<P>(rf, x, fm);
            else MQ::template eval_part<P>(wfm, p, x, fm);
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) gm[k] = group_sum<P>(gm[k]);
        if (a.emission) {
#pragma unroll
            for (int k = 0; k < DY; ++k) gm[k] = emis_mean(gm[k]);
        }
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            p1[d] = group_sum<P>(p1[d]);
            fm[d] = a.bootstrap ? p1[d] : group_sum<P>(fm[d]);
        }
        const float g_lp = diag_lp<DY>(obs_c, gm, isg, lg);
        float lw = f_lp + g_lp - q_lp + lnw;
        if (!valid) lw = ninf;

        if (valid) {   // history: one lane of the quad per array
            if (p == 0) {
#pragma unroll
                for (int d = 0; d < DX; ++d) a.X[(tb * DX + d) * N + n] = x[d];
                a.logW[tb * N + n] = lw;
            } else if (p == 1) {
#pragma unroll
                for (int d = 0; d < DX; ++d) a.Fm[(tb * DX + d) * N + n] = fm[d];
            } else if (p == 2 && a.P1) {
#pragma unroll
                for (int d = 0; d < DX; ++d) a.P1[(tb * DX + d) * N + n] = p1[d];
            }
        }

        SEC(3);   // (lpp) MLPs, quad sums, weight, history stores
        // ---- log-sum-exp over particles + CDF: per-wave maxima, one barrier ------------------------------
        const float wmx = wave_max(lw);
        const float wbase = (wmx == ninf) ? 0.f : wmx;
        const float w = (valid && p == 0) ? exp2_fast((lw - wbase) * kLog2e) : 0.f;
        float sc = wave_incl_scan(w, lane);
#if PSVO_AD
        const float wsq = wave_sum(w * w);
#endif
        if (lane == 63) {
            red[wave] = wmx;
            red[16 + wave] = sc;
#if PSVO_AD
            red[32 + wave] = wsq;
#endif
        }
        if (a.resample) {   // stage the pre-resampling particle for the gather (one lane of the quad per array)
            if (p == 1) {
#pragma unroll
                for (int d = 0; d < DX; ++d) sx[d * NPT + pn] = x[d];
            } else if (p == 2) {
#pragma unroll
                for (int d = 0; d < DX; ++d) sp[d * NPT + pn] = p1[d];
            } else if (p == 3 && !a.bootstrap) {
#pragma unroll
                for (int d = 0; d < DX; ++d) sf[d * NPT + pn] = fm[d];
            }
        }
        SEC(4);   // (lpp) wave max / scan, staging writes
        __syncthreads();
        SEC(5);   // (lpp) barrier
        // combine the (max, sum) pairs of the <= 16 waves in the lanes of a row: lane i holds wave i
        const int li = lane & 15;
        const float m_i = li < nw ? red[li] : ninf;
        const float s_i = li < nw ? red[16 + li] : 0.f;
        const float gmx = lane_bcast(group_max<16>(m_i), 0);
        const float gbase = (gmx == ninf) ? 0.f : gmx;
        const float v_i = s_i * exp2_fast((m_i - gbase) * kLog2e);        // (empty wave: 0 * exp2(-inf) = 0)
        const float pre = group_incl_scan<16>(v_i, li);
        const float total = lane_bcast(pre, nw - 1);
        const float off = uwave > 0 ? lane_bcast(pre, max(uwave - 1, 0)) : 0.f;   // sum over the waves before this one
        sc = fmaf(sc, exp2_fast((wbase - gbase) * kLog2e), off);
        const float lse_t = fmaf(kLn2, log2_fast(total), gmx);
        if (tid == 3) a.lse[tb] = lse_t;
#if PSVO_AD
        // sum w^2 on the scale of the global maximum: every lane of a row combines the same LDS words in the same order
        const float q_i = li < nw ? red[32 + li] : 0.f;
        const float r_i = exp2_fast((m_i - gbase) * kLog2e);
        const float tot2 = lane_bcast(group_incl_scan<16>(q_i * r_i * r_i, li), nw - 1);
        const float ess = total * total / tot2;
        const bool inherit = a.rs_in ? (rs_f != 0) : !(ess >= a.ess_frac * (float)N);      // (a NaN ESS resamples)
        if (tid == 7) {
            a.ess_out[tb] = ess;
            a.rs_out[tb] = inherit ? 1 : 0;
        }
#endif

        SEC(6);   // (lpp) cross-wave combination
        if (a.resample) {
            if (p == 0) {
                cdf[pn] = sc;
                if ((pn & 15) == 15) piv[pn >> 4] = sc;
            }
            __syncthreads();
            SEC(7);   // (lpp) cdf store + barrier
            int idx;
            if (a.idx_in) {
                idx = idx_c;
            } else {
                // idx = #{k : cdf[k] <= u * total} (SVO.py:266-300 as defined in the oracle), two 16-ary rounds
                const float target = u_c * total;
                const float4 pv = *reinterpret_cast<const float4*>(piv + 4 * p);
                float c1 = (pv.x <= target ? 1.f : 0.f) + (pv.y <= target ? 1.f : 0.f) +
                           (pv.z <= target ? 1.f : 0.f) + (pv.w <= target ? 1.f : 0.f);
                c1 = group_sum<P>(c1);
                const int blk = min((int)c1, (NPT >> 4) - 1);
                const float4 cv = *reinterpret_cast<const float4*>(cdf + 16 * blk + 4 * p);
                float c2 = (cv.x <= target ? 1.f : 0.f) + (cv.y <= target ? 1.f : 0.f) +
                           (cv.z <= target ? 1.f : 0.f) + (cv.w <= target ? 1.f : 0.f);
                c2 = group_sum<P>(c2);
                idx = min(16 * blk + (int)c2, N - 1);
            }
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                x[d] = sx[d * NPT + idx];
                mean1[d] = sp[d * NPT + idx];
                fmean[d] = a.bootstrap ? mean1[d] : sf[d * NPT + idx];
            }
            if (valid) {
                if (p == 3) a.idx_out[tb * N + n] = idx;
                if (p == 0) {
#pragma unroll
                    for (int d = 0; d < DX; ++d) a.Xanc[(tb * DX + d) * N + n] = x[d];
                }
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
            SEC(8);   // (lpp) search, gather, stores
            __syncthreads();  // staged arrays / red[] are rewritten next step
            SEC(9);   // (lpp) barrier
        } else {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                mean1[d] = p1[d];
                fmean[d] = fm[d];
            }
            if (valid) {
                if (p == 3) a.idx_out[tb * N + n] = n;
                if (p == 0) {
#pragma unroll
                    for (int d = 0; d < DX; ++d) a.Xanc[(tb * DX + d) * N + n] = x[d];
                }
            }
            lnw = lw - lse_t;
            __syncthreads();  // red[] reuse
        }

        take_inputs();   // (waits for the prefetch)
    };
    step(std::true_type{}, 0);
    for (int t = 1; t < T; ++t) step(std::false_type{}, t);
}

#undef PSVO_FWD_KERNEL
#undef PSVO_FWD_LPP_KERNEL
#undef PSVO_FWD_ARGS
