// The two persistent reverse-filter kernels.  filter_bwd.hip includes this file twice: PSVO_AD = 0 gives filter_bwd_kernel and
// filter_bwd_lpp_kernel, text and code as they always were; PSVO_AD = 1 gives filter_bwd_ad_kernel and filter_bwd_lpp_ad_kernel,
// the kernels of psvo_filter_backward_adaptive.
//
// Adaptive resampling: the forward pass's decisions rs (T,B) are constants here, like the indices.  The ancestor of particle n at
// step t is rs[t-1] ? idx[t-1][n] : n -- the decision row is requested together with the index row, two steps ahead of the gather
// it steers (filter_bwd_kernel: scalar loads, the select where the ancestor is used; filter_bwd_lpp_kernel: two more fields of the
// quad's list, one with lag 2) -- and the term of the carried normalised weight (`!a.resample` in the static kernels) is applied
// at exactly the steps with rs[t] == 0.  rs[t] is one word per sequence; it is a scalar (readfirstlane) where it guards
// block_sum's barriers.
#if PSVO_AD
#define PSVO_BWD_KERNEL filter_bwd_ad_kernel
#define PSVO_BWD_LPP_KERNEL filter_bwd_lpp_ad_kernel
#define PSVO_BWD_ARGS FilterBwdArgsAd
#else
#define PSVO_BWD_KERNEL filter_bwd_kernel
#define PSVO_BWD_LPP_KERNEL filter_bwd_lpp_kernel
#define PSVO_BWD_ARGS FilterBwdArgs
#endif

// DET (PSVO_TUNE_DETERMINISTIC, where the launcher finds no room for a double-buffered copy per wave: N > 256): ONE buffer of
// c = a.det_copies copies (1 <= c <= waves, the most that fit).  Every lane reads and clears its own entries of all copies (in
// copy order), a barrier, then wave w adds into copy w % c in phase w / c, ceil(waves / c) phases separated by barriers --
// inside a phase each copy has one adding wave (lane order), across phases the phase order: every sum has a fixed order.  At
// N = 512, Dx = 4 without bootstrap eight double-buffered copies of both arrays would take 256 KB of LDS; one buffer of all
// eight takes 128 KB (+ the weights: 131 KB at H = 32, one phase).
template <int DX, int DY, int H, int MAXT, bool DET = false>
__global__ void __launch_bounds__(MAXT) PSVO_BWD_KERNEL(const PSVO_BWD_ARGS a) {
    using MQ = MlpLds<DX, H, DX, PSVO_L>;
    using MG = MlpLds<DX, H, DY, PSVO_L>;
    using AC = FAcc<DX>;
    constexpr int kN = AC::kSg + DY;
    // one wave per SIMD (<= 256 lanes): let the compiler keep the loop-invariant MLP weights in VGPRs
    constexpr bool kRolled = (MAXT > 256) || (MlpLds<DX, H, DX, PSVO_L>::kSize + MlpLds<DX, H, DY, PSVO_L>::kSize > 330);
    constexpr int NBUF = DET ? 1 : 2;     // scatter-target buffers (double-buffered over t; DET: one, behind a barrier)
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = blockDim.x, nw = NT >> 6;
    const int b = blockIdx.x, B = a.B, T = a.T, N = a.N;
    const bool valid = tid < N;
    const int n = valid ? tid : N - 1;

    float* wq1 = smem;
    float* wf = wq1 + MQ::kSize;
    float* wg = wf + MQ::kSize;
    // scatter targets: one copy per wave when the launcher found room for them (a.wave_copies; see filter_bwd_lpp_kernel) --
    // fixed summation order --, else one shared copy and float atomics across the waves
    const int nc = DET ? a.det_copies : (a.wave_copies ? nw : 1);
    const int CP = DX * NT;               // floats of one copy
    float* accP = wg + MG::kSize;         // [2][nc][DX][NT] scatter targets d P1 (+ d Fm when bootstrap)
    float* accF = accP + NBUF * nc * CP;  // [2][nc][DX][NT] d Fm (allocated only when !bootstrap)
    float* red = accF + (a.bootstrap ? 0 : NBUF * nc * CP);   // 16 floats

    MQ::load(wq1, a.q1, tid, NT);
    if (!a.bootstrap) MQ::load(wf, a.f, tid, NT);
    MG::load(wg, a.g, tid, NT);
    const float* wfm = a.bootstrap ? wq1 : wf;
    for (int i = tid; i < (a.bootstrap ? 1 : 2) * NBUF * nc * CP; i += NT) accP[i] = 0.f;

    float sq1[DX], sq2[DX], sfv[DX], s0[DX], fs0[DX], isg[DY];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        sq1[d] = a.sig_q1[d];
        sq2[d] = a.two_q ? a.sig_q2[d] : 1.f;
        sfv[d] = a.bootstrap ? a.sig_q1[d] : a.sig_f[d];
        s0[d] = a.sig0[d];
        fs0[d] = a.fsig0[d];
    }
#pragma unroll
    for (int e = 0; e < DY; ++e) isg[e] = 1.f / a.sig_g[e];
    const StepKR<DX> K0 = make_stepkr<DX>(s0, sq2, fs0, a.two_q != 0);
    const StepKR<DX> K1 = make_stepkr<DX>(sq1, sq2, sfv, a.two_q != 0);

    float acc[kN];
#pragma unroll
    for (int i = 0; i < kN; ++i) acc[i] = 0.f;
    float dlnw = 0.f;  // IWAE: gradient w.r.t. the normalised log-weight carried into step t+1

    // Per-step inputs are software-prefetched: everything of step t-1 is requested at the top of step t,
    // and the ancestor index it gathers through (idx[t-2]) one step earlier still, so the dependent
    // gather Fm[t-2][idx] never sits on the critical path (two HBM round trips per step otherwise).
    // (plain arrays + scalars rather than a struct: a struct of arrays copied per step ends up in scratch)
    float m0r[DX], fm0r[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        m0r[d] = a.m0[b * DX + d];
        fm0r[d] = a.fm0[b * DX + d];
    }
#if PSVO_AD
    // the decisions of this sequence, read through the constant address space: one word per step, the same for every lane, so
    // the loads are scalar and a decision waits in an SGPR until the step that needs it -- no vector register is held for it
    const rs_word_t* rs_b = (const rs_word_t*)a.rs + b;
    auto load_rs = [&](int t) -> int { return t >= 0 ? rs_b[(size_t)t * B] : 1; };
    // the DRAW of particle n at step t - 1; it is the particle's ancestor at step t iff rs[t - 1] (selected where it is used)
    auto load_anc = [&](int t) -> int { return t >= 1 ? a.idx[((size_t)(t - 1) * B + b) * N + n] : n; };
#else
    auto load_anc = [&](int t) -> int {  // ancestor of particle n at step t (its parent lives at t-1)
        return (t >= 1 && a.resample) ? a.idx[((size_t)(t - 1) * B + b) * N + n] : n;
    };
#endif
    // load_step only ISSUES loads into raw registers: every select / add on the loaded values happens when the
    // step consumes them, one whole step later, so no s_waitcnt lands in the prefetch.  (Upstream partials with
    // nparts > 1 are summed here with dependent adds -- the host wrapper passes them already folded, nparts = 1.)
    const bool one_part = (a.nparts == 1);
    auto load_step = [&](int t, int anc, float (&sx)[DX], float (&se)[DX], float (&sm2)[DX], float (&sy)[DY],
                         float (&smean1)[DX], float (&sfmean)[DX], float (&sdfm)[DX], float (&ssc)[4]) {
        const size_t tb = (size_t)t * B + b;
        const size_t tp = (t == 0) ? tb : tb - B;              // (t = 0 has no parent: value replaced at use)
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            sx[d] = a.X[(tb * DX + d) * N + n];
            se[d] = a.eps[(tb * DX + d) * N + n];
            sm2[d] = a.two_q ? a.mu2[tb * DX + d] : 0.f;
            sfmean[d] = a.Fm[(tp * DX + d) * N + anc];
            smean1[d] = a.bootstrap ? 0.f : a.P1[(tp * DX + d) * N + anc];
            if (a.dFm_ext) {
                if (one_part) {
                    sdfm[d] = a.dFm_ext[(tb * DX + d) * N + n];
                } else {
                    float ext = 0.f;
                    for (int p = 0; p < a.nparts; ++p) ext += a.dFm_ext[((tb * a.nparts + p) * DX + d) * N + n];
                    sdfm[d] = ext;
                }
            } else {
                sdfm[d] = 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) sy[k] = a.obs[tb * DY + k];
        ssc[0] = a.logW[tb * N + n];
        ssc[1] = a.lse[tb];
        ssc[2] = a.dlse ? a.dlse[tb] : 0.f;
        if (a.dlogW_ext) {
            if (one_part) {
                ssc[3] = a.dlogW_ext[tb * N + n];
            } else {
                float ext = 0.f;
                for (int p = 0; p < a.nparts; ++p) ext += a.dlogW_ext[(tb * a.nparts + p) * N + n];
                ssc[3] = ext;
            }
        } else {
            ssc[3] = 0.f;
        }
    };
    float c_x[DX], c_e[DX], c_m2[DX], c_y[DY], c_mean1[DX], c_fmean[DX], c_dfm[DX], c_sc[4];
#if PSVO_AD
    int c_anc = load_rs(T - 2) ? load_anc(T - 1) : n;
    int anc_next = load_anc(T - 2), anc_rs_next = load_rs(T - 3);      // draw and decision behind the ancestor of step T-2
    int c_rs = load_rs(T - 1);                 // rs[t] of the step in flight
#else
    int c_anc = load_anc(T - 1);
    int anc_next = load_anc(T - 2);            // ancestor used by step T-2
#endif
    load_step(T - 1, c_anc, c_x, c_e, c_m2, c_y, c_mean1, c_fmean, c_dfm, c_sc);
    __syncthreads();

    SEC_INIT(filter_bwd)
    for (int t = T - 1; t >= 0; --t) {
        SEC(0);
        const size_t tb = (size_t)t * B + b;
        const bool first = (t == 0);
        const StepKR<DX> K = first ? K0 : K1;
        float inc[AC::kSet];  // this step's contribution to the per-dimension sums (set chosen below)
#pragma unroll
        for (int i = 0; i < AC::kSet; ++i) inc[i] = 0.f;
        const int mine = DET ? (wave % nc) * CP : a.wave_copies ? wave * CP : 0;
        float* curP = accP + (DET ? 0 : (t & 1) * nc * CP);                     // all copies of this step's targets
        float* nxtP = accP + (DET ? 0 : ((t + 1) & 1) * nc * CP) + mine;        // this wave's copy (or the shared one) for t - 1
        float* curF = accF + (DET ? 0 : (t & 1) * nc * CP);
        float* nxtF = accF + (DET ? 0 : ((t + 1) & 1) * nc * CP) + mine;

        // ---- forward quantities of this step (prefetched) ----------------------------------------------
        float n_x[DX], n_e[DX], n_m2[DX], n_y[DY], n_mean1[DX], n_fmean[DX], n_dfm[DX], n_sc[4];
        int n_anc = n;
#if PSVO_AD
        int n_rs = 1;
#endif
        if (t >= 1) {
#if PSVO_AD
            n_anc = anc_rs_next ? anc_next : n;
#else
            n_anc = anc_next;
#endif
            load_step(t - 1, n_anc, n_x, n_e, n_m2, n_y, n_mean1, n_fmean, n_dfm, n_sc);
#if PSVO_AD
            n_rs = load_rs(t - 1);
            anc_rs_next = load_rs(t - 3);
#endif
            anc_next = load_anc(t - 2);
        }
        SEC(1);   // issue of the prefetch loads
        // this step's scatter targets (complete since the barrier that ended step t + 1): requested here, ahead of their use
        float sp[DX], sf[DX];
        if (nc == 1) {           // (one shared copy, float atomics: N > 256)
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                sp[d] = curP[d * NT + tid];
                sf[d] = a.bootstrap ? 0.f : curF[d * NT + tid];
            }
        } else {
            float cp[8][DX];
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const int wc = w < nc ? w : nc - 1;       // (unconditional reads of a clamped copy + select)
#pragma unroll
                for (int d = 0; d < DX; ++d) cp[w][d] = curP[wc * CP + d * NT + tid];
            }
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                sp[d] = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) sp[d] += (w < nc) ? cp[w][d] : 0.f;       // in wave order
                sf[d] = 0.f;
            }
        }
        if (nc > 1 && !a.bootstrap) {
            float cf[8][DX];
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const int wc = w < nc ? w : nc - 1;
#pragma unroll
                for (int d = 0; d < DX; ++d) cf[w][d] = curF[wc * CP + d * NT + tid];
            }
#pragma unroll
            for (int d = 0; d < DX; ++d)
#pragma unroll
                for (int w = 0; w < 8; ++w) sf[d] += (w < nc) ? cf[w][d] : 0.f;
        }
        float x[DX], e[DX], m2[DX], y[DY], mean1[DX], fmean[DX];
        const int anc = c_anc;
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            x[d] = c_x[d];
            e[d] = c_e[d];
            m2[d] = c_m2[d];
            // parents: gathered MLP outputs of step t-1 (bootstrap: MLP_q1 == MLP_f), or the t = 0 features
            fmean[d] = first ? fm0r[d] : c_fmean[d];
            mean1[d] = first ? m0r[d] : (a.bootstrap ? c_fmean[d] : c_mean1[d]);
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) y[k] = c_y[k];
        float mu[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d)
            mu[d] = a.two_q ? K.c[d] * fmaf(K.i1[d], mean1[d], K.i2[d] * m2[d]) : mean1[d];

        // ---- gradient w.r.t. logW_t[n] ------------------------------------------------------------
        const float sm = valid ? exp2_fast((c_sc[0] - c_sc[1]) * kLog2e) : 0.f;
        float dlw = c_sc[2] * sm + c_sc[3];
#if PSVO_AD
        if (__builtin_amdgcn_readfirstlane(c_rs) == 0) {      // lnw[t+1] = lw[t] - lse[t]: one word per sequence, made a scalar
#else
        if (!a.resample) {
#endif
            const float tot = block_sum(dlnw, red, wave, lane, nw);
            dlw += dlnw - sm * tot;
        }
        if (!valid) dlw = 0.f;
        dlnw = first ? 0.f : dlw;

        SEC(2);   // d logW
        // ---- emission ---------------------------------------------------------------------------
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
                const float z = (y[k] - gm[k]) * isg[k];
                dgm[k] = dlw * z * isg[k] * dmean;
                acc[AC::kSg + k] += dlw * (z * z - 1.f) * isg[k];
                if (valid) a.dG[(tb * DY + k) * N + n] = dgm[k];
            }
            MG::template bwd_input<kRolled>(wg, x, dgm, dx);
        }
        SEC(3);   // MLP_g forward + input gradient
        // ---- transition and proposal densities ------------------------------------------------------
        float dfmean[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float z = (x[d] - fmean[d]) * K.ifs[d];
            const float tf = dlw * z * K.ifs[d];
            dx[d] -= tf;
            dfmean[d] = tf;
            inc[AC::kSfs + d] += dlw * (z * z - 1.f) * K.ifs[d];
            inc[AC::kSc + d] += dlw * K.ic[d];  // -dq/dc = +dlw / c
        }
        // ---- MLP_q1(x_t), MLP_f(x_t): gradients scattered here by step t+1 (+ backward simulation) --------
        float dPn[DX], dFn[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            dPn[d] = sp[d];
            for (int w = 0; w < nc; ++w) curP[w * CP + d * NT + tid] = 0.f;
            const float ext = c_dfm[d];
            if (a.bootstrap) {
                dPn[d] += ext;
                dFn[d] = 0.f;
            } else {
                dFn[d] = sf[d] + ext;
                for (int w = 0; w < nc; ++w) curF[w * CP + d * NT + tid] = 0.f;
            }
            if (!valid) {
                dPn[d] = 0.f;
                dFn[d] = 0.f;
            }
        }
        if (valid) {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                a.dP[(tb * DX + d) * N + n] = dPn[d];
                if (!a.bootstrap) a.dF[(tb * DX + d) * N + n] = dFn[d];
            }
        }
        SEC(4);   // densities, scatter targets from LDS, row stores
        MQ::template bwd_input<kRolled>(wq1, x, dPn, dx);
        if (!a.bootstrap) MQ::template bwd_input<kRolled>(wfm, x, dFn, dx);
        SEC(5);   // MLP_q1 (/ MLP_f) input gradient

        // ---- x = mu + c eps, mu = c (mean1/s1 + mu2/s2) ----------------------------------------------------
        float dmean1[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float dmu = dx[d];
            inc[AC::kSc + d] += dmu * e[d];
            float dm2 = 0.f;
            if (a.two_q) {
                dmean1[d] = dmu * K.c[d] * K.i1[d];
                dm2 = dmu * K.c[d] * K.i2[d];
                inc[AC::kSmm1 + d] += dmu * mean1[d];
                inc[AC::kSmb + d] += dmu * m2[d];
                inc[AC::kSmm + d] += dmu * mu[d];
                // summed over the particles by a parallel kernel after the time loop: a block sum here would put
                // a wave reduction, an LDS round trip and a barrier into every step of the serial chain
                if (valid) a.dm2_rows[(tb * DX + d) * N + n] = dm2;
            } else {
                dmean1[d] = dmu;
            }
        }
        SEC(6);   // PoG gradient, block sums of d mu2
        // ---- gather backward: scatter-add into the parents (SVO.py:255-257) ------------------------------
        if (!first) {
            if constexpr (DET) {
                __syncthreads();      // (one buffer: every lane has read and cleared this step's targets)
                for (int ph = 0; ph < (nw + nc - 1) / nc; ++ph) {
                    if (ph > 0) __syncthreads();
                    if (valid && wave / nc == ph) {
#pragma unroll
                        for (int d = 0; d < DX; ++d) {
                            if (a.bootstrap) {
                                atomicAdd(&nxtP[d * NT + anc], dmean1[d] + dfmean[d]);
                            } else {
                                atomicAdd(&nxtP[d * NT + anc], dmean1[d]);
                                atomicAdd(&nxtF[d * NT + anc], dfmean[d]);
                            }
                        }
                    }
                }
            } else if (valid) {
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    if (a.bootstrap) {
                        atomicAdd(&nxtP[d * NT + anc], dmean1[d] + dfmean[d]);
                    } else {
                        atomicAdd(&nxtP[d * NT + anc], dmean1[d]);
                        atomicAdd(&nxtF[d * NT + anc], dfmean[d]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                const float s1 = block_sum(dmean1[d], red, wave, lane, nw);
                const float s2 = block_sum(dfmean[d], red, wave, lane, nw);
                if (tid == 0) {   // (fm0 aliasing m0: ONE tensor feeds both, its gradient is the sum -- see psvo_hip.h)
                    const bool same0 = (a.fm0 == a.m0);
                    a.dm0[b * DX + d] = same0 ? s1 + s2 : s1;
                    a.dfm0[b * DX + d] = same0 ? 0.f : s2;
                }
            }
        }
        SEC(7);   // LDS scatter-add
        if (t >= 1) {
            c_anc = n_anc;
#if PSVO_AD
            c_rs = n_rs;
#endif
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                c_x[d] = n_x[d]; c_e[d] = n_e[d]; c_m2[d] = n_m2[d];
                c_mean1[d] = n_mean1[d]; c_fmean[d] = n_fmean[d]; c_dfm[d] = n_dfm[d];
            }
#pragma unroll
            for (int k = 0; k < DY; ++k) c_y[k] = n_y[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) c_sc[k] = n_sc[k];
        }
#pragma unroll
        for (int i = 0; i < AC::kSet; ++i) {  // set 0: t = 0, set 1: t >= 1 (static register indices)
            acc[i] += first ? inc[i] : 0.f;
            acc[AC::kSet + i] += first ? 0.f : inc[i];
        }
        __syncthreads();
        SEC(8);   // register rotation (waits for the prefetch) + barrier
    }

    // ---- per-sequence scalar accumulators ---------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < kN; ++i) {
        const float s = block_sum(acc[i], red, wave, lane, nw);
        if (tid == 0) a.sacc[(size_t)b * kN + i] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// Four lanes per particle (N <= 128), mirror of filter_fwd_lpp_kernel: lane p of the quad owns hidden units
// [p H/4, (p+1) H/4) of every MLP (forward recompute and input gradient), the partial input gradients are summed
// over the quad with two DPP adds; everything that is not an MLP is computed redundantly in the four lanes and
// counted once (lane p == 0) in the sums.  The reverse filter is on the critical path of a training step and its
// step is a dependent chain, so shortening the two MLP input-gradient chains is what matters.
// ---------------------------------------------------------------------------------------------
template <int DX, int DY, int H>
__global__ void __launch_bounds__(512) PSVO_BWD_LPP_KERNEL(const PSVO_BWD_ARGS a) {
    using MQ = MlpLds<DX, H, DX, PSVO_L>;
    using MG = MlpLds<DX, H, DY, PSVO_L>;
    using AC = FAcc<DX>;
    constexpr int kN = AC::kSg + DY;
    constexpr int P = 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = blockDim.x, nw = NT >> 6;
    const int NPT = NT / P;
    const int b = blockIdx.x, B = a.B, T = a.T, N = a.N;
    const int pn = tid >> 2, p = tid & 3;
    const bool valid = pn < N;
    const bool one = valid && p == 0;          // the lane of the quad that counts in sums over particles
    const int n = valid ? pn : N - 1;

    float* wq1 = smem;
    float* wf = wq1 + MQ::kSize;
    float* wg = wf + MQ::kSize;
    // Scatter targets of the resampling gather's reverse (children add into their parent): ONE COPY PER WAVE.  Float atomics
    // from several waves on one LDS word are applied in arrival order, so the sums -- and with them every gradient of the
    // step -- differed in the last bits from run to run (round-2 review).  Within a wave the atomics of one instruction are
    // resolved in lane order and instructions in program order; with a copy per wave and the parent adding the copies in
    // wave order, the order of every sum is fixed.  Cost: nw reads + clears per value where there was one (~1 % of the
    // kernel); LDS 2 x nw x DX x NPT floats (16 KB at Dx = 2, N = 128).
    const int CP = DX * NPT;              // floats of one copy
    float* accP = wg + MG::kSize;         // [2][nw][DX][NPT] d P1 (+ d Fm when bootstrap)
    float* accF = accP + 2 * nw * CP;     // [2][nw][DX][NPT] d Fm (only when !bootstrap)
    float* red = accF + 2 * nw * CP;      // 16 floats

    MQ::load(wq1, a.q1, tid, NT);
    if (!a.bootstrap) MQ::load(wf, a.f, tid, NT);
    MG::load(wg, a.g, tid, NT);
    const float* wfm = a.bootstrap ? wq1 : wf;
    for (int i = tid; i < 4 * nw * CP; i += NT) accP[i] = 0.f;

    float sq1[DX], sq2[DX], sfv[DX], s0[DX], fs0[DX], isg[DY];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        sq1[d] = a.sig_q1[d];
        sq2[d] = a.two_q ? a.sig_q2[d] : 1.f;
        sfv[d] = a.bootstrap ? a.sig_q1[d] : a.sig_f[d];
        s0[d] = a.sig0[d];
        fs0[d] = a.fsig0[d];
    }
#pragma unroll
    for (int e = 0; e < DY; ++e) isg[e] = 1.f / a.sig_g[e];
    const StepKR<DX> K0 = make_stepkr<DX>(s0, sq2, fs0, a.two_q != 0);
    const StepKR<DX> K1 = make_stepkr<DX>(sq1, sq2, sfv, a.two_q != 0);

    float acc[kN];
#pragma unroll
    for (int i = 0; i < kN; ++i) acc[i] = 0.f;
    float dlnw = 0.f;

    float m0r[DX], fm0r[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        m0r[d] = a.m0[b * DX + d];
        fm0r[d] = a.fm0[b * DX + d];
    }
    auto load_anc = [&](int t) -> int {
#if PSVO_AD
        if (t < 1) return n;
        const int r = a.rs[(size_t)(t - 1) * B + b], i = a.idx[((size_t)(t - 1) * B + b) * N + n];
        return r ? i : n;
#else
        return (t >= 1 && a.resample) ? a.idx[((size_t)(t - 1) * B + b) * N + n] : n;
#endif
    };
    const bool one_part = (a.nparts == 1);
    const bool ext_fm = a.dFm_ext && one_part, ext_lw = a.dlogW_ext && one_part;
    // Per-step inputs: the quad fetches each of them ONCE (see filter_fwd_lpp_kernel).  The field list is
    //   X[DX] | eps[DX] | Fm[anc][DX] | dFm_ext[DX] | logW | dlogW_ext | next ancestor | mu2[DX] | obs[DY] | lse | dlse | P1[anc][DX]
    // and lane p of the quad loads fields p, p + 4, ..: kSlots loads per lane and step (one fewer when bootstrap leaves the
    // last slot empty) instead of one per field.  A field of step t reads row max(t - lag, 0) of its (T, B, ., N) array: lag
    // 1 for the parent's Fm / P1 (row t - 1, indexed by the ancestor), lag 2 for the ancestor index that step t - 1 will
    // gather with (idx row t - 2).  Pointer, stride and lag of the lane's slots are set up here, once; the upstream
    // gradients in several parts (nparts > 1) keep their own loads below.
    constexpr int kFX = 0, kFE = DX, kFFm = 2 * DX, kFDf = 3 * DX, kFLw = 4 * DX, kFDlw = 4 * DX + 1, kFAnc = 4 * DX + 2,
#if PSVO_AD
    // (two more fields ahead of P1: rs[t], and the decision row that goes with the next ancestor's index row -- lag 2)
                  kFM2 = 4 * DX + 3, kFY = 5 * DX + 3, kFLse = 5 * DX + 3 + DY, kFDlse = kFLse + 1, kFRs = kFLse + 2,
                  kFRsAnc = kFLse + 3, kFP1 = kFLse + 4,
                  kFields = kFP1 + DX, kSlots = (kFields + 3) / 4;
#else
                  kFM2 = 4 * DX + 3, kFY = 5 * DX + 3, kFLse = 5 * DX + 3 + DY, kFDlse = kFLse + 1, kFP1 = kFLse + 2,
                  kFields = kFP1 + DX, kSlots = (kFields + 3) / 4;
#endif
    // (one invariant ties the three places that know about lags together: field_ptr gives lag 1 to exactly the fields of
    //  [kFFm, kFFm + DX) and [kFP1, kFP1 + DX) and lag 2 to kFAnc alone; slot_gathers / slot_lags below are the per-slot
    //  shadows of those ranges, and issue_step adds the ancestor to a lane's address iff its lag is 1)
    static_assert(kFAnc >= kFFm + DX && kFAnc < kFP1, "the ancestor field (lag 2) lies outside the gathered (lag 1) ranges");
    const int nslots = a.bootstrap ? (kFP1 + 3) / 4 : kSlots;
    auto slot_gathers = [](int s) { return (4 * s < kFFm + DX && 4 * s + 3 >= kFFm) || (4 * s < kFP1 + DX && 4 * s + 3 >= kFP1); };
#if PSVO_AD
    auto slot_lags = [&](int s) {
        return slot_gathers(s) || (4 * s <= kFAnc && 4 * s + 3 >= kFAnc) || (4 * s <= kFRsAnc && 4 * s + 3 >= kFRsAnc);
    };
#else
    auto slot_lags = [&](int s) { return slot_gathers(s) || (4 * s <= kFAnc && 4 * s + 3 >= kFAnc); };
#endif
    const in_word_t* in_ptr[kSlots];
    int in_str[kSlots], in_lag[kSlots];           // floats per time step; rows behind t
    // (the field of a lane is picked by selects over the slot's four candidates, each a compile-time field: an if / else chain
    //  on the lane's own field number would be a divergent branch per field)
    auto field_ptr = [&](int f, const in_word_t*& ptr, int& str, int& lg) {
        const in_word_t* q = nullptr;                 // base of the field's array at (row 0, b); null: absent
        int w = 0, lag = 0;                       // floats of a (t, b) row of that array
        if (f < kFE) { q = a.X + (size_t)(b * DX + f - kFX) * N + n; w = DX * N; }
        else if (f < kFFm) { q = a.eps + (size_t)(b * DX + f - kFE) * N + n; w = DX * N; }
        else if (f < kFDf) { q = a.Fm + (size_t)(b * DX + f - kFFm) * N; w = DX * N; lag = 1; }
        else if (f < kFLw) { if (ext_fm) { q = a.dFm_ext + (size_t)(b * DX + f - kFDf) * N + n; w = DX * N; } }
        else if (f == kFLw) { q = a.logW + (size_t)b * N + n; w = N; }
        else if (f == kFDlw) { if (ext_lw) { q = a.dlogW_ext + (size_t)b * N + n; w = N; } }
        else if (f == kFAnc) { if (a.resample) { q = reinterpret_cast<const in_word_t*>(a.idx) + (size_t)b * N + n; w = N; lag = 2; } }
        else if (f < kFY) { if (a.two_q) { q = a.mu2 + b * DX + f - kFM2; w = DX; } }
        else if (f < kFLse) { q = a.obs + b * DY + f - kFY; w = DY; }
        else if (f == kFLse) { q = a.lse + b; w = 1; }
        else if (f == kFDlse) { if (a.dlse) { q = a.dlse + b; w = 1; } }
#if PSVO_AD
        else if (f == kFRs) { q = reinterpret_cast<const in_word_t*>(a.rs) + b; w = 1; }
        else if (f == kFRsAnc) { q = reinterpret_cast<const in_word_t*>(a.rs) + b; w = 1; lag = 2; }
#endif
        else if (f < kFields) { if (!a.bootstrap) { q = a.P1 + (size_t)(b * DX + f - kFP1) * N; w = DX * N; lag = 1; } }
        if (q) {
            ptr = q + (size_t)max(T - 1 - lag, 0) * B * w;
            str = B * w;
            lg = lag;
        } else {                                  // re-reads one word that is always there (never used)
            ptr = a.eps + (size_t)b * DX * N + n;
            str = 0;
            lg = 0;
        }
    };
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        field_ptr(4 * s, in_ptr[s], in_str[s], in_lag[s]);
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            const in_word_t* q;
            int st, lg;
            field_ptr(4 * s + j, q, st, lg);
            in_ptr[s] = (p == j) ? q : in_ptr[s];
            in_str[s] = (p == j) ? st : in_str[s];
            in_lag[s] = (p == j) ? lg : in_lag[s];
        }
    }
    float raw_n[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) raw_n[s] = 0.f;
    // issue-only prefetch (see filter_bwd_kernel): the loads of step t, whose particles have the ancestor `anc`
    auto issue_step = [&](int t, int anc) {
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            if (s < nslots) {
                if (slot_gathers(s)) raw_n[s] = in_ptr[s][in_lag[s] == 1 ? anc : 0];
                else raw_n[s] = *in_ptr[s];
                if (slot_lags(s)) in_ptr[s] -= (t > in_lag[s]) ? in_str[s] : 0;
                else in_ptr[s] -= in_str[s];
            }
        }
    };
    // upstream gradients in several parts: every lane sums its particle's parts (issued with the prefetch, as before)
    auto issue_parts = [&](int t, float (&sdfm)[DX], float& sdlw) {
        const size_t tb = (size_t)t * B + b;
        if (a.dFm_ext && !one_part) {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                float ext = 0.f;
                for (int q = 0; q < a.nparts; ++q) ext += a.dFm_ext[((tb * a.nparts + q) * DX + d) * N + n];
                sdfm[d] = ext;
            }
        }
        if (a.dlogW_ext && !one_part) {
            float ext = 0.f;
            for (int q = 0; q < a.nparts; ++q) ext += a.dlogW_ext[(tb * a.nparts + q) * N + n];
            sdlw = ext;
        }
    };
    float c_x[DX], c_e[DX], c_m2[DX], c_y[DY], c_mean1[DX], c_fmean[DX], c_dfm[DX], c_sc[4];
    int c_anc = load_anc(T - 1), anc_next = n;
#if PSVO_AD
    int c_rs = 1;                              // rs[t] of the step in flight
#endif
    // quad broadcast of the fields loaded for step t (all 64 lanes active); `pdfm` / `pdlw`: the sums of issue_parts
    auto take_step = [&](int t, const float (&pdfm)[DX], float pdlw) {
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            c_x[d] = quad_field(raw_n, kFX + d);
            c_e[d] = quad_field(raw_n, kFE + d);
            const float m2 = quad_field(raw_n, kFM2 + d), p1 = quad_field(raw_n, kFP1 + d), df = quad_field(raw_n, kFDf + d);
            c_m2[d] = a.two_q ? m2 : 0.f;
            c_fmean[d] = quad_field(raw_n, kFFm + d);
            c_mean1[d] = a.bootstrap ? 0.f : p1;
            c_dfm[d] = a.dFm_ext ? (one_part ? df : pdfm[d]) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) c_y[k] = quad_field(raw_n, kFY + k);
        const float dlse = quad_field(raw_n, kFDlse), dlw = quad_field(raw_n, kFDlw);
        const int an = __builtin_bit_cast(int, quad_field(raw_n, kFAnc));
        c_sc[0] = quad_field(raw_n, kFLw);
        c_sc[1] = quad_field(raw_n, kFLse);
        c_sc[2] = a.dlse ? dlse : 0.f;
        c_sc[3] = a.dlogW_ext ? (one_part ? dlw : pdlw) : 0.f;
#if PSVO_AD
        c_rs = __builtin_bit_cast(int, quad_field(raw_n, kFRs));
        anc_next = (t >= 2 && __builtin_bit_cast(int, quad_field(raw_n, kFRsAnc)) != 0) ? an : n;     // ancestor of step t - 1
#else
        anc_next = (a.resample && t >= 2) ? an : n;     // ancestor of step t - 1
#endif
    };
    {
        float pdfm[DX], pdlw = 0.f;
#pragma unroll
        for (int d = 0; d < DX; ++d) pdfm[d] = 0.f;
        issue_step(T - 1, c_anc);
        issue_parts(T - 1, pdfm, pdlw);
        take_step(T - 1, pdfm, pdlw);
    }
    __syncthreads();

    SEC_INIT(filter_bwd)
    // t = 0 (own step constants, block sums instead of the scatter) is peeled out of the loop: see filter_fwd_lpp_kernel
    auto step = [&](auto first_tag, const int t) {
        SEC(0);   // (lpp) loop overhead
        const size_t tb = (size_t)t * B + b;
        constexpr bool first = decltype(first_tag)::value;
        const StepKR<DX> K = first ? K0 : K1;
        float inc[AC::kSet];
#pragma unroll
        for (int i = 0; i < AC::kSet; ++i) inc[i] = 0.f;
        float* curP = accP + (t & 1) * nw * CP;                      // all waves' copies of this step's targets
        float* nxtP = accP + ((t + 1) & 1) * nw * CP + wave * CP;    // this wave's copy for step t - 1
        float* curF = accF + (t & 1) * nw * CP;
        float* nxtF = accF + ((t + 1) & 1) * nw * CP + wave * CP;

        float n_dfm[DX], n_dlw = 0.f;
#pragma unroll
        for (int d = 0; d < DX; ++d) n_dfm[d] = 0.f;
        const int n_anc = anc_next;
        if (t >= 1) {
            issue_step(t - 1, n_anc);
            issue_parts(t - 1, n_dfm, n_dlw);
        }
        SEC(1);   // (lpp) issue of the prefetch loads
        // the scatter targets of this step (complete since the barrier that ended step t + 1) are requested HERE, a whole
        // MLP pass ahead of their use, so that the nw reads per value cost issue slots only
        float sp[DX], sf[DX];
        {
            float cp[8][DX];
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                // (unconditional reads of a clamped copy + select: a guarded load is a branch, and a wait, per copy)
                const int wc = w < nw ? w : nw - 1;
#pragma unroll
                for (int d = 0; d < DX; ++d) cp[w][d] = curP[wc * CP + d * NPT + pn];
            }
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                sp[d] = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) sp[d] += (w < nw) ? cp[w][d] : 0.f;        // the waves' copies, in wave order
                sf[d] = 0.f;
            }
        }
        if (!a.bootstrap) {
            float cf[8][DX];
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const int wc = w < nw ? w : nw - 1;
#pragma unroll
                for (int d = 0; d < DX; ++d) cf[w][d] = curF[wc * CP + d * NPT + pn];
            }
#pragma unroll
            for (int d = 0; d < DX; ++d)
#pragma unroll
                for (int w = 0; w < 8; ++w) sf[d] += (w < nw) ? cf[w][d] : 0.f;
        }
        float x[DX], e[DX], m2[DX], y[DY], mean1[DX], fmean[DX];
        const int anc = c_anc;
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            x[d] = c_x[d];
            e[d] = c_e[d];
            m2[d] = c_m2[d];
            fmean[d] = first ? fm0r[d] : c_fmean[d];
            mean1[d] = first ? m0r[d] : (a.bootstrap ? c_fmean[d] : c_mean1[d]);
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) y[k] = c_y[k];
        float mu[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d)
            mu[d] = a.two_q ? K.c[d] * fmaf(K.i1[d], mean1[d], K.i2[d] * m2[d]) : mean1[d];

        // ---- gradient w.r.t. logW_t[n] (the same in the four lanes of the particle) ---------------------------------
        const float sm = valid ? exp2_fast((c_sc[0] - c_sc[1]) * kLog2e) : 0.f;
        float dlw = c_sc[2] * sm + c_sc[3];
#if PSVO_AD
        if (__builtin_amdgcn_readfirstlane(c_rs) == 0) {      // lnw[t+1] = lw[t] - lse[t]: one word per sequence, made a scalar
#else
        if (!a.resample) {
#endif
            const float tot = block_sum(one ? dlnw : 0.f, red, wave, lane, nw);
            dlw += dlnw - sm * tot;
        }
        if (!valid) dlw = 0.f;
        dlnw = first ? 0.f : dlw;
        const float cnt = (p == 0) ? 1.f : 0.f;     // sums over particles take the quad's first lane

        SEC(2);   // (lpp) proposal mean, d logW
        // ---- emission: hidden units of MLP_g split over the quad ----------------------------------------------------
        float dxp[DX];                              // this lane's PARTIAL of d x (summed over the quad below)
#pragma unroll
        for (int d = 0; d < DX; ++d) dxp[d] = 0.f;
        {
            float gm[DY], dgm[DY];
            MG::template eval_part<P>(wg, p, x, gm);
#pragma unroll
            for (int k = 0; k < DY; ++k) {
                gm[k] = group_sum<P>(gm[k]);
                float dmean = 1.f;
                if (a.emission) { dmean = emis_dmean(gm[k]); gm[k] = emis_mean(gm[k]); }
                const float z = (y[k] - gm[k]) * isg[k];
                dgm[k] = dlw * z * isg[k] * dmean;
                acc[AC::kSg + k] += cnt * dlw * (z * z - 1.f) * isg[k];
                if (valid && p == 2) a.dG[(tb * DY + k) * N + n] = dgm[k];
            }
            MG::template bwd_input_part<P>(wg, p, x, dgm, dxp);
        }
        SEC(3);   // (lpp) MLP_g forward, quad sum, input gradient, dG row store
        // ---- transition and proposal densities ------------------------------------------------------------------------
        float dfmean[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float z = (x[d] - fmean[d]) * K.ifs[d];
            const float tf = dlw * z * K.ifs[d];
            dxp[d] -= cnt * tf;
            dfmean[d] = tf;
            inc[AC::kSfs + d] += dlw * (z * z - 1.f) * K.ifs[d];
            inc[AC::kSc + d] += dlw * K.ic[d];
        }
        // ---- MLP_q1(x_t), MLP_f(x_t): gradients scattered here by step t+1 (+ backward simulation) -----------------------
        float dPn[DX], dFn[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            dPn[d] = sp[d];
            const float ext = c_dfm[d];
            if (a.bootstrap) {
                dPn[d] += ext;
                dFn[d] = 0.f;
            } else {
                dFn[d] = sf[d] + ext;
            }
            if (!valid) {
                dPn[d] = 0.f;
                dFn[d] = 0.f;
            }
        }
        // (only this quad reads these entries, in the wave instructions above: clear them for step t-2; lane p takes the
        //  copies w = p, p + 4)
        for (int w = p; w < nw; w += 4) {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                curP[w * CP + d * NPT + pn] = 0.f;
                if (!a.bootstrap) curF[w * CP + d * NPT + pn] = 0.f;
            }
        }
        if (valid) {
            if (p == 0) {
#pragma unroll
                for (int d = 0; d < DX; ++d) a.dP[(tb * DX + d) * N + n] = dPn[d];
            } else if (p == 1 && !a.bootstrap) {
#pragma unroll
                for (int d = 0; d < DX; ++d) a.dF[(tb * DX + d) * N + n] = dFn[d];
            }
        }
        SEC(4);   // (lpp) densities, scatter targets from LDS, dP / dF row stores
        MQ::template bwd_input_part<P>(wq1, p, x, dPn, dxp);
        if (!a.bootstrap) MQ::template bwd_input_part<P>(wfm, p, x, dFn, dxp);
        SEC(5);   // (lpp) MLP_q1 (/ MLP_f) input gradient

        // ---- x = mu + c eps, mu = c (mean1/s1 + mu2/s2) -------------------------------------------------------------------
        float dmean1[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float dmu = group_sum<P>(dxp[d]);
            inc[AC::kSc + d] += dmu * e[d];
            if (a.two_q) {
                dmean1[d] = dmu * K.c[d] * K.i1[d];
                const float dm2 = dmu * K.c[d] * K.i2[d];
                inc[AC::kSmm1 + d] += dmu * mean1[d];
                inc[AC::kSmb + d] += dmu * m2[d];
                inc[AC::kSmm + d] += dmu * mu[d];
                if (valid && p == 3) a.dm2_rows[(tb * DX + d) * N + n] = dm2;
            } else {
                dmean1[d] = dmu;
            }
        }
        SEC(6);   // (lpp) quad sums of d x, product-of-Gaussians gradient, d mu2 row store
        // ---- gather backward: scatter-add into the parents (SVO.py:255-257), one dimension per lane of the quad --------
        if (!first) {
            if (valid) {
#pragma unroll
                for (int d = 0; d < DX; ++d) {
                    if ((d & 3) == p) {
                        if (a.bootstrap) {
                            atomicAdd(&nxtP[d * NPT + anc], dmean1[d] + dfmean[d]);
                        } else {
                            atomicAdd(&nxtP[d * NPT + anc], dmean1[d]);
                            atomicAdd(&nxtF[d * NPT + anc], dfmean[d]);
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                const float s1 = block_sum(one ? dmean1[d] : 0.f, red, wave, lane, nw);
                const float s2 = block_sum(one ? dfmean[d] : 0.f, red, wave, lane, nw);
                if (tid == 0) {   // (fm0 aliasing m0: ONE tensor feeds both, its gradient is the sum -- see psvo_hip.h)
                    const bool same0 = (a.fm0 == a.m0);
                    a.dm0[b * DX + d] = same0 ? s1 + s2 : s1;
                    a.dfm0[b * DX + d] = same0 ? 0.f : s2;
                }
            }
        }
        SEC(7);   // (lpp) LDS scatter-add into the parents
        if (t >= 1) {
            c_anc = n_anc;
            take_step(t - 1, n_dfm, n_dlw);
        }
#pragma unroll
        for (int i = 0; i < AC::kSet; ++i) {
            acc[i] += (first && p == 0) ? inc[i] : 0.f;
            acc[AC::kSet + i] += (!first && p == 0) ? inc[i] : 0.f;
        }
        __syncthreads();
        SEC(8);   // (lpp) register rotation (waits for the prefetch) + barrier
    };
    for (int t = T - 1; t >= 1; --t) step(std::false_type{}, t);
    step(std::true_type{}, 0);

#pragma unroll
    for (int i = 0; i < kN; ++i) {
        const float s = block_sum(valid ? acc[i] : 0.f, red, wave, lane, nw);
        if (tid == 0) a.sacc[(size_t)b * kN + i] = s;
    }
}

#undef PSVO_BWD_KERNEL
#undef PSVO_BWD_LPP_KERNEL
#undef PSVO_BWD_ARGS
