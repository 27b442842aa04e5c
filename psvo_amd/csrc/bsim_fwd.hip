// Backward simulation with proposal (PSVO): restates PSVO.backward_simulation_w_proposal
// (reference src/SMC/PSVO.py:69-203) -- see include/psvo_hip.h for the contract.
//
// Work decomposition (MI355X).  The B*N backward chains never interact (PSVO.py:116-151); each
// chain step draws M sub-particles and needs, for each, logsumexp_j over ALL N forward particles
// of the transition log-density (the reference's (M, N, N, B) tile, PSVO.py:128-133).
//   * workgroup = 256 lanes = 256/(M*HS) chains of ONE sequence b, persistent over t = T-1 .. 0;
//   * lane = (chain, [half,] sub-particle m): the lane owns proposal m (sampling, MLP_f, MLP_g); with HS = 2 the two
//     halves of a chain split the forward particles and the hidden units of every MLP (two waves per SIMD at C*);
//   * the pair loop is register-blocked over the lane's QUAD: the four lanes of a quad hold four
//     consecutive m; each lane walks the forward particles j = q, q+4, ... (q = quad lane) and
//     evaluates all four m of its quad against each j, so one 16-byte LDS broadcast read feeds
//     four pairs.  Partial (max, sum) pairs are merged across the quad with two xor-shuffles.
//   * the forward tile of step t-1 -- F'_j = MLP_f(X_{t-1}[j]) * r and W'_j = normalised log
//     weight, both pre-scaled into the log2 domain -- is staged in LDS (N * 16 B; 2 KB at N=128),
//     double-buffered, prefetched from HBM one step ahead.  The tile is never materialised.
//   * prefetch: step t requests, at its top, the inputs of step t-1 (eps, bmu2, obs, the uniform or the forced index) and
//     the raw tile of step t-2, and waits for all of them in ONE place, the `settle` in the rotation that ends the step
//     (in front of its output stores); no s_waitcnt vmcnt stands between the two.  Every load is issued in every step on
//     every path: the uniform and the forced index come through one base chosen in front of the loop, a thread's tile
//     entries are a launch-uniform number of register sets with the entry index clamped, and where there is no step t-1
//     or tile t-2 left the bases stand still and the words are dropped.  Addresses are 64-bit scalar bases that move by a
//     constant per step plus a constant 32-bit lane offset (saddr form): no multiply by t, no limit on an array's size.
//   * pair arithmetic: v = W'_j - sum_d (x'_d - F'_jd)^2  (log2 domain) in packed f32 (two sub-particles per
//     instruction); log-sum-exp in blocks of 16 tile entries: all v of a block and its maximum first, then one
//     rescale of the running sums and the block's exponentials (the tile is padded with W' = -inf to whole blocks).
#include "common.h"

namespace psvo {
inline namespace PSVO_LNS {   // l1 / l2: hidden layers of the per-particle MLPs (common.h)
PSVO_TIMERS_DEFINE(bsim_fwd)


struct BsimArgs {
    int B, T, N;
    int emission;
    psvo_mlp f, g, q1inv;
    const float *X, *Fm, *logW, *lse;
    const float *sig_f, *sig_g, *sig_q1inv, *sig_bq2;
    const float *bmu2, *minit, *sig_init, *imean, *isig;
    const float *obs, *eps_b, *u_b;
    const int32_t* sel_in;
    float *bwX, *flp, *glp, *Omega;
    int32_t* sel_out;
    float* score;
    float *lam2_all, *om_all, *mu1_all;  // optional saves for psvo_bsim_backward (may be null)
};

template <int DX>
struct TileSlot {
    static constexpr int kFloats = (DX <= 3) ? 4 : 8;
};

__device__ __forceinline__ float quad_bcast(float v, int lane, int i) { return __shfl(v, (lane & ~3) | i); }

// merge two online-lse states kept in the log2 domain
__device__ __forceinline__ void lse2_merge(float& m, float& s, float m2, float s2) {
    const float nm = fmaxf(m, m2);
    // guard -inf - -inf
    const float a = (m == nm) ? 1.f : exp2_fast(m - nm);
    const float b = (m2 == nm) ? 1.f : exp2_fast(m2 - nm);
    s = s * a + s2 * b;
    m = nm;
}

// HS = 1: lane = (chain, m).  HS = 2: lane = (chain, half, m) -- the two halves of a chain split the
// walk over the forward particles and the hidden units of every MLP evaluation, so a chain step is
// spread over 2*M lanes.  At C* (65536 (chain, m) pairs = one wave per SIMD, where a lone wave issues
// one VALU op per 4 cycles) this doubles the resident waves per SIMD.
// (Two hidden layers, Dx = 2, Dy = 1, H = 32: the kernels that fit two waves per SIMD, 256 registers, keep doing so -- left
//  alone hipcc takes 276 with the constants and the settle pairs below.  <2,1,32,4,1> does not fit without scratch and is
//  left at one wave.)
template <int DX, int DY, int H, int M, int HS>
constexpr int kBsimFwdWaves = (PSVO_L == 2 && DX == 2 && DY == 1 && H == 32 && !(M == 4 && HS == 1)) ? 2 : 1;
template <int DX, int DY, int H, int M, int HS>
__global__ void __launch_bounds__(256, (kBsimFwdWaves<DX, DY, H, M, HS>)) bsim_fwd_kernel(const BsimArgs a) {
    using MQ = MlpLds<DX, H, DX, PSVO_L>;
    using MG = MlpLds<DX, H, DY, PSVO_L>;
    constexpr int PS = TileSlot<DX>::kFloats;
    constexpr int kMaxStage = 4;
    constexpr bool kRolled = (2 * MQ::kSize + MG::kSize) > 330;
    // the forms of profiles/bsim_fwd_valu_diet.md (cross-lane sums and maxima on add_xor / max_xor, the cross-half add of the merge
    // behind the select, the first 16-entry block without a rescale) hold for the one-hidden-layer unit.  In the two-layer
    // unit each of them alone cost some instantiation scalar registers or scratch (the note's table): it keeps the plain forms.
    constexpr bool kDiet = PSVO_L == 1;
    // the first-block form only with two half-chains: with whole chains (HS = 1, four and more blocks per step, where it saves
    // the least) hipcc allocated the kernel 166 registers instead of 235 and the C4 step got 0.8 % slower
    constexpr bool kFirstBlock = kDiet && HS == 2;
    constexpr bool kPeel = (DX <= 3);   // (the Dx = 4 kernel measured slower peeled: C5 14.4 -> 17.6 ms)
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int NTB = blockDim.x;
    const int B = a.B, T = a.T, N = a.N;
    // forward tile padded (W' = -inf) so that every half-slice of a quad lane is a whole number of 4-entry blocks
    const int NP = ((N + 16 * HS - 1) / (16 * HS)) * (16 * HS);
    const int b = blockIdx.y;
    constexpr int G = M * HS;  // lanes per chain
    const int cpb = NTB / G;
    const int cl = tid / G, hpart = (tid % G) / M, m = tid % M, q = m & 3;
    const bool lead = (m == 0) && (hpart == 0);
    const int n_raw = blockIdx.x * cpb + cl;
    const bool valid = n_raw < N;
    const int n = valid ? n_raw : N - 1;
    const int gbase = lane - m;  // first lane of this chain's M-lane group inside the wave

    float* wf = smem;
    float* wg = wf + MQ::kSize;
    float* wqi = wg + MG::kSize;
    float* tile = wqi + MQ::kSize;  // 2 buffers of NP * PS floats

    MQ::load(wf, a.f, tid, NTB);
    MG::load(wg, a.g, tid, NTB);
    MQ::load(wqi, a.q1inv, tid, NTB);

    // ---- constants --------------------------------------------------------------------------
    float isf[DX], rp[DX], isg[DY];
    float kf = -DX * kHalfLog2Pi, kg = -DY * kHalfLog2Pi;
    const float rscale = sqrtf(0.5f * kLog2e);
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        const float s = a.sig_f[d];
        isf[d] = 1.f / s;
        rp[d] = isf[d] * rscale;  // (x' - F')^2 summed == 0.5*log2e*sum(((x-F)/s)^2)
        kf -= logf(s);
    }
#pragma unroll
    for (int e = 0; e < DY; ++e) {
        const float s = a.sig_g[e];
        isg[e] = 1.f / s;
        kg -= logf(s);
    }
    // PoG(q1_inv, BSim_q2) on scales (SVO.py:186-197 as called from PSVO.py:120-122)
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
    // q_init (t = T-1) and the t = 0 "filter" term
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
    float logM = logf((float)M);
    const float ninf = -__builtin_huge_valf();
    // the constants every step reads live in VGPRs (common.h: keep_in_vgpr): the scalar registers go to the array bases and
    // their strides.  (s_init, is_init, i_isig, im, mi, kinit, kiota are read in the first / last step only.)
    keep_in_vgpr(isf); keep_in_vgpr(rp); keep_in_vgpr(isg); keep_in_vgpr(pc); keep_in_vgpr(pic); keep_in_vgpr(pi1);
    keep_in_vgpr(pi2); keep_in_vgpr(kf); keep_in_vgpr(kg); keep_in_vgpr(kq); keep_in_vgpr(logM);

    // ---- addresses -----------------------------------------------------------------------------------
    // Every array is reached as  base (64-bit, wave-uniform: scalar registers) + 32-bit byte offset of the lane  -- the saddr
    // form, global_load_dword v, v_off, s[base:base+1].  The base points at the array's row (t, b) and moves back by the
    // row stride of the array's SHAPE once per step (two scalar adds); the lane's offset inside a row never changes and is
    // below 1 MiB for every shape the ABI admits (N <= 1024).  No multiply by t in the loop, and no limit on the size of an
    // array.  Three groups of bases travel one behind the other: the outputs at step t, the inputs at t - 1, the tile at t - 2.
    typedef unsigned long long u64;
    const u64 NM = (u64)N * M;
    // row strides (bytes) of (T,B), (T,B,N), (T,B,DX), (T,B,DY), (T,B,DX,N): below 2^32 (B <= 65535, N <= 1024); (T,B,N,M), (T,B,DX,N,M)
    const unsigned s_1 = 4u * B, s_n = s_1 * N, s_d = s_1 * DX, s_k = s_1 * DY, s_dn = s_n * DX;
    const u64 s_nm = s_1 * NM, s_dnm = s_nm * DX;
    const u64 r_1 = 4ull * ((u64)(T - 1) * B + b);                   // byte offset of row (T-1, b) in a (T,B) array
    const unsigned o_n = 4u * n, o_nm = 4u * (n * M + m), sN4 = 4u * N, sNM4 = 4u * N * M;   // lane offsets inside a row
    // (the offsets do not change from step to step: `here` keeps their zero-extension, which hipcc would hoist out of the
    //  loop as a 64-bit register pair, in the block of the access, where it folds into the saddr form)
    auto here = [](unsigned o) { asm volatile("" : "+v"(o)); return o; };
    auto here_s = [](int v) { asm volatile("" : "+s"(v)); return v; };      // (the same for a wave-uniform value)
    const bool forced = a.sel_in != nullptr;
    // inputs of the step that is requested next (sel_in and u_b are both 4-byte words of shape (T,B,N): one base, chosen once)
    u64 p_eps = (u64)a.eps_b + r_1 * (DX * NM), p_bmu = (u64)a.bmu2 + r_1 * DX, p_obs = (u64)a.obs + r_1 * DY,
        p_us = (forced ? (u64)a.sel_in : (u64)a.u_b) + r_1 * N;
    // forward tile that is requested next (T >= 2: the ABI refuses T = 1)
    u64 p_Fm = (u64)a.Fm + (r_1 - s_1) * (DX * N), p_logW = (u64)a.logW + (r_1 - s_1) * N, p_lse = (u64)a.lse + (r_1 - s_1);
    // outputs of the current step (the optional saves may be null: their bases are then never dereferenced)
    // which stores the lane makes, as bits of ONE register tested where they are used: as booleans they are lane masks, a
    // pair of scalar registers each, live across the whole loop (and with the bases in scalar registers, spilled to lanes)
    constexpr unsigned kOut = 1u, kMu1 = 2u, kLam2 = 4u, kOm = 8u;
    const unsigned lane_flags = (valid && lead ? kOut : 0u) | (a.mu1_all && valid && lead ? kMu1 : 0u) |
                                (a.lam2_all && valid && hpart == 0 ? kLam2 : 0u) | (a.om_all && valid && hpart == 0 ? kOm : 0u);
    auto stores = [&](unsigned bit) { return (here(lane_flags) & bit) != 0u; };
    u64 p_bwX = (u64)a.bwX + r_1 * (DX * N), p_mu1 = (u64)a.mu1_all + r_1 * (DX * N), p_glp = (u64)a.glp + r_1 * N,
        p_Om = (u64)a.Omega + r_1 * N, p_selo = (u64)a.sel_out + r_1 * N, p_flp = (u64)a.flp + r_1 * N,
        p_lam2 = (u64)a.lam2_all + r_1 * NM, p_omall = (u64)a.om_all + r_1 * NM;

    // ---- forward-tile staging -----------------------------------------------------------------
    // The global loads of step t-2's tile are issued at the top of step t and only *consumed* (scaled and
    // written to LDS) at its end: nothing between depends on them, so their latency hides behind the step.
    // A thread carries up to kMaxStage entries; how many is the same for the whole launch (nsets), and inside a set every
    // lane loads (a clamped entry where it has none), so that no load stands in a divergent region.
    const int nsets = (NP + NTB - 1) / NTB;
    float st[kMaxStage][DX + 1], st_l = 0.f;
#pragma unroll
    for (int r = 0; r < kMaxStage; ++r)
#pragma unroll
        for (int d = 0; d <= DX; ++d) st[r][d] = 0.f;
    auto stage_load = [&]() {  // global -> registers (raw), the forward step p_Fm / p_logW / p_lse point at
        st_l = ldf(as_global<const float>(p_lse), 0u);
#pragma unroll
        for (int r = 0; r < kMaxStage; ++r) {
            if (r == 0 || r < here_s(nsets)) {
                const unsigned oj = here(4u * (unsigned)min(tid + r * NTB, N - 1));
#pragma unroll
                for (int d = 0; d < DX; ++d) st[r][d] = ldf(as_global<const float>(p_Fm), oj + d * sN4);
                st[r][DX] = ldf(as_global<const float>(p_logW), oj);
            }
        }
    };
    auto stage_store = [&](float* buf) {  // registers -> LDS: F' = Fm * rho, W' = (logW - lse) * log2(e)
#pragma unroll
        for (int r = 0; r < kMaxStage; ++r) {
            const int j = (int)here(tid) + r * NTB;      // (compared here and now: no lane mask lives across the step)
            if ((r == 0 || r < here_s(nsets)) && j < NP) {
                float F[DX];
#pragma unroll
                for (int d = 0; d < DX; ++d) F[d] = st[r][d] * rp[d];
                const float W = j < N ? (st[r][DX] - st_l) * kLog2e : ninf;
                if constexpr (DX <= 3) {
                    float4 v;
                    v.x = F[0];
                    v.y = DX > 1 ? F[DX > 1 ? 1 : 0] : 0.f;
                    v.z = DX > 2 ? F[DX > 2 ? 2 : 0] : 0.f;
                    v.w = W;
                    *reinterpret_cast<float4*>(buf + j * PS) = v;
                } else {
                    *reinterpret_cast<float4*>(buf + j * PS) = make_float4(F[0], F[1], F[2], F[3]);
                    *reinterpret_cast<float4*>(buf + j * PS + 4) = make_float4(W, 0.f, 0.f, 0.f);
                }
            }
        }
    };

    // ---- per-step inputs, prefetched one step ahead ----------------------------------------------
    struct StepIn {
        float eps[DX], bmu[DX], obs[DY];
        int us;      // the uniform of the draw (bits of a float) or, teacher-forced, the index itself
    };
    auto load_inputs = [&](StepIn& s) {      // (issue only; the bases already point at the step to load)
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            s.eps[d] = ldf(as_global<const float>(p_eps), here(o_nm) + d * sNM4);
            s.bmu[d] = ldf(as_global<const float>(p_bmu), 4u * d);
        }
#pragma unroll
        for (int k = 0; k < DY; ++k) s.obs[k] = ldf(as_global<const float>(p_obs), 4u * k);
        s.us = ldi(as_global<const int32_t>(p_us), here(o_n));
    };
    // The wave waits for the words it requested in ONE place: `settle`, at the end of the step that requested them (in front
    // of the loop for step T-1 and the first tile).  The empty asm reads every word, so the s_waitcnt that guards them
    // stands there, and redefines it, so nothing later has a load to wait for.  Left to its own counting hipcc waits at the
    // first use, which for the words of step t is BEHIND the requests of step t - 1, and has to assume there the path with
    // the fewest requests: the wave then sat out the round trip of loads it had just issued, at the top of every step.
    // Every path of the loop passes through the settle, and every load of a step is issued on every path to it.
    // The words pass through the asm as aligned register PAIRS, so that each is loaded into a pair of its own.  A lone
    // register may end up as the unused half of a packed operand of the pair loop (v_pk_fma_f32 with op_sel_hi: the
    // broadcast W'), and hipcc guards the whole operand pair: a vmcnt(0) in the middle of the pair loop.
    auto settle = [&](StepIn& s) {
        constexpr int kW = 2 * DX + DY + 2 + kMaxStage * (DX + 1);
        float us = __int_as_float(s.us), pad = 0.f;
        float* w[kW + 1];
        int k = 0;
#pragma unroll
        for (int d = 0; d < DX; ++d) w[k++] = &s.eps[d];
#pragma unroll
        for (int d = 0; d < DX; ++d) w[k++] = &s.bmu[d];
#pragma unroll
        for (int e = 0; e < DY; ++e) w[k++] = &s.obs[e];
        w[k++] = &us;
        w[k++] = &st_l;
#pragma unroll
        for (int r = 0; r < kMaxStage; ++r)
#pragma unroll
            for (int d = 0; d <= DX; ++d) w[k++] = &st[r][d];
        w[k++] = &pad;
#pragma unroll
        for (int i = 0; i + 1 < kW + 1; i += 2) {
            f2 p = f2{*w[i], *w[i + 1]};
            asm volatile("" : "+v"(p));
            *w[i] = p.x;
            *w[i + 1] = p.y;
        }
        s.us = __float_as_int(us);
    };
    StepIn cur_in;
    load_inputs(cur_in);
    stage_load();
    settle(cur_in);
    stage_store(tile);
    __syncthreads();

    float xp[DX];  // x_{t+1} of this chain (same in all M lanes)
#pragma unroll
    for (int d = 0; d < DX; ++d) xp[d] = 0.f;
    float score = 0.f;

    SEC_INIT(bsim_fwd)
    // the steps t = T-1 (initial proposal, no successor) and t = 0 (prior term instead of the tile pass) are peeled:
    // the T-2 steps in between carry none of their branches
    auto step = [&](auto last_tag, auto zero_tag, const int t) {
        SEC(0);   // loop overhead / barrier tail
        const float* cur = tile + ((T - 1 - t) & 1) * NP * PS;
        float* nxt = tile + ((T - t) & 1) * NP * PS;
        const bool last = last_tag;                 // (compile-time constants in the peeled instantiations)
        const bool tzero = zero_tag;
        // the peeled step t = 0 requests nothing; everywhere else every load is issued in every step.  Where there is no
        // step t - 1 (the unpeeled loop at t = 0) or no tile t - 2 (t <= 1) the bases stay where they are: the words of the
        // row they point at are requested once more and dropped.
        constexpr bool kNoPrefetch = std::is_same<decltype(zero_tag), std::true_type>::value;
        StepIn nxt_in;
        if constexpr (!kNoPrefetch) {
            const bool in_step = kPeel || t >= 1, tile_step = t >= 2;
            p_eps -= in_step ? s_dnm : 0; p_bmu -= in_step ? s_d : 0; p_obs -= in_step ? s_k : 0; p_us -= in_step ? s_n : 0;
            load_inputs(nxt_in);
            p_Fm -= tile_step ? s_dn : 0; p_logW -= tile_step ? s_n : 0; p_lse -= tile_step ? s_1 : 0;
            stage_load();
        }

        SEC(1);   // issue of the prefetch loads
        // ---- proposal ---------------------------------------------------------------------------
        float x[DX], q_lp;
        if (last) {
            float mu[DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                mu[d] = mi[d];
                x[d] = fmaf(s_init[d], cur_in.eps[d], mu[d]);
            }
            q_lp = diag_lp<DX>(x, mu, is_init, kinit);
            if (stores(kMu1)) {
#pragma unroll
                for (int d = 0; d < DX; ++d) stf(as_global<float>(p_mu1), here(o_n) + d * sN4, 0.f);
            }
        } else {
            float m1[DX], mu[DX];
            {   // x_{t+1} is the same in all G lanes of the chain: spread MLP_q1inv's hidden units over kQS of them
                constexpr int kQS = (H / 4 < G) ? H / 4 : G;
                MQ::template eval_part<kQS>(wqi, (tid % G) & (kQS - 1), xp, m1);
#pragma unroll
                for (int d = 0; d < DX; ++d) m1[d] = kDiet ? group_sum2<kQS>(m1[d]) : group_sum<kQS>(m1[d]);
            }
            if (stores(kMu1)) {
#pragma unroll
                for (int d = 0; d < DX; ++d) stf(as_global<float>(p_mu1), here(o_n) + d * sN4, m1[d]);
            }
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                mu[d] = pc[d] * fmaf(pi1[d], m1[d], pi2[d] * cur_in.bmu[d]);
                x[d] = fmaf(pc[d], cur_in.eps[d], mu[d]);
            }
            q_lp = diag_lp<DX>(x, mu, pic, kq);
        }

        SEC(2);   // MLP_q1inv + proposal
        // ---- f(x_{t+1} | x~), g(y_t | x~) ------------------------------------------------------------
        float phi = 0.f;
        if (!last) {
            float fmx[DX];
            if constexpr (HS == 1) {
                MQ::template eval<kRolled>(wf, x, fmx);
            } else {
                MQ::template eval_part<HS, ilog2(M)>(wf, hpart, x, fmx);
#pragma unroll
                for (int d = 0; d < DX; ++d) fmx[d] = kDiet ? add_xor<M>(fmx[d]) : fmx[d] + xor_lane<M>(fmx[d]);
            }
            phi = diag_lp<DX>(xp, fmx, isf, kf);
        }
        float gm[DY];
        if constexpr (HS == 1) {
            MG::template eval<kRolled>(wg, x, gm);
        } else {
            MG::template eval_part<HS, ilog2(M)>(wg, hpart, x, gm);
#pragma unroll
            for (int k = 0; k < DY; ++k) gm[k] = kDiet ? add_xor<M>(gm[k]) : gm[k] + xor_lane<M>(gm[k]);
        }
        if (a.emission) {
#pragma unroll
            for (int k = 0; k < DY; ++k) gm[k] = emis_mean(gm[k]);
        }
        const float g_lp = diag_lp<DY>(cur_in.obs, gm, isg, kg);

        SEC(3);   // MLP_f, MLP_g, densities
        // ---- filter term: logsumexp_j( log f(x~ | X_{t-1}[j]) + W^_{t-1}[j] ) -----------------------
        float lam;
        if (!tzero) {
            float xq[4][DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                float t4[4];
                quad_bcast4(x[d] * rp[d], t4);
#pragma unroll
                for (int i = 0; i < 4; ++i) xq[i][d] = t4[i];
            }
            // The lane walks its quad-slice of the forward tile in blocks of JB entries (4 pairs per entry:
            // the quad's four sub-particles).  Phase A forms every v of the block with packed f32 math
            // (v_pk_add_f32 / v_pk_fma_f32 / v_pk_max_f32: sub-particles (0,1) and (2,3) share an instruction)
            // and the block maximum; phase B rescales the running sums ONCE per block and adds the block's
            // exponentials.  At C* one block covers the lane's whole slice, so no rescaling remains.
            f2 xa[DX], xb[DX];
#pragma unroll
            for (int d = 0; d < DX; ++d) {
                xa[d] = f2{xq[0][d], xq[1][d]};
                xb[d] = f2{xq[2][d], xq[3][d]};
            }
            f2 mxa = f2{ninf, ninf}, mxb = mxa, sma = f2{0.f, 0.f}, smb = sma;
            const int nqh = (NP >> 2) / HS;       // forward-tile entries per quad lane and half (multiple of 4)
            const int j0 = hpart * nqh;
            // (the first block of a step takes its sums from its own exponentials and its maximum as the running one:
            //  0 * exp2(-inf - base) + x == x bit for bit, so the rescale of sums that are still zero is left out)
            auto block = [&](auto jb_tag, auto first_tag, int k0) {
                constexpr int JB = decltype(jb_tag)::value;
                constexpr bool kFirst = decltype(first_tag)::value;
                f2 va[JB], vb[JB];
                f2 bma = f2{ninf, ninf}, bmb = bma;
#pragma unroll
                for (int c = 0; c < JB; ++c) {
                    const float* p = cur + ((j0 + k0 + c) * 4 + q) * PS;
                    float F[DX], W;
                    if constexpr (DX <= 3) {
                        const float4 sl = *reinterpret_cast<const float4*>(p);
                        F[0] = sl.x;
                        if (DX > 1) F[DX > 1 ? 1 : 0] = sl.y;
                        if (DX > 2) F[DX > 2 ? 2 : 0] = sl.z;
                        W = sl.w;
                    } else {
                        const float4 sl = *reinterpret_cast<const float4*>(p);
                        F[0] = sl.x; F[1] = sl.y; F[2] = sl.z; F[3] = sl.w;
                        W = p[4];
                    }
                    f2 la = f2{W, W}, lb = la;
#pragma unroll
                    for (int d = 0; d < DX; ++d) {
                        const f2 Fd = f2{F[d], F[d]};
                        const f2 ua = xa[d] - Fd, ub = xb[d] - Fd;
                        la = pk_fma(-ua, ua, la);
                        lb = pk_fma(-ub, ub, lb);
                    }
                    va[c] = la;
                    vb[c] = lb;
                    bma = pk_max(bma, la);
                    bmb = pk_max(bmb, lb);
                }
                f2 nma = bma, nmb = bmb;
                if constexpr (!kFirst) {
                    nma = pk_max(mxa, bma);
                    nmb = pk_max(mxb, bmb);
                }
                // nm == -inf only if every term so far is -inf: keep s = 0 without NaNs
                const f2 ba = f2{nma.x == ninf ? 0.f : nma.x, nma.y == ninf ? 0.f : nma.y};
                const f2 bb = f2{nmb.x == ninf ? 0.f : nmb.x, nmb.y == ninf ? 0.f : nmb.y};
                if constexpr (!kFirst) {
                    const f2 ra = mxa - ba, rb = mxb - bb;
                    sma = sma * f2{exp2_fast(ra.x), exp2_fast(ra.y)};
                    smb = smb * f2{exp2_fast(rb.x), exp2_fast(rb.y)};
                }
#pragma unroll
                for (int c = 0; c < JB; ++c) {
                    const f2 da = va[c] - ba, db = vb[c] - bb;
                    const f2 ea = f2{exp2_fast(da.x), exp2_fast(da.y)}, eb = f2{exp2_fast(db.x), exp2_fast(db.y)};
                    if (kFirst && c == 0) {
                        sma = ea;
                        smb = eb;
                    } else {
                        sma += ea;
                        smb += eb;
                    }
                }
                mxa = nma;
                mxb = nmb;
            };
            // (nqh is wave-uniform and a multiple of 4.  Only the 16-entry arm has a first-block form: with one for the 8- and
            //  the 4-entry arm as well most instantiations spilled two to four scalar registers more, profiles/bsim_fwd_valu_diet.md;
            //  a slice shorter than 16 entries starts with the general form, which is right for a first block too.)
            using I16 = std::integral_constant<int, 16>;
            int k0 = 0;
            if constexpr (kFirstBlock) {
                if (nqh >= 16) {
                    block(I16{}, std::true_type{}, 0);
                    k0 = 16;
                }
            }
            for (; k0 + 16 <= nqh; k0 += 16) block(I16{}, std::false_type{}, k0);
            if (nqh - k0 >= 8) {
                block(std::integral_constant<int, 8>{}, std::false_type{}, k0);
                k0 += 8;
            }
            if (nqh - k0 >= 4) block(std::integral_constant<int, 4>{}, std::false_type{}, k0);
            SEC(4);   // pair loop
            const float mx[4] = {mxa.x, mxa.y, mxb.x, mxb.y};
            const float sm[4] = {sma.x, sma.y, smb.x, smb.y};
            // merge the four j-slices of the quad (lane q keeps sub-particle i == q) and the chain's halves:
            // common maximum first, then ONE rescale of the lane's own sum and plain adds.  The maxima are all-reduced over
            // the quad and the halves (every lane rescales all four of its sums); the sums are all-reduced over the quad
            // only, and the other half's quad sum is added to the ONE sum the lane keeps (the partner lane, lane ^ M, has
            // the same q): (quad sum) + (other half's quad sum), as before.
            float lm = ninf, ls = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float gm;
                if constexpr (kDiet) {
                    gm = max_xor<2>(max_xor<1>(mx[i]));
                    if constexpr (HS == 2) gm = max_xor<M>(gm);
                } else {
                    gm = fmaxf(mx[i], xor_lane<1>(mx[i]));
                    gm = fmaxf(gm, xor_lane<2>(gm));
                    if constexpr (HS == 2) gm = fmaxf(gm, xor_lane<M>(gm));
                }
                const float base = (gm == ninf) ? 0.f : gm;
                float sc = sm[i] * exp2_fast(mx[i] - base);    // (mx = -inf: sm = 0 and exp2(-inf) = 0)
                if constexpr (kDiet) {
                    sc = add_xor<2>(add_xor<1>(sc));
                } else {
                    sc += xor_lane<1>(sc);
                    sc += xor_lane<2>(sc);
                }
                if constexpr (HS == 2 && !kDiet) sc += xor_lane<M>(sc);
                if (i == q) {
                    lm = gm;
                    ls = sc;
                }
            }
            if constexpr (HS == 2 && kDiet) ls = add_xor<M>(ls);
            const float lam2 = lm + log2_fast(ls);
            lam = fmaf(kLn2, lam2, kf);
            if (stores(kLam2)) stf(as_global<float>(p_lam2), here(o_nm), lam2);
        } else {
            lam = diag_lp<DX>(x, im, i_isig, kiota);  // t = 0: q0 / f density at mu_0 (PSVO.py:169-175)
        }

        SEC(5);   // quad / half merges, lam2
        // ---- omega, normalise over the M sub-particles, draw one ---------------------------------------
        const float om_raw = lam + phi + g_lp - q_lp;
        const float omx = kDiet ? group_max2<M>(om_raw) : group_max<M>(om_raw);
        const float pw = exp2_fast((om_raw - omx) * kLog2e);
        const float cdfv = kDiet ? group_incl_scan2<M>(pw, m) : group_incl_scan<M>(pw, m);  // inclusive scan across the chain's M lanes
        const float total = __shfl(cdfv, gbase + M - 1);
        const float omega = om_raw - fmaf(kLn2, log2_fast(total), omx);
        if (stores(kOm)) stf(as_global<float>(p_omall), here(o_nm), omega);
        int sel;
        if (forced) {
            sel = cur_in.us;
        } else {
            const unsigned long long bal = __ballot(cdfv <= __int_as_float(cur_in.us) * total);
            const unsigned long long mask = (M == 64) ? ~0ull : (((1ull << M) - 1ull) << gbase);
            sel = min((int)__popcll(bal & mask), M - 1);
        }
        const int src = gbase + sel;
        float xs[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) xs[d] = __shfl(x[d], src);
        const float om_s = __shfl(omega, src);
        const float phi_s = __shfl(phi, src);
        SEC(6);   // normalise over M, draw
        const float g_s = __shfl(g_lp, src);
        const float q_s = __shfl(q_lp, src);
        const float lam_s = __shfl(lam, src);
        const float Om = om_s + q_s + logM;

        // the words requested at the top of this step become the next step's here, in front of the step's own output
        // stores: the wait covers the loads and none of the stores behind it
        if constexpr (!kNoPrefetch) {
            settle(nxt_in);
            cur_in = nxt_in;
        }
        if (stores(kOut)) {
            const unsigned on = here(o_n);
#pragma unroll
            for (int d = 0; d < DX; ++d) stf(as_global<float>(p_bwX), on + d * sN4, xs[d]);
            stf(as_global<float>(p_glp), on, g_s);
            stf(as_global<float>(p_Om), on, Om);
            sti(as_global<int32_t>(p_selo), on, sel);
            if (!last) stf(as_global<float>(p_flp + s_n), on, phi_s);     // f_log_probs[t+1]
            if (tzero) stf(as_global<float>(p_flp), on, lam_s);           // f_log_probs[0] = f_init
        }
        score += g_s - Om + (last ? 0.f : phi_s) + (tzero ? lam_s : 0.f);
#pragma unroll
        for (int d = 0; d < DX; ++d) xp[d] = xs[d];

        SEC(7);   // gather of the selected sub-particle, settle of the prefetched words, output stores
        if (t >= 2) stage_store(nxt);
        __syncthreads();
        // the outputs' bases move on to step t - 1
        p_bwX -= s_dn; p_mu1 -= s_dn; p_glp -= s_n; p_Om -= s_n; p_selo -= s_n; p_flp -= s_n; p_lam2 -= s_nm; p_omall -= s_nm;
        SEC(8);   // tile store + barrier
    };
    if constexpr (kPeel) {
        step(std::true_type{}, std::false_type{}, T - 1);
        for (int t = T - 2; t >= 1; --t) step(std::false_type{}, std::false_type{}, t);
        step(std::false_type{}, std::true_type{}, 0);
    } else {
        for (int t = T - 1; t >= 0; --t) step(t == T - 1, t == 0, t);
    }
    if (valid && lead) a.score[(size_t)b * N + n] = score;
}

template <int DX, int DY, int H, int M>
static int launch_bsim(const BsimArgs& a, hipStream_t stream) {
    using MQ = MlpLds<DX, H, DX, PSVO_L>;
    using MG = MlpLds<DX, H, DY, PSVO_L>;
    constexpr int PS = TileSlot<DX>::kFloats;
    // fewer than two waves per SIMD (1024 SIMDs) with one lane per (chain, m): spread each chain over 2M lanes
    const long long waves1 = ((long long)a.B * a.N * M + 63) / 64;
    const int HS = (waves1 < 2048 && 2 * M <= 64 && (H / 2) % 4 == 0 && (PSVO_L == 1 || g_tune_l2_split)) ? 2 : 1;
    const int NP = ((a.N + 16 * HS - 1) / (16 * HS)) * (16 * HS);
    int NTB = ((a.N * M * HS + 63) / 64) * 64;
    if (NTB > 256) NTB = 256;
    const int cpb = NTB / (M * HS);
    const size_t lds = sizeof(float) * (2 * MQ::kSize + MG::kSize + 2 * (size_t)NP * PS);
    dim3 grid((a.N + cpb - 1) / cpb, a.B);
    clear_hip_error();
    if (HS == 2) {
        if constexpr (2 * M <= 64 && (H / 2) % 4 == 0)
            hipLaunchKernelGGL((bsim_fwd_kernel<DX, DY, H, M, 2>), grid, dim3(NTB), lds, stream, a);
    } else {
        hipLaunchKernelGGL((bsim_fwd_kernel<DX, DY, H, M, 1>), grid, dim3(NTB), lds, stream, a);
    }
    return launch_status();
}

}  // inline namespace PSVO_LNS
}  // namespace psvo

PSVO_L2_DECL(psvo_bsim_forward)
PSVO_ENTRY(psvo_bsim_forward)(const psvo_desc* desc, const float* X, const float* Fm, const float* logW,
                                 const float* lse, const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                                 const float* sig_f, const float* sig_g, const float* sig_q1inv,
                                 const float* sig_bq2, const float* bmu2, const float* minit,
                                 const float* sig_init, const float* imean, const float* isig, const float* obs,
                                 const float* eps_b, const float* u_b, const int32_t* sel_in, float* bwX,
                                 float* flp, float* glp, float* Omega, int32_t* sel_out, float* score,
                                 float* lam2_all, float* om_all, float* mu1_all,
                                 void* stream) {
    using namespace psvo;
    if (!desc_layers_ok(desc) || !desc_emission_ok(desc)) return PSVO_ERR_UNSUPPORTED;
#if PSVO_L == 1
    if (desc && desc->layers == 2)
        return psvo_bsim_forward_l2(desc, X, Fm, logW, lse, f, g, q1_inv, sig_f, sig_g, sig_q1inv, sig_bq2, bmu2,
            minit, sig_init, imean, isig, obs, eps_b, u_b, sel_in, bwX, flp, glp, Omega, sel_out, score, lam2_all,
            om_all, mu1_all, stream);
#endif
    if (!mlp_layers_ok(f) || !mlp_layers_ok(g) || !mlp_layers_ok(q1_inv)) return PSVO_ERR_INVALID;
    if (!desc || !Fm || !logW || !lse || !f || !g || !q1_inv || !sig_f || !sig_g || !sig_q1inv || !sig_bq2 ||
        !bmu2 || !minit || !sig_init || !imean || !isig || !obs || !eps_b || !bwX || !flp || !glp || !Omega ||
        !sel_out || !score)
        return PSVO_ERR_INVALID;
    if (!u_b && !sel_in) return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T < 2 || desc->N <= 0 || desc->M <= 0) return PSVO_ERR_INVALID;
    if (desc->N > 1024 || desc->B > 65535) return PSVO_ERR_UNSUPPORTED;
    (void)X;

    BsimArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.emission = desc->emission;
    a.f = *f; a.g = *g; a.q1inv = *q1_inv;
    a.X = X; a.Fm = Fm; a.logW = logW; a.lse = lse;
    a.sig_f = sig_f; a.sig_g = sig_g; a.sig_q1inv = sig_q1inv; a.sig_bq2 = sig_bq2;
    a.bmu2 = bmu2; a.minit = minit; a.sig_init = sig_init; a.imean = imean; a.isig = isig;
    a.obs = obs; a.eps_b = eps_b; a.u_b = u_b; a.sel_in = sel_in;
    a.bwX = bwX; a.flp = flp; a.glp = glp; a.Omega = Omega; a.sel_out = sel_out; a.score = score;
    a.lam2_all = lam2_all; a.om_all = om_all; a.mu1_all = mu1_all;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch_shape_m(desc->Dx, desc->Dy, desc->H, desc->M, [&](auto dx, auto dy, auto h, auto m) {
        return launch_bsim<dx(), dy(), h(), m()>(a, s); });
}
