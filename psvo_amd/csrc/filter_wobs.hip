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
// The two filter kernels live in filter_wobs_impl.h, compiled twice: as they were, and in their adaptive-resampling form
// (psvo_filter_forward_wobs_adaptive / psvo_filter_backward_wobs_adaptive: 18 forward and 18 reverse kernels more, no EXT form).
// A third compilation is the missing-observation form (psvo_filter_forward_wobs_missing / psvo_filter_backward_wobs_missing: a NaN
// in obs is an observation that was not made; 1 <= Dy <= 32; 18 forward and 36 reverse kernels more: the EXT forms sit behind
// psvo_filter_backward_wobs_missing_ext, for the missing-observation backward simulation of bsim_wobs_ms.hip).
// A fourth is both at once (psvo_filter_forward_wobs_missing_adaptive / psvo_filter_backward_wobs_missing_adaptive: the adaptive
// argument blocks, the missing-observation form's LDS; 1 <= Dy <= 32; 18 forward and 18 reverse kernels more, no EXT form).
// A fifth, the missing-observation form with input-driven transitions, is a unit of its own: filter_wobs_in.hip.
// (the argument blocks, LDS sizes, envelope and dispatch: filter_wobs_args.h, shared with filter_wobs_in.hip)
#include "filter_wobs_args.h"

namespace psvo {
namespace wobs {

// the kernels (filter_wobs_impl.h): the static pair, then the adaptive pair, then the missing-observation pair, then the
// adaptive missing-observation pair
#define PSVO_AD 0
#include "filter_wobs_impl.h"
#undef PSVO_AD
#define PSVO_AD 1
#include "filter_wobs_impl.h"
#undef PSVO_AD
#define PSVO_AD 0
#define PSVO_MS 1
#include "filter_wobs_impl.h"
#undef PSVO_AD
#define PSVO_AD 1
#include "filter_wobs_impl.h"
#undef PSVO_MS
#undef PSVO_AD

template <int DX, int H, bool AD = false, bool MS = false>
static int launch_fwd(const FwdArgsT<AD>& a, hipStream_t stream) {
    const int NT = (a.N + 63) & ~63;
    const bool count = a.emission == 2;
    const size_t lds = fwd_lds_bytes<DX, H>(NT, count, MS);
    clear_hip_error();
    if constexpr (MS && AD) {     // (the missing-observation form's LDS: the adaptive form's red[40 + wave] lies ahead of the cg row)
        if (count) hipLaunchKernelGGL((filter_fwd_wobs_msad_kernel<DX, H, true>), dim3(a.B), dim3(NT), lds, stream, a);
        else hipLaunchKernelGGL((filter_fwd_wobs_msad_kernel<DX, H, false>), dim3(a.B), dim3(NT), lds, stream, a);
    } else if constexpr (MS) {
        if (count) hipLaunchKernelGGL((filter_fwd_wobs_ms_kernel<DX, H, true>), dim3(a.B), dim3(NT), lds, stream, a);
        else hipLaunchKernelGGL((filter_fwd_wobs_ms_kernel<DX, H, false>), dim3(a.B), dim3(NT), lds, stream, a);
    } else if constexpr (AD) {
        if (count) hipLaunchKernelGGL((filter_fwd_wobs_ad_kernel<DX, H, true>), dim3(a.B), dim3(NT), lds, stream, a);
        else hipLaunchKernelGGL((filter_fwd_wobs_ad_kernel<DX, H, false>), dim3(a.B), dim3(NT), lds, stream, a);
    } else {
    if (count) hipLaunchKernelGGL((filter_fwd_wobs_kernel<DX, H, true>), dim3(a.B), dim3(NT), lds, stream, a);
    else hipLaunchKernelGGL((filter_fwd_wobs_kernel<DX, H, false>), dim3(a.B), dim3(NT), lds, stream, a);
    }
    return launch_status();
}


template <int DX, int H, bool AD = false, bool MS = false>
static int launch_bwd(const BwdArgsT<AD>& a, const BwdOut& o, hipStream_t stream) {
    const int NT = (a.N + 63) & ~63;
    const size_t lds = bwd_lds_bytes<DX, H>(NT, a.Dy, a.bootstrap != 0);
    clear_hip_error();
    const bool ext = a.dFm_ext || a.dlogW_ext;
    if constexpr (MS && AD) {     // (no EXT form, as for either twin)
        (void)ext;
        if (a.emission == 2) hipLaunchKernelGGL((filter_bwd_wobs_msad_kernel<DX, H, false, true>), dim3(a.B), dim3(NT), lds, stream, a);
        else hipLaunchKernelGGL((filter_bwd_wobs_msad_kernel<DX, H, false, false>), dim3(a.B), dim3(NT), lds, stream, a);
    } else if constexpr (MS) {     // (EXT: psvo_filter_backward_wobs_missing_ext, the missing backward simulation behind it)
        if (a.emission == 2) {
            if (ext) hipLaunchKernelGGL((filter_bwd_wobs_ms_kernel<DX, H, true, true>), dim3(a.B), dim3(NT), lds, stream, a);
            else hipLaunchKernelGGL((filter_bwd_wobs_ms_kernel<DX, H, false, true>), dim3(a.B), dim3(NT), lds, stream, a);
        } else {
            if (ext) hipLaunchKernelGGL((filter_bwd_wobs_ms_kernel<DX, H, true, false>), dim3(a.B), dim3(NT), lds, stream, a);
            else hipLaunchKernelGGL((filter_bwd_wobs_ms_kernel<DX, H, false, false>), dim3(a.B), dim3(NT), lds, stream, a);
        }
    } else if constexpr (AD) {     // (no EXT form: no backward simulation runs behind an adaptive filter)
        (void)ext;
        if (a.emission == 2) hipLaunchKernelGGL((filter_bwd_wobs_ad_kernel<DX, H, false, true>), dim3(a.B), dim3(NT), lds, stream, a);
        else hipLaunchKernelGGL((filter_bwd_wobs_ad_kernel<DX, H, false, false>), dim3(a.B), dim3(NT), lds, stream, a);
    } else if (a.emission == 2) {
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

// the checks and the launch behind psvo_filter_forward_wobs (ad == nullptr), psvo_filter_forward_wobs_adaptive,
// psvo_filter_forward_wobs_missing (ms) and psvo_filter_forward_wobs_missing_adaptive (ad and ms)
static int filter_forward_wobs_checked(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                       const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                                       const float* mu2, const float* m0, const float* sig0, const float* fm0,
                                       const float* fsig0, const float* obs, const float* eps, const float* u,
                                       const int32_t* idx_in, float* X, float* Xanc, float* Fm, float* P1, float* logW,
                                       int32_t* idx_out, float* lse, const psvo::wobs::FwdArgsAd* ad, void* stream,
                                       bool ms = false) {
    using namespace psvo;
    using namespace psvo::wobs;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!desc || !q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X || !Xanc || !Fm ||
        !logW || !idx_out || !lse)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (ms && desc->T < 2) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f)) return PSVO_ERR_INVALID;
    if (desc->resample && !u && !idx_in) return PSVO_ERR_INVALID;
    if (!filter_shape_ok(desc, ms ? 1 : 3)) return PSVO_ERR_UNSUPPORTED;

    FwdArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy;
    a.resample = desc->resample; a.two_q = desc->two_q; a.bootstrap = desc->bootstrap; a.emission = desc->emission;
    a.q1 = *q1; a.f = desc->bootstrap ? *q1 : *f; a.g = *g;
    a.sig_q1 = sig_q1; a.sig_q2 = sig_q2; a.sig_f = sig_f; a.sig_g = sig_g;
    a.mu2 = mu2; a.m0 = m0; a.sig0 = sig0; a.fm0 = fm0; a.fsig0 = fsig0;
    a.obs = obs; a.eps = eps; a.u = u; a.idx_in = idx_in;
    a.X = X; a.Xanc = Xanc; a.Fm = Fm; a.P1 = P1; a.logW = logW; a.idx_out = idx_out; a.lse = lse;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ad) {
        FwdArgsAd aa;
        static_cast<FwdArgs&>(aa) = a;
        aa.ess_frac = ad->ess_frac; aa.rs_in = ad->rs_in; aa.rs_out = ad->rs_out; aa.ess_out = ad->ess_out;
        if (ms) return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_fwd<dx(), h(), true, true>(aa, s); });
        return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_fwd<dx(), h(), true>(aa, s); });
    }
    if (ms) return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_fwd<dx(), h(), false, true>(a, s); });
    return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_fwd<dx(), h()>(a, s); });
}

extern "C" int psvo_filter_forward_wobs_missing(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                                const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                                                const float* mu2, const float* m0, const float* sig0, const float* fm0,
                                                const float* fsig0, const float* obs, const float* eps, const float* u,
                                                const int32_t* idx_in, float* X, float* Xanc, float* Fm, float* P1, float* logW,
                                                int32_t* idx_out, float* lse, void* stream) {
    return filter_forward_wobs_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, u, idx_in,
                                       X, Xanc, Fm, P1, logW, idx_out, lse, nullptr, stream, true);
}

extern "C" int psvo_filter_forward_wobs(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                        const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                                        const float* mu2, const float* m0, const float* sig0, const float* fm0,
                                        const float* fsig0, const float* obs, const float* eps, const float* u,
                                        const int32_t* idx_in, float* X, float* Xanc, float* Fm, float* P1, float* logW,
                                        int32_t* idx_out, float* lse, void* stream) {
    return filter_forward_wobs_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, u, idx_in,
                                       X, Xanc, Fm, P1, logW, idx_out, lse, nullptr, stream);
}

extern "C" int psvo_filter_forward_wobs_adaptive(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f,
                                                 const psvo_mlp* g, const float* sig_q1, const float* sig_q2,
                                                 const float* sig_f, const float* sig_g, const float* mu2, const float* m0,
                                                 const float* sig0, const float* fm0, const float* fsig0, const float* obs,
                                                 const float* eps, const float* u, const int32_t* idx_in, float* X,
                                                 float* Xanc, float* Fm, float* P1, float* logW, int32_t* idx_out, float* lse,
                                                 float ess_frac, const int32_t* rs_in, int32_t* rs_out, float* ess_out,
                                                 void* stream) {
    // the adaptive contract first: a threshold (NaN is none), a filter that resamples at all, somewhere to record the decisions
    if (!desc || !(ess_frac > 0.f) || !desc->resample || !rs_out || !ess_out) return PSVO_ERR_INVALID;
    psvo::wobs::FwdArgsAd ad;
    ad.ess_frac = ess_frac; ad.rs_in = rs_in; ad.rs_out = rs_out; ad.ess_out = ess_out;
    return filter_forward_wobs_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, u, idx_in,
                                       X, Xanc, Fm, P1, logW, idx_out, lse, &ad, stream);
}

extern "C" int psvo_filter_forward_wobs_missing_adaptive(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f,
                                                         const psvo_mlp* g, const float* sig_q1, const float* sig_q2,
                                                         const float* sig_f, const float* sig_g, const float* mu2,
                                                         const float* m0, const float* sig0, const float* fm0,
                                                         const float* fsig0, const float* obs, const float* eps, const float* u,
                                                         const int32_t* idx_in, float* X, float* Xanc, float* Fm, float* P1,
                                                         float* logW, int32_t* idx_out, float* lse, float ess_frac,
                                                         const int32_t* rs_in, int32_t* rs_out, float* ess_out, void* stream) {
    // the adaptive contract first, as psvo_filter_forward_wobs_adaptive has it; then the missing pair's envelope
    if (!desc || !(ess_frac > 0.f) || !desc->resample || !rs_out || !ess_out) return PSVO_ERR_INVALID;
    psvo::wobs::FwdArgsAd ad;
    ad.ess_frac = ess_frac; ad.rs_in = rs_in; ad.rs_out = rs_out; ad.ess_out = ess_out;
    return filter_forward_wobs_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, u, idx_in,
                                       X, Xanc, Fm, P1, logW, idx_out, lse, &ad, stream, true);
}

extern "C" long long psvo_filter_wobs_ws_floats(int B, int T, int N, int Dx, int Dy) {
    return (long long)B * (10 * Dx + Dy) + (long long)T * B * Dx * N;
}

// the checks and the launch behind psvo_filter_backward_wobs(_ext) (rs == nullptr), psvo_filter_backward_wobs_adaptive,
// psvo_filter_backward_wobs_missing (ms) and psvo_filter_backward_wobs_missing_adaptive (rs and ms)
static int filter_backward_wobs_checked(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, int nparts,
    const float* dFm_ext, const float* dlogW_ext, float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
    float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0, float* ws, const int32_t* rs,
    void* stream, bool ms = false) {
    using namespace psvo;
    using namespace psvo::wobs;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!desc || !q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X || !Fm || !logW ||
        !lse || !dP || !dG || !dm0 || !dfm0 || !dsig_q1 || !dsig_q2 || !dsig_f || !dsig_g || !dsig0 || !dfsig0 || !ws)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (ms && desc->T < 2) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2 || !dmu2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f || !P1 || !dF)) return PSVO_ERR_INVALID;
    if (desc->resample && !idx) return PSVO_ERR_INVALID;
    if ((dFm_ext || dlogW_ext) && nparts <= 0) return PSVO_ERR_INVALID;
    if (!filter_shape_ok(desc, ms ? 1 : 3)) return PSVO_ERR_UNSUPPORTED;

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
    if (rs) {
        BwdArgsAd aa;
        static_cast<BwdArgs&>(aa) = a;
        aa.rs = rs;
        if (ms) return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_bwd<dx(), h(), true, true>(aa, o, s); });
        return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_bwd<dx(), h(), true>(aa, o, s); });
    }
    if (ms) return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_bwd<dx(), h(), false, true>(a, o, s); });
    return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_bwd<dx(), h()>(a, o, s); });
}

extern "C" int psvo_filter_backward_wobs_missing(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, float* dP, float* dF,
    float* dG, float* dmu2, float* dm0, float* dfm0, float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g,
    float* dsig0, float* dfsig0, float* ws, void* stream) {
    return filter_backward_wobs_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, X, Fm,
                                        P1, logW, lse, idx, dlse, 0, nullptr, nullptr, dP, dF, dG, dmu2, dm0, dfm0, dsig_q1,
                                        dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, ws, nullptr, stream, true);
}

// (the EXT = true instantiations of filter_bwd_wobs_ms_kernel when dFm_ext or dlogW_ext is given: 18 kernels, no new text)
extern "C" int psvo_filter_backward_wobs_missing_ext(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, int nparts,
    const float* dFm_ext, const float* dlogW_ext, float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
    float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0, float* ws, void* stream) {
    return filter_backward_wobs_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, X, Fm,
                                        P1, logW, lse, idx, dlse, nparts, dFm_ext, dlogW_ext, dP, dF, dG, dmu2, dm0, dfm0,
                                        dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, ws, nullptr, stream, true);
}

extern "C" int psvo_filter_backward_wobs_ext(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, int nparts,
    const float* dFm_ext, const float* dlogW_ext, float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
    float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0, float* ws, void* stream) {
    return filter_backward_wobs_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, X, Fm,
                                        P1, logW, lse, idx, dlse, nparts, dFm_ext, dlogW_ext, dP, dF, dG, dmu2, dm0, dfm0,
                                        dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, ws, nullptr, stream);
}

extern "C" int psvo_filter_backward_wobs_adaptive(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, float* dP, float* dF,
    float* dG, float* dmu2, float* dm0, float* dfm0, float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g,
    float* dsig0, float* dfsig0, float* ws, const int32_t* rs, void* stream) {
    // the adaptive contract first: a filter that resamples at all, and the decisions it took
    if (!desc || !desc->resample || !rs) return PSVO_ERR_INVALID;
    return filter_backward_wobs_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, X, Fm,
                                        P1, logW, lse, idx, dlse, 0, nullptr, nullptr, dP, dF, dG, dmu2, dm0, dfm0, dsig_q1,
                                        dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, ws, rs, stream);
}

extern "C" int psvo_filter_backward_wobs_missing_adaptive(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, float* dP, float* dF,
    float* dG, float* dmu2, float* dm0, float* dfm0, float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g,
    float* dsig0, float* dfsig0, float* ws, const int32_t* rs, void* stream) {
    // the adaptive contract first, as psvo_filter_backward_wobs_adaptive has it; then the missing pair's envelope
    if (!desc || !desc->resample || !rs) return PSVO_ERR_INVALID;
    return filter_backward_wobs_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, X, Fm,
                                        P1, logW, lse, idx, dlse, 0, nullptr, nullptr, dP, dF, dG, dmu2, dm0, dfm0, dsig_q1,
                                        dsig_q2, dsig_f, dsig_g, dsig0, dfsig0, ws, rs, stream, true);
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
