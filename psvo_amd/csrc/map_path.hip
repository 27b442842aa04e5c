// MAP trajectory (particle Viterbi; Godsill, Doucet and West 2001) on the particle system a forward filter left in HBM -- see
// include/psvo_hip.h (psvo_map_path) for the contract.  Every particle of every step is a node of a T x N lattice; the path
// through it that maximises  log mu(x_0) + sum_t log f(x_t | x_{t-1}) + sum_t log g(y_t | x_t)  is found by the max-product
// recursion
//     d_0[j] = log N(X[0][j]; fm0, fsig0) + G_0[j],      d_t[j] = G_t[j] + max_k (delta[t-1][k] + l_{t-1}[j,k]),
// l the transition density of ffbs.hip, G_t[j] the emission log-density of particle j over the observed entries of step t.
//
// Work decomposition (MI355X): two launches, so that the serial chain over t carries only what depends on t - 1.
//   map_emission_kernel   G_t[j] for every (t, b) at once: a grid over (t, b), a lane per particle, MLP_g from its LDS image
//                         (wobs_common.h), the step's observation row staged once per workgroup.  Written into delta[t,b,j].
//                         H (Dx + Dy) multiply-adds per particle against N Dx in a pair pass: at wide Dy this is the larger
//                         part of the work, and it fills the machine where the recursion cannot.
//   map_viterbi_kernel    one persistent workgroup per sequence walks t upwards; lane = j.  A step stages delta[t-1][k] + cst
//                         and Fm[t-1][k] as LDS rows (as ffbs_kernel stages pass 1) and runs ONE N x N pair phase with a running
//                         (max, argmax) (ffbs_pair.h: pair_argmax) -- the smoother runs two with a log-sum-exp each.  Natural-log
//                         domain throughout: nothing is exponentiated, so the base-2 rescaling of ffbs.hip would buy nothing.
//                         Then G is added, the workgroup maximum taken (wave max, a fold over the <= 8 waves in wave order) and
//                         delta, lmax, bp written.  Two barriers per step: the staging one and the fold's.
//   backtrack             in the same kernel behind a workgroup barrier: the lowest index among the last step's maxima (a ballot
//                         per wave, the minimum over the waves), then one lane walks bp downwards -- T dependent reads -- and
//                         writes path and Xmap.
// Ties: every comparison is a strict `>` walking upwards, so the LOWEST index wins at every level (accumulator, merge of the
// two accumulators, wave, workgroup).  No atomics, no sum whose order could vary: the output is the same bit for bit on every
// run, whatever PSVO_TUNE_DETERMINISTIC says.  Every index written is one a loop counted or a clamped one: nothing is
// addressed with a value the data decided.
#include "common.h"
#include "ffbs_pair.h"
#include "wobs_common.h"

namespace psvo {

using wobs::kMaxDy;

constexpr int kMapOrigins = 4;      // (t, b) pairs per workgroup of the emission kernel where one is a single wave (N <= 64)

struct MapArgs {
    int B, T, N, Dy, emission;
    int nwo, G;                     // emission kernel: waves per (t, b), (t, b) pairs per workgroup (G > 1 only with nwo = 1)
    psvo_mlp g;
    const float *sig_f, *sig_g, *fm0, *fsig0, *obs, *X, *Fm;
    float *delta, *lmax;
    int32_t *bp, *path;
    float* Xmap;
};

// G_t[j] = sum over the observed entries e of obs[t,b,:] of term_e(X[t,b,:,j]), in the order e = 0 .. Dy - 1, terms and constants
// those of forecast_kernel<.., MS = true>: a NaN observation only feeds a select on a broadcast, and a row with nothing observed
// gives exactly 0.  CNT: the count emission (psvo_desc.emission = 2) as a compile-time form, so that the Gaussian instantiations
// carry neither its logarithm nor the fp64 log-factorial; emission 0 / 1 is a run-time select on the mean, as in the wide filters.
template <int DX, int H, bool CNT>
__global__ void __launch_bounds__(512) map_emission_kernel(const MapArgs a) {
    using MG = wobs::GLds<DX, H>;
    __shared__ __attribute__((aligned(16))) float wg[MG::kSize];
    __shared__ float isg[kMaxDy];                       // 1 / sig_g
    __shared__ float cg[kMaxDy];                        // the constant of one Gaussian term
    __shared__ float ybuf[kMapOrigins][kMaxDy];         // the observation rows of the workgroup's (t, b) pairs
    __shared__ float lfbuf[kMapOrigins][kMaxDy];        // CNT: log Gamma(y + 1) of the rows in ybuf

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = blockDim.x;
    const int N = a.N, Dy = a.Dy, nwo = a.nwo;
    const int TB = a.T * a.B;
    const int og = wave / nwo, wo = wave - og * nwo;    // pair within the workgroup, wave within the pair
    const int o_raw = blockIdx.x * a.G + og;
    const bool live = o_raw < TB;                       // (the last workgroup may hold fewer than G pairs)
    const int o = live ? o_raw : TB - 1;                // clamp so that loads stay in bounds
    const int nl = wo * 64 + lane;
    const bool valid = nl < N;
    const int n = valid ? nl : N - 1;
    const bool softplus_mean = a.emission != 0;

    MG::load(wg, a.g, Dy, tid, NT);
    if constexpr (!CNT) {
        if (tid < Dy) {
            const float s = a.sig_g[tid];
            isg[tid] = 1.f / s;
            cg[tid] = -(logf(s) + kHalfLog2Pi);
        }
    }
    if (wo == 0 && lane < Dy) {
        const float y = a.obs[(size_t)o * Dy + lane];
        ybuf[og][lane] = y;
        if constexpr (CNT) lfbuf[og][lane] = wobs::log_factorial(y);
    }
    float x[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) x[d] = a.X[((size_t)o * DX + d) * N + n];
    __syncthreads();

    const float* y = ybuf[og];
    float h[H];
    MG::hidden(wg, x, h);
    float acc = 0.f;
#pragma unroll 1
    for (int e = 0; e < Dy; ++e) {
        const float r = MG::out(wg, e, h);
        const float ye = y[e];
        float term;
        if constexpr (CNT) {
            term = wobs::count_term(ye, r) - lfbuf[og][e];
        } else {
            const float mu = softplus_mean ? emis_mean(r) : r;
            const float z = (ye - mu) * isg[e];
            term = fmaf(-0.5f * z, z, cg[e]);
        }
        acc += (ye == ye) ? term : 0.f;
    }
    if (live && valid) a.delta[(size_t)o * N + n] = acc;
}

template <int DX, int MAXT>
__global__ void __launch_bounds__(MAXT) map_viterbi_kernel(const MapArgs a) {
    constexpr int DXP = ffbs_dxp(DX);
    constexpr int NP = (DX + 1) / 2;
    constexpr float kRsqrt2 = 0.7071067811865476f;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = blockDim.x, nw = NT >> 6;
    const int b = blockIdx.x, B = a.B, T = a.T, N = a.N;
    const bool valid = tid < N;
    const int n = valid ? tid : N - 1;      // clamp so that loads stay in bounds
    const int n8 = (N + 7) & ~7;            // staged rows the pair loop walks (<= NT)
    const float ninf = -__builtin_huge_valf();

    float* sA = smem;                               // [NT]      rows: delta[t-1][k] + cst
    float* sm = sA + NT;                            // [NT][DXP] rows: Fm[t-1][k]
    float* red = sm + DXP * NT;                     // [8]       per-wave maxima of the step
    int* redi = reinterpret_cast<int*>(red + 8);    // [8]       per-wave lowest index among the last step's maxima

    // constant transition scale: l[j,k] = cst - sum_d ((x[j,d] - m[k,d]) r[d])^2,  r = 1 / (sqrt(2) s)
    float r[DX], cst = -DX * kHalfLog2Pi;
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        const float s = a.sig_f[d];
        r[d] = kRsqrt2 / s;
        cst -= logf(s);
    }
    f2 r2[NP];
    pack_row<DX>(r, r2);

    // rows of one step: X[t], G_t (which the emission kernel left in delta[t]) and Fm[t - 1].  No branch in here (ffbs.hip)
    auto load_rows = [&](int t, float (&x)[DX], float& g, float (&fm)[DX]) {
        const size_t tb = (size_t)t * B + b, tp = (size_t)max(t - 1, 0) * B + b;
        g = a.delta[tb * N + n];
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            x[d] = a.X[(tb * DX + d) * N + n];
            fm[d] = a.Fm[(tp * DX + d) * N + n];
        }
    };

    // d_t -> lmax[t], delta[t] = d_t - lmax[t], bp[t]; returns this lane's delta (-inf in the padding lanes)
    auto finish = [&](int t, float v, int arg) {
        const size_t tb = (size_t)t * B + b;
        const float vv = valid ? v : ninf;
        const float wm = wave_max(vv);
        if (lane == 0) red[wave] = wm;
        __syncthreads();
        float mx = red[0];
        for (int i = 1; i < nw; ++i) mx = fmaxf(mx, red[i]);
        const float mb = (mx == ninf) ? 0.f : mx;
        const float dl = vv - mb;
        if (valid) {
            a.delta[tb * N + n] = dl;
            a.bp[tb * N + n] = arg;
        }
        if (tid == 0) a.lmax[tb] = mx;
        return dl;
    };

    float x_c[DX], fm_c[DX], g_c;
    load_rows(0, x_c, g_c, fm_c);
    float x_n[DX], fm_n[DX], g_n;
    load_rows(min(1, T - 1), x_n, g_n, fm_n);      // prefetch: consumed one step later

    // ---- t = 0: the prior; every particle is its own predecessor ------------------------------------------------------------
    float dprev;
    {
        float q = 0.f, c0 = -DX * kHalfLog2Pi;
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float s0 = a.fsig0[d];
            const float z = (x_c[d] - a.fm0[(size_t)b * DX + d]) * (kRsqrt2 / s0);
            q = fmaf(z, z, q);
            c0 -= logf(s0);
        }
        dprev = finish(0, (c0 - q) + g_c, tid);
    }

    for (int t = 1; t < T; ++t) {
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            x_c[d] = x_n[d];
            fm_c[d] = fm_n[d];
        }
        g_c = g_n;
        load_rows(min(t + 1, T - 1), x_n, g_n, fm_n);      // (the last step reads its own rows again; nothing uses them)

        // ---- stage the rows of the pair phase (padding rows: -inf and zeros, so that their pair term stays -inf) -----------
        float row_m[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) row_m[d] = valid ? fm_c[d] : 0.f;
        lds_row_store<DX>(sm + tid * DXP, row_m);
        sA[tid] = valid ? dprev + cst : ninf;
        __syncthreads();
        // ---- pair phase: lane = j, rows k ------------------------------------------------------------------------------------
        f2 own2[NP];
        pack_row<DX>(x_c, own2);
        float best;
        int arg;
        pair_argmax<DX>(sA, sm, own2, r2, n8, best, arg);
        dprev = finish(t, g_c + best, arg);
    }

    // ---- backtrack ------------------------------------------------------------------------------------------------------------
    if (a.path == nullptr && a.Xmap == nullptr) return;
    const unsigned long long hits = __ballot(valid && dprev == 0.f);
    if (lane == 0) redi[wave] = hits ? wave * 64 + (__ffsll((long long)hits) - 1) : N;
    __syncthreads();        // (bp of every step is visible to the workgroup behind this one too)
    if (tid == 0) {
        int j = redi[0];
        for (int i = 1; i < nw; ++i) j = min(j, redi[i]);
        if (j >= N) j = 0;      // (no entry equal to 0: the inputs were not finite)
        for (int t = T - 1; t >= 0; --t) {
            const size_t tb = (size_t)t * B + b;
            const int jn = a.bp[tb * N + j];
            if (a.path) a.path[tb] = j;
            if (a.Xmap) {
#pragma unroll
                for (int d = 0; d < DX; ++d) a.Xmap[tb * DX + d] = a.X[(tb * DX + d) * N + j];
            }
            j = min(max(jn, 0), N - 1);
        }
    }
}

template <int DX, int H, bool CNT>
static int launch_map_emission(MapArgs& a, hipStream_t stream) {
    const long long TB = (long long)a.T * a.B;
    a.nwo = (a.N + 63) >> 6;
    a.G = a.nwo == 1 ? kMapOrigins : 1;
    const int NT = 64 * a.nwo * a.G;
    const int blocks = (int)((TB + a.G - 1) / a.G);
    clear_hip_error();
    hipLaunchKernelGGL((map_emission_kernel<DX, H, CNT>), dim3(blocks), dim3(NT), 0, stream, a);
    return launch_status();
}

template <int DX>
static int launch_map_viterbi(const MapArgs& a, hipStream_t stream) {
    constexpr int DXP = ffbs_dxp(DX);
    const int NT = (a.N + 63) & ~63;
    const size_t lds = sizeof(float) * ((size_t)(1 + DXP) * NT + 16);
    clear_hip_error();
    if (NT <= 256) hipLaunchKernelGGL((map_viterbi_kernel<DX, 256>), dim3(a.B), dim3(NT), lds, stream, a);
    else hipLaunchKernelGGL((map_viterbi_kernel<DX, 512>), dim3(a.B), dim3(NT), lds, stream, a);
    return launch_status();
}

}  // namespace psvo

extern "C" int psvo_map_path(const psvo_desc* desc, const psvo_mlp* g, const float* sig_f, const float* sig_g,
                             const float* fm0, const float* fsig0, const float* obs, const float* X, const float* Fm,
                             float* delta, float* lmax, int32_t* bp, int32_t* path, float* Xmap, void* stream) {
    using namespace psvo;
    if (!desc || !g || !sig_f || !fm0 || !fsig0 || !obs || !X || !Fm || !delta || !lmax || !bp) return PSVO_ERR_INVALID;
    if (!g->W1 || !g->b1 || !g->W2 || !g->b2) return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (!desc_layers_ok(desc) || desc->layers == 2) return PSVO_ERR_UNSUPPORTED;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!sig_g && desc->emission != 2) return PSVO_ERR_INVALID;
    if (desc->Dy < 1 || desc->Dy > wobs::kMaxDy || desc->N > 512) return PSVO_ERR_UNSUPPORTED;
    if (desc->Dx < 2 || desc->Dx > 4 || (desc->H != 16 && desc->H != 32 && desc->H != 64)) return PSVO_ERR_UNSUPPORTED;
    if ((long long)desc->T * desc->B > 0x7fffffffLL) return PSVO_ERR_UNSUPPORTED;

    MapArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy; a.emission = desc->emission;
    a.nwo = a.G = 1;
    a.g = *g;
    a.sig_f = sig_f; a.sig_g = sig_g; a.fm0 = fm0; a.fsig0 = fsig0; a.obs = obs; a.X = X; a.Fm = Fm;
    a.delta = delta; a.lmax = lmax; a.bp = bp; a.path = path; a.Xmap = Xmap;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // launch 1: G into delta, every (t, b) at once
    const int st = pick_dx(desc->Dx, [&](auto dx) {
        return pick_h(desc->H, [&](auto h) {
            return a.emission == 2 ? launch_map_emission<dx(), h(), true>(a, s) : launch_map_emission<dx(), h(), false>(a, s); }); });
    if (st != PSVO_OK) return st;
    // launch 2: the recursion and the backtrack, a workgroup per sequence
    return pick_dx(desc->Dx, [&](auto dx) { return launch_map_viterbi<dx()>(a, s); });
}
