// k-step predictive distribution of a particle cloud -- see include/psvo_hip.h (psvo_particle_forecast) for the contract.  Per
// sequence b and origin t every particle is pushed through the transition K times,
//     x^(0)_n = X[t,b,:,n],   x^(k+1)_n = MLP_f(x^(k)_n) + sig_f (*) eps[k,t,b,:,n],
// and at every horizon k = 0..K the weighted cloud is read through the emission: mu_n = emission mean of x^(k)_n,
//     ymean = sum_n w_n mu_n,   yvar = sum_n w_n mu_n^2 - ymean^2 + v,   xmean = sum_n w_n x^(k)_n,
//     lpd   = logsumexp_n(log w_n + log g(obs[t+k,b] | x^(k)_n))         (0 where t + k >= T).
//
// Work decomposition (MI355X): origins are independent, so the grid is over (t, b) and the horizon loop runs in the kernel.  A
// lane is a particle; an origin takes ceil(N / 64) waves.  A workgroup holds one origin, or kFcOrigins of them when an origin
// is a single wave (N <= 64): the weights of MLP_f and MLP_g are staged in LDS once per workgroup, and one wave per workgroup
// would stage them for 64 particles only.  Nothing a wave computes depends on which workgroup it sits in.
// A horizon is: emission walk over the Dy outputs (wobs_common.h), each lane's terms reduced over the WAVE with the DPP scan
// and written by lane 63 into the wave's slot of a ping-pong LDS buffer -- 2 Dy + Dx sums and the (max, sum) pair of the
// log-sum-exp -- then ONE workgroup barrier, then the first wave of the origin folds the slots of the origin's waves in wave
// order (lane j owns output j; the log-sum-exp pairs are merged in the same order) and writes the outputs, while every wave
// goes on to the transition.  The slots of horizon k are rewritten at horizon k + 2, behind barrier k + 1, which their
// readers reach after reading; the observation row of horizon k + 1 is staged ahead of barrier k in the same way.
// No atomics; every sum is a wave scan or a fold over <= 8 waves in wave order: the output is the same bit for bit on every
// run, whatever PSVO_TUNE_DETERMINISTIC says.
//
// Exogenous inputs (IN: psvo_particle_forecast_input, on top of MS): the transition from horizon k to k + 1 of origin (t, b) takes
// the first-layer bias b1 + hb_f[t+k,b,:] where the others take b1 (b1 alone where t + k >= Tv: zero input).  The EFFECTIVE row is
// kept in a two-half LDS buffer hbuf[2][kFcOrigins][H], a row per origin of the workgroup: lane j < H of the origin's first wave
// requests word j of row k at the top of horizon k, beside the noise, and stores b1[j] + word (ONE fp32 add, as the filter's
// input form makes it; b1 from the LDS image) into half k & 1 next to stage_row(k + 1), ahead of barrier k.  The transition of
// horizon k reads that half behind barrier k (row_bias.h: RowBias, the operations of MlpLds::eval<true> in their order, so that
// hb_f = 0 gives the bits of the missing form).  The half is next written in horizon k + 2, behind barrier k + 1, which every
// reader of row k has reached after its transition; the other half, which horizon k - 1's transition may still be reading while
// row k is stored, is not touched.  So no barrier is added: a horizon stays ONE workgroup barrier.  (A row stored one horizon
// earlier -- row k + 1 ahead of barrier k -- would land in the half that the slower waves of the origin still read in the
// transition of horizon k - 1.)  A clamped dead origin of the last workgroup stages the row of origin T B - 1: in bounds.
#include "common.h"
#include "row_bias.h"
#include "wobs_common.h"

namespace psvo {

using wobs::kMaxDy;

constexpr int kFcOrigins = 4;                   // origins per workgroup when an origin is one wave
constexpr int kFcWaves = 8;                     // waves per workgroup, at most
constexpr int kFcSlot = 2 * kMaxDy + 8;         // floats per wave and horizon: S1[32] | S2[32] | Sx[4] | max, sum | pad

struct ForecastArgs {
    int B, T, N, Dy, K;
    int nwo, G;                                 // waves per origin, origins per workgroup (G > 1 only with nwo = 1)
    psvo_mlp f, g;
    const float *sig_f, *sig_g, *X, *logW, *obs, *eps;
    float *ymean, *yvar, *xmean, *lpd;
};

// the arguments of the input form: ForecastArgs field for field, so that what the kernel reads by name or by offset is found in
// either, then the input's.  A type of its own: the argument block of the other instantiations does not move
struct ForecastArgsIn {
    int B, T, N, Dy, K;
    int nwo, G;
    psvo_mlp f, g;
    const float *sig_f, *sig_g, *X, *logW, *obs, *eps;
    float *ymean, *yvar, *xmean, *lpd;
    const float* hb_f;                          // (Tv,B,H) the input's share of MLP_f's first layer
    int Tv;                                     // rows of hb_f, Tv >= T
};

// EMIS: psvo_desc.emission as a compile-time form, so that the Gaussian instantiations carry neither the softplus nor the fp64
// log-factorial of the count emission
// MS: the missing-observation form (psvo_particle_forecast_missing), compile-time too, so that the MS = false instantiations keep
// their code and registers.  A NaN in the target row is an entry that was not observed: y[e] is a broadcast, so y == y is the
// same in every lane and only feeds a select; the log-density adds the observed terms in the order e = 0 .. Dy - 1, each Gaussian
// term with its own constant c_e = -(log sig_g[e] + 1/2 log 2 pi) from one more LDS row (the filter's rule, filter_wobs_impl.h),
// and a target row with nothing observed gives lpd = 0 exactly.  ymean, yvar and xmean do not read obs.
// IN: the input form (above), compile-time as well: every line of it sits under `if constexpr (IN)`.
template <int DX, int H, int EMIS, bool MS, bool IN = false>
__global__ void __launch_bounds__(512) forecast_kernel(const std::conditional_t<IN, ForecastArgsIn, ForecastArgs> a) {
    using ForecastArgs = std::conditional_t<IN, ForecastArgsIn, psvo::ForecastArgs>;     // (what PSVO_ARG takes its offsets from)
    using MF = MlpLds<DX, H, DX, 1>;
    using MG = wobs::GLds<DX, H>;
    __shared__ __attribute__((aligned(16))) float wf[MF::kSize];
    __shared__ __attribute__((aligned(16))) float wg[MG::kSize];
    __shared__ float isg[kMaxDy];                               // 1 / sig_g
    __shared__ float ybuf[2][kFcOrigins][kMaxDy];               // observation rows of horizon k (k & 1) and k + 1
    __shared__ float lfbuf[2][kFcOrigins][kMaxDy];              // count emission: log Gamma(y + 1) of the rows in ybuf
    __shared__ float red[2][kFcWaves][kFcSlot];                 // per-wave partial sums of horizon k (k & 1)
    __shared__ float cg[kMaxDy];                                // MS, Gaussian forms: the constant of one term (else unused)
    __shared__ __attribute__((aligned(16))) float hbuf[IN ? 2 : 1][IN ? kFcOrigins : 1][IN ? H : 4];   // IN: bias rows of horizon k (k & 1), k - 1

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = blockDim.x;
    const int N = a.N, Dy = a.Dy, K = a.K;
    constexpr int emission = EMIS;
    // (sizes that only per-lane address arithmetic reads: opaque in a VGPR, as keep_in_vgpr does for floats -- the count
    //  instantiations otherwise run out of scalar registers beside the fp64 constants of the log-factorial)
    int B = a.B, T = a.T, nwo = a.nwo;
    asm volatile("" : "+v"(B));
    asm volatile("" : "+v"(T));
    asm volatile("" : "+v"(nwo));
    [[maybe_unused]] int Tv = 0;
    if constexpr (IN) {
        Tv = a.Tv;
        asm volatile("" : "+v"(Tv));
    }
    const int TB = T * B;
    const int og = wave / nwo, wo = wave - og * nwo;             // origin within the workgroup, wave within the origin
    const int o_raw = blockIdx.x * a.G + og;
    const bool live = o_raw < TB;                                // (the last workgroup may hold fewer than G origins)
    const int o = live ? o_raw : TB - 1;                         // clamp so that loads stay in bounds
    const int t = o / B, b = o - t * B;
    const int nl = wo * 64 + lane;
    const bool valid = nl < N;
    const int n = valid ? nl : N - 1;
    const float ninf = -__builtin_huge_valf();
    const bool first = wo == 0;                                  // the wave that stages the origin's rows and folds its slots
    // IN: the lanes that stage the bias row (opaque, as the sizes above: a mask held across the loop costs the count
    // instantiations a scalar pair they do not have)
    [[maybe_unused]] int stager = 0;
    if constexpr (IN) {
        stager = first && lane < H;
        asm volatile("" : "+v"(stager));
    }

    MF::load(wf, a.f, tid, NT);
    MG::load(wg, a.g, Dy, tid, NT);
    if (tid < Dy) isg[tid] = emission == 2 ? 0.f : 1.f / a.sig_g[tid];
    if constexpr (MS && EMIS != 2) {
        if (tid < Dy) cg[tid] = -(logf(a.sig_g[tid]) + kHalfLog2Pi);
    }
    // (the six pointers the horizon loop uses are re-read from the kernel arguments where they are used -- common.h: PSVO_ARG --
    //  held in scalar registers across the loop they do not fit beside the loop's own and hipcc spills them)
    const bool has_obs = a.obs != nullptr, has_eps = a.eps != nullptr, has_lpd = a.lpd != nullptr;
    auto stage_row = [&](int k) {       // observation row of horizon k, by the first Dy lanes of the origin
        if (has_obs && first && lane < Dy) {
            const int tk = t + k;
            const float y = tk < T ? PSVO_ARG(ForecastArgs, obs)[((size_t)tk * B + b) * Dy + lane] : 0.f;
            ybuf[k & 1][og][lane] = y;
            lfbuf[k & 1][og][lane] = emission == 2 ? wobs::log_factorial(y) : 0.f;
        }
    };
    stage_row(0);
    float lg = -Dy * kHalfLog2Pi;
    if constexpr (!MS) {    // (MS: the constant travels with each observed term)
        if (emission != 2) {
            for (int e = 0; e < Dy; ++e) lg -= logf(a.sig_g[e]);
        }
        keep_in_vgpr(lg);
    }
    // emission variance of output `lane` (the count emission takes the predictive mean itself)
    const float var0 = (emission == 0 && lane < Dy) ? a.sig_g[lane] * a.sig_g[lane] : 1.f;

    float x[DX], sf[DX];
#pragma unroll
    for (int d = 0; d < DX; ++d) {
        x[d] = a.X[((size_t)o * DX + d) * N + n];
        sf[d] = has_eps ? a.sig_f[d] : 0.f;
    }
    keep_in_vgpr(sf);

    // ---- w_n = softmax_n logW[t,b,:] (1 / N without logW): max and sum over the origin's waves, in wave order ----------------
    const float lw = valid ? (a.logW ? a.logW[(size_t)o * N + n] : 0.f) : ninf;
    const float wmx = wave_max(lw);
    if (lane == 0) red[1][wave][0] = wmx;
    __syncthreads();        // (weights, scales and the first observation row are visible behind this one too)
    float mx = red[1][og * nwo][0];
    for (int i = 1; i < nwo; ++i) mx = fmaxf(mx, red[1][og * nwo + i][0]);
    const float mb = (mx == ninf) ? 0.f : mx;
    const float wu = valid ? expf(lw - mb) : 0.f;
    const float wsum = wave_incl_scan(wu, lane);
    if (lane == 63) red[1][wave][1] = wsum;
    __syncthreads();
    float tot = 0.f;
    for (int i = 0; i < nwo; ++i) tot += red[1][og * nwo + i][1];
    const float wn = wu / tot;
    const float logwn = (lw - mb) - logf(tot);

    for (int k = 0; k <= K; ++k) {
        const bool more = k < K;
        float ek[DX];
#pragma unroll
        for (int d = 0; d < DX; ++d) ek[d] = 0.f;
        if (more && has_eps) {      // consumed behind the emission walk and the barrier
            const float* eps = PSVO_ARG(ForecastArgs, eps);
#pragma unroll
            for (int d = 0; d < DX; ++d) ek[d] = eps[(((size_t)k * TB + o) * DX + d) * N + n];
        }
        [[maybe_unused]] float hbk = 0.f;       // IN: word `lane` of hb_f[t+k,b,:], in flight during the emission walk
        if constexpr (IN) {
            if (more && stager && t + k < Tv)
                hbk = PSVO_ARG(ForecastArgs, hb_f)[((size_t)(t + k) * B + b) * H + lane];
        }
        float* slot = red[k & 1][wave];
        const float* y = ybuf[k & 1][og];
        const float* lf = lfbuf[k & 1][og];

        // ---- emission: Dy outputs in the order e = 0 .. Dy - 1 -----------------------------------------------------------
        [[maybe_unused]] int nobs = 0;      // MS: observed entries of the target row (the same number in every lane)
        {
            float h[H];
            MG::hidden(wg, x, h);
            float acc = 0.f;
#pragma unroll 1
            for (int e = 0; e < Dy; ++e) {
                const float r = MG::out(wg, e, h);
                const float mu = emission ? emis_mean(r) : r;
                const float wm = wn * mu;
                const float s1 = wave_incl_scan(wm, lane);
                const float s2 = wave_incl_scan(wm * mu, lane);
                if (lane == 63) {
                    slot[e] = s1;
                    slot[kMaxDy + e] = s2;
                }
                if (has_lpd) {
                    if constexpr (MS) {     // observed terms only, constant included; the same choice in every lane
                        const float ye = y[e];
                        float term;
                        if (emission == 2) {
                            term = wobs::count_term(ye, r) - lf[e];
                        } else {
                            const float z = (ye - mu) * isg[e];
                            term = fmaf(-0.5f * z, z, cg[e]);
                        }
                        const bool ob = (ye == ye);
                        acc += ob ? term : 0.f;
                        nobs += ob ? 1 : 0;
                    } else if (emission == 2) {
                        acc += wobs::count_term(y[e], r) - lf[e];
                    } else {
                        const float z = (y[e] - mu) * isg[e];
                        acc = fmaf(z, z, acc);
                    }
                }
            }
            if (has_lpd) {
                const float g_lp = (MS || emission == 2) ? acc : fmaf(-0.5f, acc, lg);
                const float v = valid ? logwn + g_lp : ninf;
                const float vm = wave_max(v);
                const float vb = (vm == ninf) ? 0.f : vm;
                const float ps = wave_incl_scan(expf(v - vb), lane);
                if (lane == 63) {
                    slot[2 * kMaxDy + 4] = vm;
                    slot[2 * kMaxDy + 5] = ps;
                }
            }
        }
#pragma unroll
        for (int d = 0; d < DX; ++d) {
            const float sx = wave_incl_scan(wn * x[d], lane);
            if (lane == 63) slot[2 * kMaxDy + d] = sx;
        }
        if (more) stage_row(k + 1);
        if constexpr (IN) {     // the bias row of THIS horizon's transition: read behind the barrier, its half rewritten at k + 2
            if (more && stager) {
                const float b1 = wf[MF::kB1 + lane];
                hbuf[k & 1][og][lane] = t + k < Tv ? b1 + hbk : b1;
            }
        }
        __syncthreads();

        // ---- fold the origin's slots in wave order: lane j of its first wave owns output j -------------------------------
        if (live && first) {
            const float* s0 = red[k & 1][og * nwo];
            const size_t ko = (size_t)k * TB + o;
            if (lane < Dy) {
                float m = 0.f, q = 0.f;
                for (int i = 0; i < nwo; ++i) {
                    m += s0[i * kFcSlot + lane];
                    q += s0[i * kFcSlot + kMaxDy + lane];
                }
                float* ymean = PSVO_ARG(ForecastArgs, ymean);
                float* yvar = PSVO_ARG(ForecastArgs, yvar);
                if (ymean) ymean[ko * Dy + lane] = m;
                if (yvar) yvar[ko * Dy + lane] = (q - m * m) + (emission == 2 ? m : var0);
            } else if (lane < Dy + DX) {
                const int d = lane - Dy;
                float m = 0.f;
                for (int i = 0; i < nwo; ++i) m += s0[i * kFcSlot + 2 * kMaxDy + d];
                float* xmean = PSVO_ARG(ForecastArgs, xmean);
                if (xmean) xmean[ko * DX + d] = m;
            } else if (lane == Dy + DX && has_lpd) {
                float out = 0.f;
                if (t + k < T && (!MS || nobs > 0)) {
                    float M = s0[2 * kMaxDy + 4];
                    for (int i = 1; i < nwo; ++i) M = fmaxf(M, s0[i * kFcSlot + 2 * kMaxDy + 4]);
                    const float Mb = (M == ninf) ? 0.f : M;
                    float S = 0.f;
                    for (int i = 0; i < nwo; ++i) {
                        const float mi = s0[i * kFcSlot + 2 * kMaxDy + 4];      // (-inf: a wave of weight zero, its sum is 0)
                        S += (mi == ninf) ? 0.f : s0[i * kFcSlot + 2 * kMaxDy + 5] * expf(mi - Mb);
                    }
                    out = Mb + logf(S);
                }
                PSVO_ARG(ForecastArgs, lpd)[ko] = out;
            }
        }

        // ---- transition -----------------------------------------------------------------------------------------------------
        if (more) {
            float fx[DX];
            if constexpr (IN) wobs::RowBias<DX, H>::eval(wf, hbuf[k & 1][og], x, fx);
            else MF::template eval<true>(wf, x, fx);
#pragma unroll
            for (int d = 0; d < DX; ++d) x[d] = fmaf(sf[d], ek[d], fx[d]);
        }
    }
}

template <int DX, int H, int EMIS, bool MS, bool IN = false, class Args = ForecastArgs>
static int launch_forecast(Args& a, hipStream_t stream) {
    const long long TB = (long long)a.T * a.B;
    a.nwo = (a.N + 63) >> 6;
    a.G = a.nwo == 1 ? kFcOrigins : 1;
    const int NT = 64 * a.nwo * a.G;
    const int blocks = (int)((TB + a.G - 1) / a.G);
    clear_hip_error();
    hipLaunchKernelGGL((forecast_kernel<DX, H, EMIS, MS, IN>), dim3(blocks), dim3(NT), 0, stream, a);
    return launch_status();
}

}  // namespace psvo

// the checks and the launch behind psvo_particle_forecast, psvo_particle_forecast_missing (ms) and psvo_particle_forecast_input
// (in, on top of ms: hb_f and Tv are checked with the other arguments, ahead of the envelope)
static int particle_forecast_checked(const psvo_desc* desc, int K, const psvo_mlp* f, const psvo_mlp* g, const float* sig_f,
                                     const float* sig_g, const float* X, const float* logW, const float* obs, const float* eps,
                                     float* ymean, float* yvar, float* xmean, float* lpd, void* stream, bool ms,
                                     bool in = false, const float* hb_f = nullptr, int Tv = 0) {
    using namespace psvo;
    if (!desc || !f || !g || !X) return PSVO_ERR_INVALID;
    if (!f->W1 || !f->b1 || !f->W2 || !f->b2 || !g->W1 || !g->b1 || !g->W2 || !g->b2) return PSVO_ERR_INVALID;
    if (!ymean && !yvar && !xmean && !lpd) return PSVO_ERR_INVALID;
    if (lpd && !obs) return PSVO_ERR_INVALID;
    if (eps && !sig_f) return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0 || K < 0) return PSVO_ERR_INVALID;
    if (in && (!hb_f || Tv < desc->T)) return PSVO_ERR_INVALID;
    if (!desc_layers_ok(desc) || desc->layers == 2) return PSVO_ERR_UNSUPPORTED;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!sig_g && desc->emission != 2) return PSVO_ERR_INVALID;
    if (desc->Dy < 1 || desc->Dy > wobs::kMaxDy || desc->N > 512) return PSVO_ERR_UNSUPPORTED;
    if ((long long)desc->T * desc->B > 0x7fffffffLL) return PSVO_ERR_UNSUPPORTED;

    ForecastArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy; a.K = K;
    a.nwo = a.G = 1;
    a.f = *f; a.g = *g;
    a.sig_f = sig_f; a.sig_g = sig_g; a.X = X; a.logW = logW; a.obs = obs; a.eps = eps;
    a.ymean = ymean; a.yvar = yvar; a.xmean = xmean; a.lpd = lpd;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (in) {
        ForecastArgsIn ai;
        ai.B = a.B; ai.T = a.T; ai.N = a.N; ai.Dy = a.Dy; ai.K = a.K;
        ai.nwo = ai.G = 1;
        ai.f = a.f; ai.g = a.g;
        ai.sig_f = sig_f; ai.sig_g = sig_g; ai.X = X; ai.logW = logW; ai.obs = obs; ai.eps = eps;
        ai.ymean = ymean; ai.yvar = yvar; ai.xmean = xmean; ai.lpd = lpd;
        ai.hb_f = hb_f; ai.Tv = Tv;
        return pick_dx(desc->Dx, [&](auto dx) {
            return pick_h(desc->H, [&](auto h) {
                return pick<0, 1, 2>(desc->emission, [&](auto em) {
                    return launch_forecast<dx(), h(), em(), true, true>(ai, s); }); }); });
    }
    return pick_dx(desc->Dx, [&](auto dx) {
        return pick_h(desc->H, [&](auto h) {
            return pick<0, 1, 2>(desc->emission, [&](auto em) {
                return ms ? launch_forecast<dx(), h(), em(), true>(a, s) : launch_forecast<dx(), h(), em(), false>(a, s); }); }); });
}

extern "C" int psvo_particle_forecast(const psvo_desc* desc, int K, const psvo_mlp* f, const psvo_mlp* g, const float* sig_f,
                                      const float* sig_g, const float* X, const float* logW, const float* obs, const float* eps,
                                      float* ymean, float* yvar, float* xmean, float* lpd, void* stream) {
    return particle_forecast_checked(desc, K, f, g, sig_f, sig_g, X, logW, obs, eps, ymean, yvar, xmean, lpd, stream, false);
}

extern "C" int psvo_particle_forecast_missing(const psvo_desc* desc, int K, const psvo_mlp* f, const psvo_mlp* g,
                                              const float* sig_f, const float* sig_g, const float* X, const float* logW,
                                              const float* obs, const float* eps, float* ymean, float* yvar, float* xmean,
                                              float* lpd, void* stream) {
    return particle_forecast_checked(desc, K, f, g, sig_f, sig_g, X, logW, obs, eps, ymean, yvar, xmean, lpd, stream, true);
}

extern "C" int psvo_particle_forecast_input(const psvo_desc* desc, int K, const psvo_mlp* f, const psvo_mlp* g,
                                            const float* sig_f, const float* sig_g, const float* X, const float* logW,
                                            const float* obs, const float* eps, float* ymean, float* yvar, float* xmean,
                                            float* lpd, const float* hb_f, int Tv, void* stream) {
    return particle_forecast_checked(desc, K, f, g, sig_f, sig_g, X, logW, obs, eps, ymean, yvar, xmean, lpd, stream, true, true,
                                     hb_f, Tv);
}
