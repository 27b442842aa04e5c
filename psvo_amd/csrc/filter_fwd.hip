// Forward particle filter: one persistent workgroup per sequence, time loop in-kernel.
// Restates SVO.SMC (reference src/SMC/SVO.py:60-180) -- see include/psvo_hip.h for the contract.
//
// Work decomposition (MI355X): lane = particle n, workgroup = sequence b.  Everything inside a
// step is per-lane except the log-sum-exp over particles and the multinomial draw, which are a
// wavefront shuffle reduction/scan plus one LDS hop across the <= 16 waves of the workgroup.
// MLP weights live in LDS and are read as wave-uniform float4 broadcasts.  In bootstrap mode the
// proposal mean of a resampled particle is MLP_f(X_t[a]) = Fm_t[a], so the transition MLP is
// evaluated once per pre-resampling particle and *gathered* together with the particle instead
// of being re-evaluated after the gather (halves the dependent MLP chain per step).
#include "common.h"

namespace psvo {
inline namespace PSVO_LNS {   // l1 / l2: hidden layers of the per-particle MLPs (common.h)
PSVO_TIMERS_DEFINE(filter_fwd)


struct FilterArgs {
    int B, T, N;
    int resample, two_q, bootstrap, emission;
    psvo_mlp q1, f, g;
    const float *sig_q1, *sig_q2, *sig_f, *sig_g;
    const float *mu2, *m0, *sig0, *fm0, *fsig0, *obs, *eps, *u;
    const int32_t* idx_in;
    float *X, *Xanc, *Fm, *P1, *logW;
    int32_t* idx_out;
    float* lse;
};

// Adaptive resampling (psvo_filter_forward_adaptive): the static arguments plus the ESS threshold, the teacher-forced decisions
// (or null) and the two (T,B) outputs.  A type of its own, so that the static kernels keep their argument block.
struct FilterArgsAd : FilterArgs {
    float ess_frac;
    const int32_t* rs_in;
    int32_t* rs_out;
    float* ess_out;
};
template <bool AD>
using FilterArgsT = std::conditional_t<AD, FilterArgsAd, FilterArgs>;


// the kernels (filter_fwd_impl.h): the static pair, then the adaptive pair
#define PSVO_AD 0
#include "filter_fwd_impl.h"
#undef PSVO_AD
#define PSVO_AD 1
#include "filter_fwd_impl.h"
#undef PSVO_AD

template <int DX, int DY, int H, bool AD = false>
static int launch_filter(const FilterArgsT<AD>& a, hipStream_t stream) {
    using MQ = MlpLds<DX, H, DX, PSVO_L>;
    using MG = MlpLds<DX, H, DY, PSVO_L>;
    // latency-bound regime (N <= 128: at most 512 lanes, 256 VGPRs each): four lanes per particle.  Only the
    // shapes that compile without scratch use it; the rest keep one lane per particle.
    // (two hidden layers: always -- a lane then walks H / 4 units of the H x H layer instead of all H, and this kernel is a
    //  latency chain of one workgroup per sequence: C* sizes at "64,64", filter_fwd 6.4 -> 2.0 ms)
    constexpr bool kLppOk = (H % 16 == 0) && (PSVO_L == 2 || (H <= 32 && DX <= 3) || H == 16);
    if constexpr (kLppOk) {
        if (a.N <= 128) {
            const int NT4 = (4 * a.N + 63) & ~63;
            const int NPT = NT4 / 4;
            const size_t lds4 = sizeof(float) * (2 * MQ::kSize + MG::kSize + NPT + 16 + 3 * DX * NPT + (AD ? 48 : 32));
            clear_hip_error();
            if constexpr (AD)
                hipLaunchKernelGGL((filter_fwd_lpp_ad_kernel<DX, DY, H, 512>), dim3(a.B), dim3(NT4), lds4, stream, a);
            else
                hipLaunchKernelGGL((filter_fwd_lpp_kernel<DX, DY, H, 512>), dim3(a.B), dim3(NT4), lds4, stream, a);
            return launch_status();
        }
    }
    const int NT = (a.N + 63) & ~63;
    const size_t lds = sizeof(float) * (2 * MQ::kSize + MG::kSize + NT + 3 * DX * NT + 48);
    clear_hip_error();
    // the register budget follows the workgroup size: <= 256 threads is one wave per SIMD, so
    // the compiler may keep every MLP weight resident in VGPRs
    if constexpr (AD) {
        if (NT <= 256 && a.emission)
            hipLaunchKernelGGL((filter_fwd_ad_kernel<DX, DY, H, 256, 1>), dim3(a.B), dim3(NT), lds, stream, a);
        else if (NT <= 256)
            hipLaunchKernelGGL((filter_fwd_ad_kernel<DX, DY, H, 256, 0>), dim3(a.B), dim3(NT), lds, stream, a);
        else
            hipLaunchKernelGGL((filter_fwd_ad_kernel<DX, DY, H, 512>), dim3(a.B), dim3(NT), lds, stream, a);
    } else {
    if (NT <= 256 && a.emission)
        hipLaunchKernelGGL((filter_fwd_kernel<DX, DY, H, 256, 1>), dim3(a.B), dim3(NT), lds, stream, a);
    else if (NT <= 256)
        hipLaunchKernelGGL((filter_fwd_kernel<DX, DY, H, 256, 0>), dim3(a.B), dim3(NT), lds, stream, a);
    else
        hipLaunchKernelGGL((filter_fwd_kernel<DX, DY, H, 512>), dim3(a.B), dim3(NT), lds, stream, a);
    }
    return launch_status();
}

}  // inline namespace PSVO_LNS
}  // namespace psvo

namespace psvo {
inline namespace PSVO_LNS {
// the checks and the launch behind psvo_filter_forward (ad == nullptr) and psvo_filter_forward_adaptive
static int filter_forward_checked(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                  const float* sig_q1, const float* sig_q2, const float* sig_f,
                                  const float* sig_g, const float* mu2, const float* m0, const float* sig0,
                                  const float* fm0, const float* fsig0, const float* obs, const float* eps,
                                  const float* u, const int32_t* idx_in, float* X, float* Xanc, float* Fm, float* P1,
                                  float* logW, int32_t* idx_out, float* lse, const FilterArgsAd* ad, void* stream) {
    if (!mlp_layers_ok(q1) || !mlp_layers_ok(f) || !mlp_layers_ok(g)) return PSVO_ERR_INVALID;
    if (!desc || !q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X ||
        !Xanc || !Fm || !logW || !idx_out || !lse)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f)) return PSVO_ERR_INVALID;
    if (desc->resample && !u && !idx_in) return PSVO_ERR_INVALID;
    if (desc->N > 512) return PSVO_ERR_UNSUPPORTED;

    FilterArgs a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N;
    a.resample = desc->resample; a.two_q = desc->two_q; a.bootstrap = desc->bootstrap; a.emission = desc->emission;
    a.q1 = *q1; a.f = desc->bootstrap ? *q1 : *f; a.g = *g;
    a.sig_q1 = sig_q1; a.sig_q2 = sig_q2; a.sig_f = sig_f; a.sig_g = sig_g;
    a.mu2 = mu2; a.m0 = m0; a.sig0 = sig0; a.fm0 = fm0; a.fsig0 = fsig0;
    a.obs = obs; a.eps = eps; a.u = u; a.idx_in = idx_in;
    a.X = X; a.Xanc = Xanc; a.Fm = Fm; a.P1 = P1; a.logW = logW; a.idx_out = idx_out; a.lse = lse;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ad) {
        FilterArgsAd aa;
        static_cast<FilterArgs&>(aa) = a;
        aa.ess_frac = ad->ess_frac; aa.rs_in = ad->rs_in; aa.rs_out = ad->rs_out; aa.ess_out = ad->ess_out;
        return dispatch_shape(desc->Dx, desc->Dy, desc->H, [&](auto dx, auto dy, auto h) {
            return launch_filter<dx(), dy(), h(), true>(aa, s); });
    }
    return dispatch_shape(desc->Dx, desc->Dy, desc->H, [&](auto dx, auto dy, auto h) {
        return launch_filter<dx(), dy(), h()>(a, s); });
}
}  // inline namespace PSVO_LNS
}  // namespace psvo

PSVO_L2_DECL(psvo_filter_forward)
PSVO_ENTRY(psvo_filter_forward)(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                   const float* sig_q1, const float* sig_q2, const float* sig_f,
                                   const float* sig_g, const float* mu2, const float* m0, const float* sig0,
                                   const float* fm0, const float* fsig0, const float* obs, const float* eps,
                                   const float* u, const int32_t* idx_in, float* X, float* Xanc, float* Fm, float* P1,
                                   float* logW, int32_t* idx_out, float* lse, void* stream) {
    using namespace psvo;
    if (!desc_layers_ok(desc) || !desc_emission_ok(desc)) return PSVO_ERR_UNSUPPORTED;
#if PSVO_L == 1
    if (desc && desc->layers == 2)
        return psvo_filter_forward_l2(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs,
            eps, u, idx_in, X, Xanc, Fm, P1, logW, idx_out, lse, stream);
#endif
    return filter_forward_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, u,
                                  idx_in, X, Xanc, Fm, P1, logW, idx_out, lse, nullptr, stream);
}

PSVO_L2_DECL(psvo_filter_forward_adaptive)
PSVO_ENTRY(psvo_filter_forward_adaptive)(const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                   const float* sig_q1, const float* sig_q2, const float* sig_f,
                                   const float* sig_g, const float* mu2, const float* m0, const float* sig0,
                                   const float* fm0, const float* fsig0, const float* obs, const float* eps,
                                   const float* u, const int32_t* idx_in, float* X, float* Xanc, float* Fm, float* P1,
                                   float* logW, int32_t* idx_out, float* lse, float ess_frac, const int32_t* rs_in,
                                   int32_t* rs_out, float* ess_out, void* stream) {
    using namespace psvo;
    // the adaptive contract first: a threshold (NaN is none), a filter that resamples at all, somewhere to record the decisions
    if (!desc || !(ess_frac > 0.f) || !desc->resample || !rs_out || !ess_out) return PSVO_ERR_INVALID;
    if (!desc_layers_ok(desc) || !desc_emission_ok(desc)) return PSVO_ERR_UNSUPPORTED;
#if PSVO_L == 1
    if (desc->layers == 2)
        return psvo_filter_forward_adaptive_l2(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs,
            eps, u, idx_in, X, Xanc, Fm, P1, logW, idx_out, lse, ess_frac, rs_in, rs_out, ess_out, stream);
#endif
    FilterArgsAd ad;
    ad.ess_frac = ess_frac; ad.rs_in = rs_in; ad.rs_out = rs_out; ad.ess_out = ess_out;
    return filter_forward_checked(desc, q1, f, g, sig_q1, sig_q2, sig_f, sig_g, mu2, m0, sig0, fm0, fsig0, obs, eps, u,
                                  idx_in, X, Xanc, Fm, P1, logW, idx_out, lse, &ad, stream);
}
