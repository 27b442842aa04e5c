// Exogenous inputs with adaptive resampling: the input-driven filter pair of filter_wobs_in.hip (the missing-observation form with a
// first-layer bias row per step, every 1 <= Dy <= 32 and emission form) resampling a sequence at step t only where its effective
// sample size has fallen below ess_frac N, or where rs_in says so (include/psvo_hip.h: psvo_filter_forward_wobs_input_adaptive,
// psvo_filter_backward_wobs_input_adaptive).  This unit is filter_wobs_impl.h compiled a sixth time, PSVO_IN = 1, PSVO_MS = 1 and
// PSVO_AD = 1: 18 forward and 18 reverse kernels (no EXT form: nothing runs behind an adaptive filter under autograd) and not one
// line of their own -- what the input form adds sits under `#if PSVO_IN` there, what the adaptive form adds under `#if PSVO_AD`,
// and the two sets do not touch (filter_wobs_impl.h says why).  The argument blocks are FwdArgsInAd / BwdArgsInAd
// (filter_wobs_args.h).  As for the input pair, the gradient of hb is psvo_mlp_wgrad_rowbias's business.
#include "filter_wobs_args.h"
#include "row_bias.h"

namespace psvo {
namespace wobs {

#define PSVO_AD 1
#define PSVO_MS 1
#define PSVO_IN 1
#include "filter_wobs_impl.h"
#undef PSVO_IN
#undef PSVO_MS
#undef PSVO_AD

// (the LDS of the input pair: the missing-observation form with both rows of the count form, plus hbuf[2][2 H])
template <int DX, int H>
static int launch_fwd_inad(const FwdArgsInAd& a, hipStream_t stream) {
    const int NT = (a.N + 63) & ~63;
    const size_t lds = fwd_lds_bytes<DX, H>(NT, true) + sizeof(float) * 4 * H;
    clear_hip_error();
    if (a.emission == 2) hipLaunchKernelGGL((filter_fwd_wobs_inad_kernel<DX, H, true>), dim3(a.B), dim3(NT), lds, stream, a);
    else hipLaunchKernelGGL((filter_fwd_wobs_inad_kernel<DX, H, false>), dim3(a.B), dim3(NT), lds, stream, a);
    return launch_status();
}

template <int DX, int H>
static int launch_bwd_inad(const BwdArgsInAd& a, const BwdOut& o, hipStream_t stream) {
    const int NT = (a.N + 63) & ~63;
    const size_t lds = bwd_lds_bytes<DX, H>(NT, a.Dy, a.bootstrap != 0) + sizeof(float) * 4 * H;
    clear_hip_error();
    if (a.emission == 2) hipLaunchKernelGGL((filter_bwd_wobs_inad_kernel<DX, H, false, true>), dim3(a.B), dim3(NT), lds, stream, a);
    else hipLaunchKernelGGL((filter_bwd_wobs_inad_kernel<DX, H, false, false>), dim3(a.B), dim3(NT), lds, stream, a);
    if (a.two_q) {
        launch_row_sum(a.dm2_rows, (long long)a.T * a.B * DX, a.N, a.dmu2, stream);
    }
    (void)launch_filter_bwd_finalize(DX, {a.sacc, a.B, a.Dy, a.two_q, a.bootstrap, a.sig_q1, a.sig_q2, a.sig0, (int)(a.fsig0 == a.sig0),
                                          o.dsig_q1, o.dsig_q2, o.dsig_f, o.dsig_g, o.dsig0, o.dfsig0}, stream);
    return launch_status();
}

}  // namespace wobs
}  // namespace psvo

extern "C" int psvo_filter_forward_wobs_input_adaptive(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1, const float* sig_q2,
    const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0, const float* fm0,
    const float* fsig0, const float* obs, const float* eps, const float* u, const int32_t* idx_in, float* X, float* Xanc,
    float* Fm, float* P1, float* logW, int32_t* idx_out, float* lse, float ess_frac, const int32_t* rs_in, int32_t* rs_out,
    float* ess_out, const float* hb_q1, const float* hb_f, void* stream) {
    using namespace psvo;
    using namespace psvo::wobs;
    // the adaptive contract first, as psvo_filter_forward_wobs_adaptive has it; then the input pair's checks and envelope
    if (!desc || !(ess_frac > 0.f) || !desc->resample || !rs_out || !ess_out) return PSVO_ERR_INVALID;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X || !Xanc || !Fm || !logW ||
        !idx_out || !lse || !hb_q1)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T < 2 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f || !hb_f)) return PSVO_ERR_INVALID;
    if (!u && !idx_in) return PSVO_ERR_INVALID;
    if (!filter_shape_ok(desc, 1)) return PSVO_ERR_UNSUPPORTED;

    FwdArgsInAd a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy;
    a.resample = desc->resample; a.two_q = desc->two_q; a.bootstrap = desc->bootstrap; a.emission = desc->emission;
    a.q1 = *q1; a.f = desc->bootstrap ? *q1 : *f; a.g = *g;
    a.sig_q1 = sig_q1; a.sig_q2 = sig_q2; a.sig_f = sig_f; a.sig_g = sig_g;
    a.mu2 = mu2; a.m0 = m0; a.sig0 = sig0; a.fm0 = fm0; a.fsig0 = fsig0;
    a.obs = obs; a.eps = eps; a.u = u; a.idx_in = idx_in;
    a.X = X; a.Xanc = Xanc; a.Fm = Fm; a.P1 = P1; a.logW = logW; a.idx_out = idx_out; a.lse = lse;
    a.ess_frac = ess_frac; a.rs_in = rs_in; a.rs_out = rs_out; a.ess_out = ess_out;
    a.hb_q1 = hb_q1; a.hb_f = desc->bootstrap ? hb_q1 : hb_f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_fwd_inad<dx(), h()>(a, s); });
}

extern "C" int psvo_filter_backward_wobs_input_adaptive(
    const psvo_desc* desc, const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g, const float* sig_q1,
    const float* sig_q2, const float* sig_f, const float* sig_g, const float* mu2, const float* m0, const float* sig0,
    const float* fm0, const float* fsig0, const float* obs, const float* eps, const float* X, const float* Fm,
    const float* P1, const float* logW, const float* lse, const int32_t* idx, const float* dlse, float* dP, float* dF,
    float* dG, float* dmu2, float* dm0, float* dfm0, float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g,
    float* dsig0, float* dfsig0, float* ws, const int32_t* rs, const float* hb_q1, const float* hb_f, void* stream) {
    using namespace psvo;
    using namespace psvo::wobs;
    // the adaptive contract first, as psvo_filter_backward_wobs_adaptive has it; then the input pair's checks and envelope
    if (!desc || !desc->resample || !rs) return PSVO_ERR_INVALID;
    if (!desc_emission_ok(desc, 2)) return PSVO_ERR_UNSUPPORTED;
    if (!q1 || !g || !sig_q1 || !sig_g || !m0 || !sig0 || !fm0 || !fsig0 || !obs || !eps || !X || !Fm || !logW || !lse || !dP ||
        !dG || !dm0 || !dfm0 || !dsig_q1 || !dsig_q2 || !dsig_f || !dsig_g || !dsig0 || !dfsig0 || !ws || !hb_q1)
        return PSVO_ERR_INVALID;
    if (desc->B <= 0 || desc->T < 2 || desc->N <= 0) return PSVO_ERR_INVALID;
    if (desc->two_q && (!mu2 || !sig_q2 || !dmu2)) return PSVO_ERR_INVALID;
    if (!desc->bootstrap && (!f || !sig_f || !P1 || !dF || !hb_f)) return PSVO_ERR_INVALID;
    if (!idx) return PSVO_ERR_INVALID;
    if (!filter_shape_ok(desc, 1)) return PSVO_ERR_UNSUPPORTED;

    BwdArgsInAd a;
    a.B = desc->B; a.T = desc->T; a.N = desc->N; a.Dy = desc->Dy;
    a.resample = desc->resample; a.two_q = desc->two_q; a.bootstrap = desc->bootstrap; a.emission = desc->emission;
    a.q1 = *q1; a.f = desc->bootstrap ? *q1 : *f; a.g = *g;
    a.sig_q1 = sig_q1; a.sig_q2 = sig_q2; a.sig_f = sig_f; a.sig_g = sig_g;
    a.mu2 = mu2; a.m0 = m0; a.sig0 = sig0; a.fm0 = fm0; a.fsig0 = fsig0; a.obs = obs; a.eps = eps;
    a.X = X; a.Fm = Fm; a.P1 = P1; a.logW = logW; a.lse = lse; a.idx = idx; a.dlse = dlse;
    a.nparts = 0; a.dFm_ext = nullptr; a.dlogW_ext = nullptr;
    a.dP = dP; a.dF = dF; a.dG = dG; a.dmu2 = dmu2; a.dm0 = dm0; a.dfm0 = dfm0;
    a.sacc = ws;
    a.dm2_rows = ws + (long long)desc->B * (10 * desc->Dx + desc->Dy);
    a.rs = rs;
    a.hb_q1 = hb_q1; a.hb_f = desc->bootstrap ? hb_q1 : hb_f;
    BwdOut o{dsig_q1, dsig_q2, dsig_f, dsig_g, dsig0, dfsig0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dispatch_dx_h(desc->Dx, desc->H, [&](auto dx, auto h) { return launch_bwd_inad<dx(), h()>(a, o, s); });
}
