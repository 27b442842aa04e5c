// What the units of the wide-observation filter kernels share (filter_wobs.hip, filter_wobs_in.hip, filter_wobs_inad.hip): the argument blocks of the
// two kernels of filter_wobs_impl.h, their LDS sizes, and the envelope and dispatch of the entry points.
#pragma once
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

// Adaptive resampling (psvo_filter_forward_wobs_adaptive / psvo_filter_backward_wobs_adaptive): the static arguments plus the
// ESS threshold, the teacher-forced decisions (or null) and the two (T,B) outputs; in the reverse pass the decisions rs (T,B).
// Types of their own, so that the static kernels keep their argument blocks.
struct FwdArgsAd : FwdArgs {
    float ess_frac;
    const int32_t* rs_in;
    int32_t* rs_out;
    float* ess_out;
};
struct BwdArgsAd : BwdArgs {
    const int32_t* rs;
};
template <bool AD>
using FwdArgsT = std::conditional_t<AD, FwdArgsAd, FwdArgs>;
template <bool AD>
using BwdArgsT = std::conditional_t<AD, BwdArgsAd, BwdArgs>;
// a decision word read through the constant address space (uniform address: a scalar load)
typedef const __attribute__((address_space(4))) int32_t rs_word_t;
// the decisions of the launch, re-read from the kernel arguments at their point of use (BwdArgsAd::rs sits behind the base)
__device__ __forceinline__ const int32_t* arg_rs() {
    return arg_ptr<const int32_t>((unsigned)(sizeof(BwdArgsAd) - sizeof(const int32_t*)));
}
static_assert(sizeof(BwdArgsAd) == sizeof(BwdArgs) + sizeof(const int32_t*), "rs is the last word of the adaptive arguments");

// Exogenous inputs (psvo_filter_forward_wobs_input / psvo_filter_backward_wobs_input, filter_wobs_in.hip): the static arguments
// plus the input's share of the hidden pre-activations of MLP_q1 / MLP_f, hb[t,b,:] = v[b,t,:] W1[Dx:] (T,B,H) each; hb_f is not
// read under bootstrap.  Types of their own, as for the adaptive pair.
struct FwdArgsIn : FwdArgs {
    const float *hb_q1, *hb_f;
};
struct BwdArgsIn : BwdArgs {
    const float *hb_q1, *hb_f;
};

// Both (psvo_filter_forward_wobs_input_adaptive / psvo_filter_backward_wobs_input_adaptive, filter_wobs_inad.hip): the adaptive
// blocks with the bias rows behind them, so that every field keeps the offset it has in FwdArgsAd / BwdArgsAd -- rs is still
// the last word of the BwdArgsAd part, where arg_rs() fetches it.  Types of their own once more.
struct FwdArgsInAd : FwdArgsAd {
    const float *hb_q1, *hb_f;
};
struct BwdArgsInAd : BwdArgsAd {
    const float *hb_q1, *hb_f;
};
static_assert(sizeof(BwdArgsInAd) == sizeof(BwdArgsAd) + 2 * sizeof(const float*), "the bias rows sit behind rs");

// (ms: the missing-observation form keeps one more row, the per-output constants, where the count form has its log-factorials)
template <int DX, int H>
static size_t fwd_lds_bytes(int NT, bool count, bool ms = false) {
    return sizeof(float) * (2 * MlpLds<DX, H, DX, 1>::kSize + GLds<DX, H>::kSize + 3 * kMaxDy + NT + 3 * DX * NT + 48 +
                            (count ? 2 * kMaxDy : ms ? kMaxDy : 0));
}

struct BwdOut {
    float *dsig_q1, *dsig_q2, *dsig_f, *dsig_g, *dsig0, *dfsig0;
};

template <int DX, int H>
static size_t bwd_lds_bytes(int NT, int Dy, bool bootstrap) {
    return sizeof(float) * (2 * MlpLds<DX, H, DX, 1>::kSize + GLds<DX, H>::kSize + 3 * kMaxDy + 16 + (size_t)NT
                            + (size_t)(bootstrap ? DX : 2 * DX) * NT + (size_t)Dy * NT + 10 * DX);
}

// the envelope of the two filter entry points (host only): 3 <= Dy <= 32, one hidden layer, N <= 512; Dx and H by dispatch
// (min_dy = 1: the missing-observation pair, which also serves the widths of the plain kernels)
static bool filter_shape_ok(const psvo_desc* d, int min_dy = 3) {
    return d->Dy >= min_dy && d->Dy <= kMaxDy && d->layers >= 0 && d->layers <= 1 && d->N <= 512 && d->B <= 65535;
}

template <class F>
static int dispatch_dx_h(int Dx, int H, F&& f) {
    return pick_dx(Dx, [&](auto dx) { return pick_h(H, [&](auto h) { return f(dx, h); }); });
}

}  // namespace wobs
}  // namespace psvo
