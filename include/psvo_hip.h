/*
 * psvo_hip.h -- C ABI of the MI355X-native PSVO hot path (libpsvo_hip.so).
 *
 * The reference (amoretti86/PSVO) has no FFI/plugin registry: the hot path sits behind a
 * Python object protocol (`Obj(model, FLAGS).get_log_ZSMC(obs, hidden)`, reference
 * src/trainer.py:108, src/runner.py:70-79).  This header is the boundary a maintainer would
 * bind from that protocol; each entry point names the reference code it replaces.
 * INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless it says "host"; float = fp32, indices int32;
 *   - the caller allocates every input, output and workspace buffer; the library never
 *     allocates device memory and keeps no pointer after a call returns;
 *   - every entry point is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return value: 0 = ok, <0 = psvo_status error (see psvo_status_string);
 *   - HBM layout is particle-minor SoA so that a wavefront's lanes (particles) are contiguous:
 *         particles  X[t][b][d][n]      -> (T, B, Dx, N)
 *         weights    logW[t][b][n]      -> (T, B, N)
 *         per-seq    lse[t][b]          -> (T, B)
 *         features   mu2[t][b][d]       -> (T, B, Dx),  obs[t][b][e] -> (T, B, Dy)
 *         bsim noise eps_b[t][b][d][n][m] -> (T, B, Dx, N, M)
 *     (the reference's own internal layout is (T, N, B, D), src/SMC/SVO.py:176-178; the
 *     host mirror permutes to the reference's (B, T, N, Dx) at the Python boundary).
 *   - per-particle MLPs have ONE hidden layer of width H (reference default `*_layers=[32]`,
 *     src/runner_flag.py:53-57) or TWO of the same width (`*_layers=[64, 64]`, the example the reference's flag
 *     file gives, src/runner_flag.py:50-52; psvo_desc.layers = 2); kernels are instantiated for Dx in {2,3,4},
 *     Dy in {1,2} (3 .. 32 for the filter alone: the *_wobs entry points), H in {16,32,64} (two layers: {32,64}),
 *     M in {4,8,16,32}; N <= 512 (filter, PSVOwR reverse
 *     pass), N <= 1024 (backward simulation); any T, B <= 65535.  Anything else returns PSVO_ERR_UNSUPPORTED
 *     (never a silent fallback).
 */
#ifndef PSVO_HIP_H
#define PSVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSVO_ABI_VERSION 6

typedef enum {
    PSVO_OK = 0,
    PSVO_ERR_INVALID = -1,      /* null pointer / non-positive size / inconsistent desc       */
    PSVO_ERR_UNSUPPORTED = -2,  /* (Dx, Dy, H, M, N) outside the instantiated kernel set      */
    PSVO_ERR_HIP = -3           /* a HIP runtime call failed (launch error)                   */
} psvo_status;

/* Problem descriptor.  Mirrors the reference FLAGS that shape the path
 * (src/runner_flag.py:22-28,88-113; read at src/SMC/SVO.py:7-29, src/SMC/PSVO.py:9-19). */
typedef struct {
    int32_t B;          /* sequences in this call (FLAGS.batch_size, local shard)              */
    int32_t T;          /* time steps (FLAGS.time)                                             */
    int32_t N;          /* FLAGS.n_particles                                                   */
    int32_t M;          /* FLAGS.n_particles_for_BSim_proposal (bsim only)                     */
    int32_t Dx;         /* FLAGS.Dx                                                            */
    int32_t Dy;         /* FLAGS.Dy                                                            */
    int32_t H;          /* hidden width of ALL per-particle MLPs of the call (q1 / f / g / q1_inv): 16, 32 or
                           64.  Narrower or unequal widths (q1_layers=24, g_layers=16): the caller pads W1
                           columns, b1 and W2 rows with zeros up to H -- a padded unit contributes exactly 0 --
                           and drops the padded entries of the gradients (psvo_amd/SMC/SVO.py:_mlp_params)   */
    int32_t resample;   /* 1: multinomial resampling every step (SVO/AESMC/PSVO); 0: IWAE      */
    int32_t two_q;      /* FLAGS.use_2_q                                                       */
    int32_t bootstrap;  /* FLAGS.use_bootstrap (f shares q1's MLP and sigma)                   */
    int32_t emission;   /* 0: g = N(MLP_g(x), sig_g) (tf_mvn).  1: FLAGS.poisson_emission -- the
                           reference's tf_poisson (src/distribution/poisson.py:27-50) is a UNIT-scale
                           normal whose mean is softplus(MLP_g(x)) + 1e-6: pass sig_g = ones; the
                           dsig_g output is then meaningless.
                           2: the count emission, a Poisson law per output -- wide-observation entry
                           points only (see "Count emission" below); sig_g as for 1.
                           Any other value: PSVO_ERR_UNSUPPORTED from every entry point that reads the
                           field, ahead of its pointer checks ({0, 1} outside the wide entry points)  */
    int32_t layers;     /* hidden layers of ALL per-particle MLPs of the call: 0 or 1 = one (psvo_mlp.Wh / bh
                           ignored), 2 = two layers of width H each (FLAGS.q1_layers="64,64" ...,
                           src/transformation/MLP.py:24-38,50-54).  An MLP with fewer layers than the others
                           cannot be padded (an extra relu layer is not the identity): UNSUPPORTED upstream */
} psvo_desc;

/* Per-particle MLP, keras Dense layout (reference src/transformation/MLP.py:27-46):
 * hidden_0: W1 (Din, H) row-major, b1 (H); mu_layer: W2 (H, Dout) row-major, b2 (Dout);
 * with psvo_desc.layers == 2 also hidden_1 between them: Wh (H, H) row-major, bh (H)
 *     mu = relu(relu(x W1 + b1) Wh + bh) W2 + b2;
 * Wh / bh are NULL (ignored) for one hidden layer. */
typedef struct {
    const float* W1;
    const float* b1;
    const float* W2;
    const float* b2;
    const float* Wh;
    const float* bh;
} psvo_mlp;

int psvo_abi_version(void);
const char* psvo_status_string(int status);
/* Tuning switches (process-wide; for A/B measurements and tests -- results are the same to rounding under every value):
 *   PSVO_TUNE_BSIM_BWD: which reverse backward-simulation kernel psvo_bsim_backward launches.
 *     -1 default (measured best), 0 = lane = (chain, half, m) with per-j butterflies, 1 = "j on lanes" layout with the per-j
 *     sums on the VALU, 2 = the same with the per-j sums on v_mfma_f32_16x16x4_f32, 3 = the same as 1 with the pair exponents
 *     on v_mfma_f32_16x16x4_f32 (Dx = 2; otherwise as 1), 4 = the same as 3 on v_mfma_f32_16x16x32_bf16 with every f32
 *     operand split into three bf16 pieces (Dx = 2; otherwise as 1).  It changes psvo_bsim_blocks():
 *     set it before sizing workspaces. */
#define PSVO_TUNE_BSIM_BWD 1
/*   PSVO_TUNE_ROWS_BWD: rows per workgroup of psvo_rows_mlp_backward: 0 = chosen by the number of rows (default), 16, 64.
 *     It changes psvo_rows_mlp_blocks(): set it before sizing workspaces. */
#define PSVO_TUNE_ROWS_BWD 2
/*   PSVO_TUNE_L2_SPLIT: two-hidden-layer builds of psvo_bsim_forward / _backward: 0 (default) one lane per (chain, m);
 *   1 = a chain spread over 2 M lanes for small problems, as the one-layer builds do.  Set before sizing buffers. */
#define PSVO_TUNE_L2_SPLIT 3
/*   PSVO_TUNE_WGRAD2: psvo_mlp2_wgrad's H x H products: 0 (default) = v_mfma_f32_16x16x4_f32; 2 / 3 = bf16 matrix
 *   instructions with every f32 operand split into two / three bf16 pieces (products carried to 2^-17 / 2^-24 relative). */
#define PSVO_TUNE_WGRAD2 5
/*   PSVO_TUNE_FILTER_BWD: psvo_filter_backward in the bootstrap wiring with resampling (one hidden layer): 1 (default) = the
 *   affine scan (coefficients of every step in parallel, one or four waves per sequence for the recurrence, rows in
 *   parallel) where it pays -- no upstream gradient from a backward simulation, or N > 256 --, 2 = the scan wherever it
 *   applies, 0 = the persistent reverse kernel (one workgroup per sequence), which every other wiring uses. */
#define PSVO_TUNE_FILTER_BWD 6
/*   PSVO_TUNE_SKEW: start-up phase offset between the workgroups that share a CU in the backward-simulation kernels, in
 *   per cent of the kernel's estimate of its pair-phase length (default 0 = all workgroups start together: measured, it
 *   changes nothing -- profiles/r03_bsim_bwd_C5_ab.md -- and is kept as an A/B knob). */
#define PSVO_TUNE_SKEW 4
/*   PSVO_TUNE_DETERMINISTIC: 0 (default) = the kernels as measured; 1 = fixed-order sums on the reverse paths, so that two runs
 *   of the same inputs give bit-identical outputs.  Like every key it is process-global and takes effect when an operation is
 *   LAUNCHED (or captured into a hipGraph: a replay runs the kernels chosen at capture time).  Under 1, psvo_filter_backward and
 *   psvo_filter_backward_cov run the persistent reverse filter with fixed-order scatter copies where the default adds with float
 *   atomics in arrival order (N > 256; the cov filter at N > 64); every other route they take already sums in a fixed order.
 *   The backward simulations with state-dependent scales need a workspace under 1: psvo_bsim_backward_cov_ws /
 *   psvo_bsimwr_backward_cov_ws with det_ws = psvo_bsim_cov_det_ws_floats(B, N, M, Dx, Dy) floats (per-workgroup slices of
 *   every cross-workgroup sum, folded in workgroup order after each step: one launch per step in both modes); without it
 *   (det_ws NULL, or the entry points without _ws) they return PSVO_ERR_INVALID under 1.  With 0, det_ws is ignored.
 *   Values other than 0 and 1: PSVO_ERR_INVALID. */
#define PSVO_TUNE_DETERMINISTIC 8
int psvo_set_tuning(int key, int value);          /* PSVO_OK or PSVO_ERR_INVALID */
int psvo_get_tuning(int key);

/* hipGetErrorString of the most recent failed launch on the calling thread (PSVO_ERR_HIP). */
const char* psvo_last_hip_error(void);

/* ---------------------------------------------------------------------------------------------
 * Forward particle filter.  Replaces SVO.SMC (reference src/SMC/SVO.py:60-180) including
 * sample_from_2_dist (:182-232, diagonal branch), resample_X / get_resample_idx (:243-300)
 * and the per-step reduce_logsumexp of compute_log_ZSMC (:302-311).
 *
 * One persistent workgroup per sequence loops over t in-kernel.
 *
 *  q1, f, g       per-particle MLPs; when desc->bootstrap != 0, `f` is ignored (f == q1).
 *  sig_q1/sig_q2/sig_f (Dx), sig_g (Dy)  already-clipped scales max(softplus(raw), min)
 *                 (src/distribution/mvn.py:80-90); sig_q2 ignored when !two_q;
 *                 sig_f ignored when bootstrap.
 *  mu2  (T,B,Dx)  hoisted MLP_q2(e_t[b]) (proposal term that does not depend on particles);
 *                 ignored when !two_q.
 *  m0   (B,Dx), sig0 (Dx)   t=0 proposal term: MLP_q0(X0 feature), sigma_q0 (SVO.py:80-88).
 *  fm0  (B,Dx), fsig0 (Dx)  t=0 transition term: equal to (m0, sig0) when bootstrap&&two_q,
 *                 else (MLP_f(X0 feature), sigma_f) (SVO.py:91-92).
 *  obs  (T,B,Dy)
 *  eps  (T,B,Dx,N) standard-normal draws (injected; the reference draws them with mvn.sample)
 *  u    (T,B,N)   uniforms in [0,1) for the multinomial draw; used when idx_in == NULL
 *  idx_in (T,B,N) int32 teacher-forced ancestor indices or NULL
 *
 *  outputs: X (T,B,Dx,N) pre-resampling particles (Xs_ta), Xanc (T,B,Dx,N) resampled particles
 *  (X_ancestors_ta), Fm (T,B,Dx,N) = MLP_f(X_t) (transition means of every forward particle,
 *  consumed by the backward simulation), P1 (T,B,Dx,N) = MLP_q1(X_t) (optional, may be NULL; only
 *  needed by psvo_filter_backward when !bootstrap), logW (T,B,N) (log_Ws_ta), idx_out (T,B,N)
 *  ancestors, lse (T,B) = logsumexp_n logW[t,b,:].
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_forward(const psvo_desc* desc,
                        const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                        const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                        const float* mu2,
                        const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                        const float* obs, const float* eps, const float* u, const int32_t* idx_in,
                        float* X, float* Xanc, float* Fm, float* P1, float* logW, int32_t* idx_out,
                        float* lse, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Forward particle filter with STATE-DEPENDENT diagonal scales: FLAGS.output_cov and FLAGS.diag_cov
 * (reference src/runner_flag.py:67-70,221-222).  Every MLP then has a second output head (`sigma_layer`,
 * src/transformation/MLP.py:40-46) and every distribution's scale is
 *     sigma(input) = sigma_con + 0.1 * (exp(hidden(input) W_sigma + b_sigma) + 1e-6)
 * (MLP.py:58-61, src/distribution/mvn.py:66-71; sigma_con = the state-independent vector of get_sigma, mvn.py:80-90).
 * Same loop and outputs as psvo_filter_forward (SVO.SMC, src/SMC/SVO.py:60-180); differences:
 *  q1, f, g        W2 = [mu_layer | sigma_layer] (H, 2 Dout) row-major, b2 = [b_mu | b_sigma] (2 Dout); one hidden
 *                  layer (desc->layers <= 1; two layers: PSVO_ERR_UNSUPPORTED).  desc->emission = 1: the reference's
 *                  tf_poisson drops MLP_g's covariance head (src/distribution/poisson.py:33) -- unit scale, sigc_g unused
 *  sigc_q1/sigc_f (Dx), sigc_g (Dy)   the sigma_con parts (already clipped); sigc_f ignored when bootstrap
 *  mu2, sig2 (T,B,Dx)   hoisted q2 mean AND scale per step and sequence; ignored when !two_q
 *  m0, sig0, fm0, fsig0 (B,Dx)   t = 0 proposal / transition mean and scale per sequence (SVO.py:80-92)
 *  outputs         as psvo_filter_forward, plus Fs (T,B,Dx,N) = the scale of f given X_t (beside its mean Fm) and
 *                  P1s (T,B,Dx,N) beside P1 (both required when !bootstrap, ignored otherwise).
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_forward_cov(const psvo_desc* desc,
                            const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                            const float* sigc_q1, const float* sigc_f, const float* sigc_g,
                            const float* mu2, const float* sig2,
                            const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                            const float* obs, const float* eps, const float* u, const int32_t* idx_in,
                            float* X, float* Xanc, float* Fm, float* Fs, float* P1, float* P1s, float* logW,
                            int32_t* idx_out, float* lse, void* stream);

/* Reverse mode of psvo_filter_forward_cov (TensorFlow autodiff of the loop in the reference, src/trainer.py:115-118).
 *  inputs  : the forward call's inputs and outputs; upstream gradients dlse (T,B), dFm_ext / dFs_ext (T,B,Dx,N),
 *            dlogW_ext (T,B,N), each optional (NULL = zero).
 *  outputs : rows for psvo_mlp_wgrad, one pair per MLP -- w.r.t. the mu_layer output and w.r.t. the RAW sigma_layer
 *            output (d sigma / d raw = 0.1 exp(raw) already applied): dP / dPs (T,B,Dx,N) for MLP_q1 (which is also f
 *            when bootstrap), dF / dFs for MLP_f (!bootstrap), dG / dGs (T,B,Dy,N) for MLP_g;
 *            dmu2, dsig2 (T,B,Dx); dm0, dsig0, dfm0, dfsig0 (B,Dx) (written separately even when the caller passed the
 *            same buffer as m0 and fm0: add them); dsigc_q1 / dsigc_f (Dx), dsigc_g (Dy) = d loss / d sigma_con.
 *  ws      : workspace, psvo_filter_cov_ws_floats(B, T, N, Dx, Dy) floats, 16-byte aligned. */
long long psvo_filter_cov_ws_floats(int B, int T, int N, int Dx, int Dy);
int psvo_filter_backward_cov(const psvo_desc* desc,
                             const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                             const float* sigc_q1, const float* sigc_f, const float* sigc_g,
                             const float* mu2, const float* sig2,
                             const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                             const float* obs, const float* eps,
                             const float* X, const float* Fm, const float* Fs, const float* P1, const float* P1s,
                             const float* logW, const float* lse, const int32_t* idx,
                             const float* dlse, const float* dFm_ext, const float* dFs_ext, const float* dlogW_ext,
                             float* dP, float* dPs, float* dF, float* dFs, float* dG, float* dGs,
                             float* dmu2, float* dsig2,
                             float* dm0, float* dsig0, float* dfm0, float* dfsig0,
                             float* dsigc_q1, float* dsigc_f, float* dsigc_g,
                             float* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Marginal particle smoother: forward filtering, backward smoothing (FFBS) on the particle system a forward filter left in
 * HBM.  Restates FFBS_reweight_log_Ws of the reference's unused sweep code (not_used/SMC_supreme/SMC.py:451-482, with
 * smoothing_perc = 1 and normalised inputs) and its resampling of X_prevs by the reweighted weights (:87-94); the flags FFBS /
 * FFBS_to_learn are carried by auto_sh.py:94-97.  Added within ABI 6: purely additive, no existing struct or signature changed.
 *
 * Per sequence b, with a_t[k] = logW[t,b,k] - logsumexp_k logW[t,b,:] and the transition density
 *     l_t[j,k] = log N(X[t+1,b,:,j]; Fm[t,b,:,k], s_t[:,k]),   diagonal, on SCALES, the -sum_d log s_t[d,k] term included,
 *     s_t[:,k] = sig_f[:] (constant) or Fs[t,b,:,k] (per particle):
 *     S[T-1][k] = a_{T-1}[k]
 *     for t = T-2 .. 0:   den[j]  = logsumexp_k (a_t[k] + l_t[j,k])
 *                         S[t][k] = a_t[k] + logsumexp_j (S[t+1][j] - den[j] + l_t[j,k])
 * X[t+1] and Fm[t] are both pre-resampling histories, the pair the backward simulation's N x N term uses (PSVO.py:128-133).
 * S[t] is renormalised at every step (an identity in exact arithmetic), so sum_k exp logWs[t,b,k] = 1 to fp32 rounding.
 *
 * One persistent workgroup per sequence walks t downwards; the N x N tile is recomputed in both pair phases and never
 * written to HBM; no MLP is evaluated.  No atomics and every sum in a fixed order: two calls on the same inputs give
 * bit-identical outputs, with or without PSVO_TUNE_DETERMINISTIC.  No gradient: the outputs are evaluation quantities.
 *
 *  desc            B, T, N, Dx are read; nothing else is looked at.  Dx in {2,3,4}, N <= 512 (else PSVO_ERR_UNSUPPORTED);
 *                  T = 1 is valid (the output is then the normalised filter weights)
 *  X, Fm (T,B,Dx,N) outputs of psvo_filter_forward / psvo_filter_forward_cov
 *  Fs  (T,B,Dx,N)  per-particle transition scales (psvo_filter_forward_cov), or NULL
 *  sig_f (Dx)      constant transition scale, or NULL; exactly one of Fs / sig_f (else PSVO_ERR_INVALID)
 *  logW (T,B,N)    the filter's log-weights (entries of -inf are particles of weight zero)
 *  u (T,B,N)       uniforms in [0,1) for N multinomial draws per step from exp logWs[t,b,:], or idx_in (T,B,N) teacher-forced
 *                  draws (values clamped to [0, N)); both NULL = no draw.  The draw is the filter's: cdf[idx-1] <= u total < cdf[idx]
 *                  on the inclusive prefix sums of the weights, last index clamped
 *  outputs: logWs (T,B,N) normalised smoothed log-weights (required);
 *           Xmean (T,B,Dx) = sum_k exp(logWs[t,b,k]) X[t,b,:,k] and ess (T,B) = 1 / sum_k exp(2 logWs[t,b,k]), each may be NULL;
 *           Xs (T,B,Dx,N) = X[t,b,:,idx] and idx_out (T,B,N), each may be NULL; non-NULL needs u or idx_in (else PSVO_ERR_INVALID).
 * ------------------------------------------------------------------------------------------- */
int psvo_ffbs_smooth(const psvo_desc* desc,
                     const float* X, const float* Fm, const float* Fs, const float* sig_f, const float* logW,
                     const float* u, const int32_t* idx_in,
                     float* logWs, float* Xmean, float* ess, float* Xs, int32_t* idx_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward-sampled trajectories (forward filtering, backward simulation: FFBSi) on the particle system a forward filter left
 * in HBM: N whole paths per sequence, where psvo_ffbs_smooth draws every step on its own from the smoothed marginals.  Added
 * within ABI 6: purely additive.  Notation of psvo_ffbs_smooth (a_t, l_t, s_t); per sequence b and trajectory n = 0..N-1:
 *     t = T-1 :  v[n,k] = a_{T-1}[k]
 *     t < T-1 :  v[n,k] = a_t[k] + l_t(X[t+1,b,:,j_{t+1}(n)]; k)
 *     j_t(n)      = #{k : cdf_n[k] <= u[t,b,n] total_n}, clamped to N-1    (the filter's draw; cdf_n = inclusive prefix sums in
 *                   k order of exp(v[n,k] - shift_n), total_n their sum)
 *     logq[t,b,n] = v[n,j_t(n)] - logsumexp_k v[n,:]
 *     Xs[t,b,:,n] = X[t,b,:,j_t(n)]
 *     distinct[t,b] = number of different values among j_t(0..N-1)
 * sum_t logq[t,b,n] is the log-probability of path n under the sampler; distinct is the path-degeneracy diagnostic (the
 * counterpart of the smoother's ess).  The kernel shifts by the log-sum-exp itself, so its weights are normalised and
 * total_n = 1 to the rounding of one fp32 number; where cdf_n ends below u the draw is clamped to the LAST PARTICLE WITH
 * logW > -inf.  A particle of weight zero (logW = -inf) is never drawn.
 *
 * One persistent workgroup per sequence walks t downwards, a lane per trajectory; the N x N tile is recomputed in both pair
 * phases of a step and never stored; no MLP is evaluated.  No atomics and every sum in a fixed order: two calls on the same
 * inputs give bit-identical outputs, with or without PSVO_TUNE_DETERMINISTIC.  No gradient.
 *
 *  desc            B, T, N, Dx are read; nothing else is looked at.  Dx in {2,3,4}, N <= 512 (else PSVO_ERR_UNSUPPORTED);
 *                  T = 1 is valid (N draws from the normalised filter weights)
 *  X, Fm, Fs, sig_f, logW   as for psvo_ffbs_smooth; exactly one of Fs / sig_f (else PSVO_ERR_INVALID)
 *  u (T,B,N)       uniforms in [0,1), one per trajectory and step, or NULL
 *  idx_in (T,B,N)  teacher-forced indices (values clamped to [0, N)), or NULL; at least one of u / idx_in (else
 *                  PSVO_ERR_INVALID), idx_in wins.  logq, Xs and distinct are produced for the forced indices
 *  outputs: Xs (T,B,Dx,N), idx_out (T,B,N), logq (T,B,N), distinct (T,B); each may be NULL, not all (else PSVO_ERR_INVALID).
 * ------------------------------------------------------------------------------------------- */
int psvo_ffbs_sample(const psvo_desc* desc,
                     const float* X, const float* Fm, const float* Fs, const float* sig_f, const float* logW,
                     const float* u, const int32_t* idx_in,
                     float* Xs, int32_t* idx_out, float* logq, int32_t* distinct, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Particle forecast: the k-step predictive distribution of a weighted particle cloud, k = 0..K, from every origin t of a
 * sequence at once.  Added within ABI 6: purely additive.  Per sequence b and origin t:
 *     w_n         = softmax_n(logW[t,b,:])                     (1 / N without logW)
 *     x^(0)_n     = X[t,b,:,n]
 *     x^(k+1)_n   = MLP_f(x^(k)_n) + sig_f (*) eps[k,t,b,:,n]  (no noise term without eps)
 *     mu_n        = MLP_g(x^(k)_n)                             (emission 0);  softplus(MLP_g(x^(k)_n)) + 1e-6  (emission 1, 2)
 *     ymean[k,t,b,:] = sum_n w_n mu_n
 *     yvar [k,t,b,:] = sum_n w_n mu_n^2 - ymean^2 + v,          v = sig_g^2 (emission 0), 1 (emission 1), ymean (emission 2)
 *     xmean[k,t,b,:] = sum_n w_n x^(k)_n
 *     lpd  [k,t,b]   = logsumexp_n(log w_n + log g(obs[t+k,b,:] | x^(k)_n))   where t + k < T, else exactly 0
 * with log g as the filter kernels score it: the diagonal normal around mu_n with scale sig_g (emissions 0 and 1; the caller
 * passes ones for the unit-scale normal of emission 1) or sum_e y_e log mu_n,e - mu_n,e - log Gamma(y_e + 1) (emission 2).
 * ymean, yvar and xmean are produced for every (k, t), past the end of the data included.  The caller passes q1's MLP and
 * scale as f under the bootstrap wiring; desc->bootstrap is not looked at.
 *
 * A lane per particle, a workgroup per origin (four origins where N <= 64); the horizon loop runs in the kernel with one
 * workgroup barrier per horizon.  No atomics and every sum in a fixed order (wave scan, then the waves in wave order): two
 * calls on the same inputs give bit-identical outputs, with or without PSVO_TUNE_DETERMINISTIC.  No gradient.
 *
 *  desc            B, T, N, Dx, Dy, H, emission, layers are read.  Dx in {2,3,4}, 1 <= Dy <= 32, H in {16,32,64}, N <= 512,
 *                  emission in {0,1,2}, one hidden layer (layers = 2: PSVO_ERR_UNSUPPORTED, as everything outside this list)
 *  K               horizons beyond the origin, >= 0 (K = 0: the cloud read through the emission, no transition)
 *  f, g            MLP_f (Dx -> Dx) and MLP_g (Dx -> Dy), one hidden layer of width H
 *  sig_f (Dx)      transition scale; may be NULL without eps
 *  sig_g (Dy)      emission scale; may be NULL for emission 2 only
 *  X (T,B,Dx,N)    the cloud at every origin (the filter's Xanc, backward-sampled paths, ...)
 *  logW (T,B,N)    log-weights of the cloud, or NULL = equal weights; entries of -inf are particles of weight zero
 *  obs (T,B,Dy)    observations, or NULL (then lpd must be NULL)
 *  eps (K,T,B,Dx,N) standard normals, or NULL = noise-free propagation of every particle
 *  outputs: ymean, yvar (K+1,T,B,Dy), xmean (K+1,T,B,Dx), lpd (K+1,T,B); each may be NULL, not all (else PSVO_ERR_INVALID).
 * ------------------------------------------------------------------------------------------- */
int psvo_particle_forecast(const psvo_desc* desc, int K,
                           const psvo_mlp* f, const psvo_mlp* g, const float* sig_f, const float* sig_g,
                           const float* X, const float* logW, const float* obs, const float* eps,
                           float* ymean, float* yvar, float* xmean, float* lpd, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Particle forecast on missing observations (added within ABI 6: purely additive).  psvo_particle_forecast with one change of
 * meaning: a NaN in obs[t+k,b,e] is an entry that was not observed (the rule of psvo_filter_forward_wobs_missing), and
 *     lpd[k,t,b] = logsumexp_n(log w_n + sum_{e observed} term_e(x^(k)_n))
 * with the terms added in the order e = 0 .. Dy-1: -1/2 z_e^2 - log sig_g[e] - 1/2 log 2 pi (emissions 0 and 1, the constant with
 * its term) or y_e log mu_e - mu_e - log Gamma(y_e + 1) (emission 2).  The choice is a select on a broadcast; a NaN never reaches
 * a sum.  lpd is exactly 0 where t + k >= T and where the target row has nothing observed.  ymean, yvar and xmean do not read
 * obs and equal psvo_particle_forecast's bit for bit.  With every entry observed lpd equals psvo_particle_forecast's bit for
 * bit for emission 2 and to rounding for emissions 0 and 1 (the sum groups differently).  No atomics, the same fold order: two
 * calls give bit-identical outputs.  Arguments, envelope and refusals are those of psvo_particle_forecast, which itself still
 * answers NaN for a NaN target.
 * ------------------------------------------------------------------------------------------- */
int psvo_particle_forecast_missing(const psvo_desc* desc, int K,
                           const psvo_mlp* f, const psvo_mlp* g, const float* sig_f, const float* sig_g,
                           const float* X, const float* logW, const float* obs, const float* eps,
                           float* ymean, float* yvar, float* xmean, float* lpd, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Particle forecast under exogenous inputs (added within ABI 6: purely additive).  psvo_particle_forecast_missing with an
 * input-driven transition, x_{t+1} ~ f(. | x_t, v_t): the first layer of MLP_f is applied to concat[x, v], and the input's share
 * of its pre-activation is handed over as rows, as psvo_filter_forward_wobs_input takes them,
 *     hb_f[s,b,:] = v[b,s,:] W1[Dx:]                  (Tv,B,H) at the kernel width, zero beyond the model's hidden width,
 * while f.W1 holds the state's rows W1[:Dx] alone.  The transition from horizon k to k + 1 of origin (t, b) is
 *     x^(k+1)_n = relu(x^(k)_n W1[:Dx] + (b1 + hb_f[t+k,b,:])) W2 + b2 + sig_f (*) eps[k,t,b,:,n]:
 * the state of origin t at horizon k meets v_{t+k}.  Tv >= T; rows T .. Tv-1 are inputs planned past the end of the data, and
 * where t + k >= Tv the bias is b1 alone (zero input, the rule of the filter's t = 0 terms).  b1 + hb_f is ONE fp32 add, made
 * once per (origin, horizon); everything else is the arithmetic of psvo_particle_forecast_missing in its order, so hb_f = 0
 * gives that call's outputs bit for bit, and with K = 0 no row is used.  Emission, moments, lpd, NaN = not observed and the fold
 * orders are those of psvo_particle_forecast_missing; no atomics: two calls give bit-identical outputs.
 * PSVO_ERR_INVALID for hb_f == NULL or Tv < T (beside the refusals of psvo_particle_forecast); PSVO_ERR_UNSUPPORTED exactly
 * where psvo_particle_forecast_missing answers it.
 * ------------------------------------------------------------------------------------------- */
int psvo_particle_forecast_input(const psvo_desc* desc, int K,
                           const psvo_mlp* f, const psvo_mlp* g, const float* sig_f, const float* sig_g,
                           const float* X, const float* logW, const float* obs, const float* eps,
                           float* ymean, float* yvar, float* xmean, float* lpd,
                           const float* hb_f, int Tv, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MAP trajectory (particle Viterbi; Godsill, Doucet and West 2001) on the particle system a forward filter left in HBM: the
 * single most probable path through the T x N lattice of particles, where psvo_ffbs_smooth gives marginals and
 * psvo_ffbs_sample random paths.  Added within ABI 6: purely additive.  Notation of psvo_ffbs_smooth; per sequence b:
 *     G_t[j]   = sum_{e : obs[t,b,e] is not NaN} term_e(X[t,b,:,j])   terms, order e = 0..Dy-1 and constants exactly as in
 *                                                                     psvo_particle_forecast_missing; exactly 0 where nothing
 *                                                                     is observed
 *     l_t[j,k] = log N(X[t+1,b,:,j]; Fm[t,b,:,k], sig_f)              diagonal, on scales, the -sum log sig_f term included
 *     d_0[j]   = log N(X[0,b,:,j]; fm0[b,:], fsig0) + G_0[j]
 *     d_t[j]   = G_t[j] + max_k (delta[t-1,b,k] + l_{t-1}[j,k])       bp[t,b,j] = the LOWEST k that attains the max;
 *                                                                     bp[0,b,j] = j
 *     lmax[t,b]    = max_j d_t[j]
 *     delta[t,b,j] = d_t[j] - lmax[t,b]                               natural log; renormalised every step like the filter's lse
 *     path[T-1,b]  = the lowest j with delta[T-1,b,j] == 0
 *     path[t-1,b]  = bp[t,b,path[t,b]]
 *     Xmap[t,b,:]  = X[t,b,:,path[t,b]]
 * sum_t lmax[t,b] is the joint log-density of the best path, log p(x*_{0:T-1}, observed y), maximised over all N^T paths in
 * O(T N^2).  logW is not read: every particle is a lattice node whatever its weight.  A NaN in obs is always an entry that was
 * not observed (the rule of psvo_filter_forward_wobs_missing); there is no second form.  Precondition: X, Fm, scales and weights
 * are finite.  Whatever the inputs hold, every bp and path entry lies in [0, N) and nothing is addressed with a value read from
 * the data: every argmax starts at 0 and moves on strict `>`.
 *
 * Two launches: the emission terms G for every (t, b) at once (a lane per particle, written into delta), then one persistent
 * workgroup per sequence that walks t upwards with one N x N pair phase per step (the tile is recomputed, never stored; no
 * exponential) and backtracks behind a workgroup barrier.  No atomics, every maximum in a fixed order with the lowest index
 * winning ties: two calls on the same inputs give bit-identical outputs, with or without PSVO_TUNE_DETERMINISTIC.  No gradient.
 *
 *  desc            B, T, N, Dx, Dy, H, emission, layers are read.  Dx in {2,3,4}, 1 <= Dy <= 32, H in {16,32,64}, N <= 512,
 *                  emission in {0,1,2}, one hidden layer (everything outside this list: PSVO_ERR_UNSUPPORTED).  T = 1 and
 *                  N = 1 are valid
 *  g               MLP_g (Dx -> Dy), one hidden layer of width H
 *  sig_f (Dx)      the constant transition scale the filter weighted with
 *  sig_g (Dy)      emission scale; may be NULL for emission 2 only
 *  fm0 (B,Dx), fsig0 (Dx)   mean and scale of the t = 0 transition term, as psvo_filter_forward takes them
 *  obs (T,B,Dy)    observations; NaN = not observed
 *  X, Fm (T,B,Dx,N) outputs of the forward filter
 *  outputs: delta (T,B,N), lmax (T,B), bp (T,B,N) int32 (all required; delta and bp are also the kernel's workspace);
 *           path (T,B) int32 and Xmap (T,B,Dx), each may be NULL (both NULL: no backtrack).
 *  Every other NULL, and B, T or N <= 0, returns PSVO_ERR_INVALID before any launch.
 * ------------------------------------------------------------------------------------------- */
int psvo_map_path(const psvo_desc* desc, const psvo_mlp* g, const float* sig_f, const float* sig_g,
                  const float* fm0, const float* fsig0, const float* obs, const float* X, const float* Fm,
                  float* delta, float* lmax, int32_t* bp, int32_t* path, float* Xmap, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward simulation with proposal, STATE-DEPENDENT diagonal scales (FLAGS.output_cov and FLAGS.diag_cov; see
 * psvo_filter_forward_cov).  Same loop and outputs as psvo_bsim_forward (PSVO.backward_simulation_w_proposal, reference
 * src/SMC/PSVO.py:69-203); differences:
 *  Fm, Fs (T,B,Dx,N)   mean AND scale of f given every forward particle (outputs of psvo_filter_forward_cov): the transition
 *                  tile (PSVO.py:128-133, never materialised) has a scale per forward particle
 *  f, g, q1_inv    W2 = [mu_layer | sigma_layer] (H, 2 Dout), b2 (2 Dout); one hidden layer; desc->emission = 1 drops MLP_g's
 *                  covariance head as the reference's tf_poisson does
 *  sigc_f, sigc_q1inv (Dx), sigc_g (Dy)   the sigma_con parts
 *  bmu2, bsig2 (T,B,Dx); minit, sinit, imean, isig (B,Dx)   hoisted means and scales per row (BSim_q2; BSim_q_init at
 *                  t = T-1; the t = 0 prior term f / q0 at mu_0, PSVO.py:169-175)
 *  saves (all four or none; required by psvo_bsim_backward_cov): lam_all (T,B,N,M) log2-domain filter term, om_all (T,B,N,M)
 *                  normalised sub-particle log-weights, mu1_all / s1_all (T,B,Dx,N) mean and scale of q1_inv given bwX[t+1].
 * ------------------------------------------------------------------------------------------- */
int psvo_bsim_forward_cov(const psvo_desc* desc,
                          const float* Fm, const float* Fs, const float* logW, const float* lse,
                          const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                          const float* sigc_f, const float* sigc_g, const float* sigc_q1inv,
                          const float* bmu2, const float* bsig2,
                          const float* minit, const float* sinit, const float* imean, const float* isig,
                          const float* obs, const float* eps_b, const float* u_b, const int32_t* sel_in,
                          float* bwX, float* flp, float* glp, float* Omega, int32_t* sel_out, float* score,
                          float* lam_all, float* om_all, float* mu1_all, float* s1_all,
                          void* stream);

/* Reverse mode of psvo_bsim_forward_cov (TensorFlow autodiff of the loop in the reference, src/trainer.py:115-118).
 *  inputs  : the forward call's inputs, its outputs bwX, sel, the four saves, and dscore (B,N) = d loss / d score.
 *  outputs : rows for psvo_mlp_wgrad, w.r.t. the mu_layer output and w.r.t. the RAW sigma_layer output of every MLP
 *            evaluation: xt (T,B,Dx,N,M) sub-particles, dFt / dFts (T,B,Dx,N,M) for MLP_f(x~), dGt / dGts (T,B,Dy,N,M)
 *            for MLP_g(x~), dmu1 / dmu1s (T,B,Dx,N) for MLP_q1inv(bwX[t+1]);
 *            ACCUMULATED with float atomics -- the caller zero-fills them: dFm, dFs (T,B,Dx,N), dlogW (T,B,N), dlse (T,B)
 *            (-> psvo_filter_backward_cov as dFm_ext, dFs_ext, dlogW_ext and added to dlse), dbmu2, dbsig2 (T,B,Dx),
 *            dminit, dsinit, dimean, disig (B,Dx), dsigc_f, dsigc_q1inv (Dx), dsigc_g (Dy).
 *  The summation order of the atomics is not fixed: results are reproducible to rounding, not bit for bit, unless
 *  PSVO_TUNE_DETERMINISTIC is 1 (psvo_bsim_backward_cov_ws: fixed-order slices and folds instead of the atomics). */
int psvo_bsim_backward_cov(const psvo_desc* desc,
                           const float* Fm, const float* Fs, const float* logW, const float* lse,
                           const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                           const float* sigc_f, const float* sigc_g, const float* sigc_q1inv,
                           const float* bmu2, const float* bsig2,
                           const float* minit, const float* sinit, const float* imean, const float* isig,
                           const float* obs, const float* eps_b, const float* bwX, const int32_t* sel,
                           const float* lam_all, const float* om_all, const float* mu1_all, const float* s1_all,
                           const float* dscore,
                           float* xt, float* dFt, float* dFts, float* dGt, float* dGts, float* dmu1, float* dmu1s,
                           float* dFm, float* dFs, float* dlogW, float* dlse,
                           float* dbmu2, float* dbsig2,
                           float* dminit, float* dsinit, float* dimean, float* disig,
                           float* dsigc_f, float* dsigc_g, float* dsigc_q1inv,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * PSVOwR (backward simulation WITH RESAMPLING across the chains, reference src/SMC/PSVOwR.py:65-198) with state-dependent
 * diagonal scales.  Inputs as psvo_bsim_forward_cov plus u_r (T,B,N) uniforms of the cross-chain draw (or anc_in (T,B,N)
 * teacher-forced ancestors); outputs as psvo_bsimwr_forward: bwX, bwXanc (T,B,Dx,N), bwW (T,B,N) per-step chain
 * log-weights, lseW (T,B) = logsumexp_n bwW, sel_out, anc_out (T,B,N), plus omsel (T,B,N) (the drawn sub-particles'
 * normalised log-weights = the logits of the cross-chain draw; required) and the four saves.
 * The cross-chain draw couples every chain of a sequence once per step: the loop is T + 2 launches (one per time step,
 * one for the draw of step 0, one for lseW) issued by this call on `stream`; no cooperative launch, no workspace.
 * psvo_bsimwr_backward_cov: its reverse (T launches); outputs as psvo_bsim_backward_cov (rows; accumulated with float
 * atomics into zero-filled dFm, dFs, dlogW, dlse, dbmu2, dbsig2, dminit, dsinit, dimean, disig, dsigc_*); the q1_inv rows
 * dmu1 / dmu1s pair with the inputs bwXanc[t+1]; dXs (T,B,Dx,N): zero-filled workspace (d loss / d bwX).
 * ------------------------------------------------------------------------------------------- */
long long psvo_bsim_cov_det_ws_floats(int B, int N, int M, int Dx, int Dy);
int psvo_bsim_backward_cov_ws(const psvo_desc* desc,
                              const float* Fm, const float* Fs, const float* logW, const float* lse,
                              const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                              const float* sigc_f, const float* sigc_g, const float* sigc_q1inv,
                              const float* bmu2, const float* bsig2,
                              const float* minit, const float* sinit, const float* imean, const float* isig,
                              const float* obs, const float* eps_b, const float* bwX, const int32_t* sel,
                              const float* lam_all, const float* om_all, const float* mu1_all, const float* s1_all,
                              const float* dscore,
                              float* xt, float* dFt, float* dFts, float* dGt, float* dGts, float* dmu1, float* dmu1s,
                              float* dFm, float* dFs, float* dlogW, float* dlse,
                              float* dbmu2, float* dbsig2,
                              float* dminit, float* dsinit, float* dimean, float* disig,
                              float* dsigc_f, float* dsigc_g, float* dsigc_q1inv,
                              float* det_ws, void* stream);

int psvo_bsimwr_forward_cov(const psvo_desc* desc,
                            const float* Fm, const float* Fs, const float* logW, const float* lse,
                            const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                            const float* sigc_f, const float* sigc_g, const float* sigc_q1inv,
                            const float* bmu2, const float* bsig2,
                            const float* minit, const float* sinit, const float* imean, const float* isig,
                            const float* obs, const float* eps_b, const float* u_b, const float* u_r,
                            const int32_t* sel_in, const int32_t* anc_in,
                            float* bwX, float* bwXanc, float* bwW, float* lseW, int32_t* sel_out, int32_t* anc_out,
                            float* omsel, float* lam_all, float* om_all, float* mu1_all, float* s1_all,
                            void* stream);
int psvo_bsimwr_backward_cov(const psvo_desc* desc,
                             const float* Fm, const float* Fs, const float* logW, const float* lse,
                             const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                             const float* sigc_f, const float* sigc_g, const float* sigc_q1inv,
                             const float* bmu2, const float* bsig2,
                             const float* minit, const float* sinit, const float* imean, const float* isig,
                             const float* obs, const float* eps_b,
                             const float* bwXanc, const float* bwW, const float* lseW,
                             const int32_t* sel, const int32_t* anc,
                             const float* lam_all, const float* om_all, const float* mu1_all, const float* s1_all,
                             const float* dlseW,
                             float* xt, float* dFt, float* dFts, float* dGt, float* dGts, float* dmu1, float* dmu1s,
                             float* dFm, float* dFs, float* dlogW, float* dlse,
                             float* dbmu2, float* dbsig2,
                             float* dminit, float* dsinit, float* dimean, float* disig,
                             float* dsigc_f, float* dsigc_g, float* dsigc_q1inv,
                             float* dXs, void* stream);
int psvo_bsimwr_backward_cov_ws(const psvo_desc* desc,
                                const float* Fm, const float* Fs, const float* logW, const float* lse,
                                const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                                const float* sigc_f, const float* sigc_g, const float* sigc_q1inv,
                                const float* bmu2, const float* bsig2,
                                const float* minit, const float* sinit, const float* imean, const float* isig,
                                const float* obs, const float* eps_b,
                                const float* bwXanc, const float* bwW, const float* lseW,
                                const int32_t* sel, const int32_t* anc,
                                const float* lam_all, const float* om_all, const float* mu1_all, const float* s1_all,
                                const float* dlseW,
                                float* xt, float* dFt, float* dFts, float* dGt, float* dGts, float* dmu1, float* dmu1s,
                                float* dFm, float* dFs, float* dlogW, float* dlse,
                                float* dbmu2, float* dbsig2,
                                float* dminit, float* dsinit, float* dimean, float* disig,
                                float* dsigc_f, float* dsigc_g, float* dsigc_q1inv,
                                float* dXs, float* det_ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward simulation with proposal.  Replaces PSVO.backward_simulation_w_proposal
 * (reference src/SMC/PSVO.py:69-203): the (M, N, N, B) transition tile (:128-133) is never
 * materialised -- forward-particle means are staged in LDS and reduced with an online
 * log-sum-exp.
 *
 *  X, Fm, logW, lse      outputs of psvo_filter_forward (pre-resampling history, PSVO.py:39)
 *  f, g, q1_inv          per-particle MLPs (f == q1 when bootstrap: pass q1)
 *  sig_f, sig_g, sig_q1inv, sig_bq2 (Dx / Dy)
 *  bmu2 (T,B,Dx)         hoisted MLP_BSim_q2(enc_t[b])
 *  minit (B,Dx), sig_init (Dx)   MLP_BSim_q_init(enc_{T-1}[b]), its sigma (PSVO.py:86-87)
 *  imean (B,Dx), isig (Dx)       t=0 "filter" term: (MLP_q0(mu_0), sigma_q0) when
 *                        bootstrap&&two_q else (MLP_f(mu_0), sigma_f) (PSVO.py:169-173)
 *  obs (T,B,Dy); eps_b (T,B,Dx,N,M) normal draws; u_b (T,B,N) uniforms; sel_in (T,B,N) or NULL
 *
 *  outputs: bwX (T,B,Dx,N) (bw_Xs), flp (T,B,N) (f_log_probs), glp (T,B,N) (g_log_probs),
 *  Omega (T,B,N) (bw_log_Omegas), sel_out (T,B,N) chosen sub-particle, score (B,N) =
 *  sum_t(flp+glp-Omega) (psvo_elbo_bsim turns it into logsumexp_n score - log N, PSVO.py:52-67).
 *  lam2_all (T,B,N,M), om_all (T,B,N,M), mu1_all (T,B,Dx,N): optional (NULL) saves for
 *  psvo_bsim_backward -- the log2-domain filter term, the normalised sub-particle log-weights and
 *  MLP_q1inv(bwX[t+1]).
 * ------------------------------------------------------------------------------------------- */
int psvo_bsim_forward(const psvo_desc* desc,
                      const float* X, const float* Fm, const float* logW, const float* lse,
                      const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                      const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
                      const float* bmu2, const float* minit, const float* sig_init,
                      const float* imean, const float* isig,
                      const float* obs, const float* eps_b, const float* u_b, const int32_t* sel_in,
                      float* bwX, float* flp, float* glp, float* Omega, int32_t* sel_out,
                      float* score,
                      float* lam2_all, float* om_all, float* mu1_all,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reverse mode of psvo_bsim_forward (TensorFlow autodiff of PSVO.backward_simulation_w_proposal in
 * the reference, src/trainer.py:115-118).  The N x N tile is recomputed, not stored.
 *
 *  inputs  : the forward call's inputs (eps_b as drawn), its outputs bwX, sel and the three optional
 *            saves lam2_all (T,B,N,M), om_all (T,B,N,M), mu1_all (T,B,Dx,N) (required here), and
 *            dscore (B,N) = d loss / d score.
 *  outputs : rows for psvo_mlp_wgrad: xt (T,B,Dx,N,M) sub-particles, dFt (T,B,Dx,N,M) w.r.t.
 *            MLP_f(x~), dGt (T,B,Dy,N,M) w.r.t. MLP_g(x~), dmu1 (T,B,Dx,N) w.r.t. MLP_q1inv(bwX[t+1]);
 *            per-workgroup partials (nblk = psvo_bsim_blocks(desc)) dFm_part (T,B,nblk,Dx,N), dlogW_part (T,B,nblk,N)
 *            and sacc_part (B * nblk * psvo_bsim_acc_size(Dx, Dy) floats) for psvo_bsim_backward_fold;
 *            per-chain rows (to be summed over N): dbmu2_rows (T,B,Dx,N), dminit_rows (B,Dx,N), dimean_rows (B,Dx,N).
 *  The gradient w.r.t. lse is zero analytically (the normalised weights' gradients sum to zero per chain) and of the
 *  size of its fp32 rounding numerically; it is returned all the same (dlse below), as autodiff of the reference's graph
 *  carries it: psvo_filter_backward then subtracts the softmax-weighted sum from d logW, which is what keeps that pass
 *  well-conditioned when the forward particles are far from the data (tests/test_gpu_notebook_curve.py).
 *
 * psvo_bsim_backward_fold (one launch, to be issued right behind): folds the partials in workgroup order into
 *            dFm (T,B,Dx,N), dlogW (T,B,N) = d loss / d (Fm, logW) of the forward filter -> psvo_filter_backward, and the
 *            scale gradients dsig_f, dsig_q1inv, dsig_bq2, dsig_init, disig (Dx), dsig_g (Dy);
 *            dlse (T,B) or NULL = -sum_n dlogW[t,b,n] = d loss / d lse of the forward filter (ABI 5).
 *            Alignment: none is required.  The fold moves 16 bytes per access when N % 4 == 0 and dFm_part, dlogW_part,
 *            dFm and dlogW are all 16-byte aligned, 4 bytes otherwise; every element adds its workgroups in the same order
 *            either way, so the results do not depend on which is taken.
 * ------------------------------------------------------------------------------------------- */
int psvo_bsim_blocks(const psvo_desc* desc);      /* nblk for this problem under the current PSVO_TUNE_BSIM_BWD setting */
int psvo_bsim_acc_size(int Dx, int Dy);
int psvo_bsim_backward(const psvo_desc* desc,
                       const float* Fm, const float* logW, const float* lse,
                       const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                       const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
                       const float* bmu2, const float* minit, const float* sig_init,
                       const float* imean, const float* isig,
                       const float* obs, const float* eps_b,
                       const float* bwX, const int32_t* sel,
                       const float* lam2_all, const float* om_all, const float* mu1_all,
                       const float* dscore,
                       float* xt, float* dFt, float* dGt, float* dmu1,
                       float* dFm_part, float* dlogW_part,
                       float* dbmu2_rows, float* dminit_rows, float* dimean_rows,
                       float* sacc_part, void* stream);
int psvo_bsim_backward_fold(const psvo_desc* desc, const float* dFm_part, const float* dlogW_part, const float* sacc_part,
                            const float* sig_q1inv, const float* sig_bq2, float* dFm, float* dlogW,
                            float* dsig_f, float* dsig_g, float* dsig_q1inv, float* dsig_bq2, float* dsig_init,
                            float* disig, float* dlse, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PSVOwR: backward simulation with cross-chain resampling and a per-step ELBO.
 * Replaces PSVOwR.backward_simulation_w_resampling (reference src/SMC/PSVOwR.py:65-198), called from
 * PSVOwR.get_log_ZSMC (src/SMC/PSVOwR.py:38-62).  A sequence is owned by a cluster of
 * psvo_bsimwr_blocks(B, N, M) persistent workgroups (cooperative launch) that meet at one barrier per step.
 *
 *  inputs  : as psvo_bsim_forward (the filter's Fm, logW, lse; the hoisted backward-proposal inputs),
 *            plus  u_r (T,B,N) uniforms of the cross-chain multinomial draw (or NULL with anc_in)
 *                  anc_in (T,B,N) teacher-forced cross-chain ancestors (NULL = draw from u_r).
 *            The reference resamples after every step including t = 0 (PSVOwR.py:150-160, 187-196).
 *  outputs : bwX    (T,B,Dx,N) selected sub-particle of every chain before the cross-chain draw
 *            bwXanc (T,B,Dx,N) the resampled chains, bwXanc[t][k] = bwX[t][anc[t][k]]  (the returned
 *                              trajectories bw_Xs, PSVOwR.py:198)
 *            bwW    (T,B,N)    bw_log_W of the step (PSVOwR.py:135-142), lseW (T,B) = logsumexp_n bwW
 *                              (ELBO = sum_t lseW[t] - T log N, PSVOwR.py:144-148, 184-185)
 *            sel_out, anc_out (T,B,N) drawn sub-particle / cross-chain ancestor indices
 *            lam2_all (T,B,N,M), om_all (T,B,N,M), mu1_all (T,B,Dx,N): optional saves for
 *            psvo_bsimwr_backward.
 *  ws      : workspace, psvo_bsimwr_ws_floats(B, T, N) floats, 8-byte aligned (a two-step ring of tagged 64-bit
 *            words through which the workgroups of a sequence exchange the chains' selected states and
 *            log-weights; its last word is nonzero afterwards iff a poll timed out).
 * ------------------------------------------------------------------------------------------- */
int psvo_bsimwr_blocks(int B, int N, int M);
long long psvo_bsimwr_ws_floats(int B, int T, int N);
int psvo_bsimwr_forward(const psvo_desc* desc,
                        const float* Fm, const float* logW, const float* lse,
                        const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                        const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
                        const float* bmu2, const float* minit, const float* sig_init,
                        const float* imean, const float* isig,
                        const float* obs, const float* eps_b, const float* u_b, const float* u_r,
                        const int32_t* sel_in, const int32_t* anc_in,
                        float* bwX, float* bwXanc, float* bwW, float* lseW,
                        int32_t* sel_out, int32_t* anc_out,
                        float* lam2_all, float* om_all, float* mu1_all,
                        float* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reverse mode of psvo_bsimwr_forward (TensorFlow autodiff of the loop above, src/trainer.py:115-118).
 *  inputs  : the forward call's inputs and outputs (all three saves required) and dlseW (T,B) =
 *            d loss / d lseW.
 *  outputs : rows for psvo_mlp_wgrad: xt, dFt (T,B,Dx,N,M), dGt (T,B,Dy,N,M), dmu1 (T,B,Dx,N) w.r.t.
 *            MLP_q1inv(bwXanc[t+1]);  per-workgroup partials (K = psvo_bsimwr_blocks(B, N, M), to be summed
 *            over that axis) dFm_part (T,B,K,Dx,N), dlogW_part (T,B,K,N), dlse_part (T,B,K) ->
 *            psvo_filter_backward (here the gradient w.r.t. the filter's lse is NOT zero);
 *            per-chain rows (to be summed over N) dbmu2_rows (T,B,Dx,N), dminit_rows (B,Dx,N),
 *            dimean_rows (B,Dx,N); scale gradients as psvo_bsim_backward.
 *  sacc    : workspace, B * K * psvo_bsim_acc_size(Dx, Dy) floats.
 *  ws      : workspace, psvo_bsimwr_bwd_ws_floats(B, T, N, Dx) floats, 8-byte aligned (d loss / d bwXanc exchanged
 *            between the workgroups of a sequence as tagged 64-bit words; last word nonzero iff a poll timed out).
 * ------------------------------------------------------------------------------------------- */
long long psvo_bsimwr_bwd_ws_floats(int B, int T, int N, int Dx);
int psvo_bsimwr_backward(const psvo_desc* desc,
                         const float* Fm, const float* logW, const float* lse,
                         const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                         const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
                         const float* bmu2, const float* minit, const float* sig_init,
                         const float* imean, const float* isig,
                         const float* obs, const float* eps_b,
                         const float* bwXanc, const float* bwW, const float* lseW,
                         const int32_t* sel, const int32_t* anc,
                         const float* lam2_all, const float* om_all, const float* mu1_all,
                         const float* dlseW,
                         float* xt, float* dFt, float* dGt, float* dmu1,
                         float* dFm_part, float* dlogW_part, float* dlse_part,
                         float* dbmu2_rows, float* dminit_rows, float* dimean_rows,
                         float* dsig_f, float* dsig_g, float* dsig_q1inv, float* dsig_bq2, float* dsig_init,
                         float* disig, float* sacc, float* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reverse mode of psvo_filter_forward.  The reference obtains these gradients from TensorFlow
 * autodiff of the tf.while_loop (reference src/trainer.py:115-118; no stop_gradient in src/,
 * SURVEY.md Appendix B).  One persistent workgroup per sequence walks t = T-1 .. 0; in the bootstrap wiring with
 * resampling (one hidden layer) the pass may instead run as an affine scan -- coefficients of every step in one parallel launch,
 * one or four waves per sequence for the recurrence, rows and sums in a third launch (PSVO_TUNE_FILTER_BWD; same outputs).
 *
 *  inputs  : everything psvo_filter_forward took (eps as drawn), its outputs X, Fm, P1 (NULL when
 *            bootstrap), logW, lse, idx, and the upstream gradients
 *              dlse      (T,B)              d loss / d lse[t,b]            (NULL = 0)
 *              dFm_ext   (T,B,nparts,Dx,N)  d loss / d Fm, summed over the `nparts` axis (NULL = 0)
 *              dlogW_ext (T,B,nparts,N)     d loss / d logW, likewise      (NULL = 0)
 *            (nparts = workgroups per sequence of psvo_bsim_backward, which writes partials).
 *  outputs : per-evaluation output gradients for psvo_mlp_wgrad
 *              dP (T,B,Dx,N) w.r.t. MLP_q1(X_t) (includes the transition share when bootstrap),
 *              dF (T,B,Dx,N) w.r.t. MLP_f(X_t) (only when !bootstrap), dG (T,B,Dy,N) w.r.t. MLP_g(X_t);
 *            hoisted-input gradients dmu2 (T,B,Dx), dm0 (B,Dx), dfm0 (B,Dx);
 *            scale gradients dsig_q1, dsig_q2, dsig_f, dsig0, dfsig0 (Dx), dsig_g (Dy).
 *  sacc    : workspace, psvo_filter_ws_floats(B, T, N, Dx, Dy) floats, 16-byte aligned: B * psvo_filter_acc_size(Dx, Dy)
 *            per-sequence sums, the (T,B,Dx,N) per-particle rows of d mu2 (which a parallel kernel sums over N after the
 *            time loop), the affine scan's step records and per-step partial sums.
 *  Aliasing rule: when fm0 and m0 are the SAME buffer (bootstrap and use_2_q: f_0 is q0's own density,
 *            SVO.py:86-92) d m0 receives the sum of both gradients and d fm0 is zero; likewise d sig0 / d fsig0 when
 *            fsig0 and sig0 are the same buffer.
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_acc_size(int Dx, int Dy);
long long psvo_filter_ws_floats(int B, int T, int N, int Dx, int Dy);
int psvo_filter_backward(const psvo_desc* desc,
                         const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                         const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                         const float* mu2,
                         const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                         const float* obs, const float* eps,
                         const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                         const int32_t* idx,
                         const float* dlse, int nparts, const float* dFm_ext, const float* dlogW_ext,
                         float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                         float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                         float* sacc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Adaptive resampling (not in the reference; added within ABI 6: purely additive, no existing struct or signature changed).
 * psvo_filter_forward / psvo_filter_backward with the resampling decision made per (step, sequence) on the device, from the
 * effective sample size of the step's weights.  With w_n = exp(logW[t,b,n] - max_n logW[t,b,:]) over the N particles,
 *     ESS[t,b] = (sum_n w_n)^2 / sum_n w_n^2,        the sequence resamples at t  iff  !(ESS[t,b] >= ess_frac * N)
 * (a NaN ESS resamples).  Every step makes and writes the multinomial draw exactly as psvo_filter_forward with resample = 1
 * does -- idx_out[t] is the draw (idx_in teacher-forces it), Xanc[t] the gathered particles, an equally weighted sample at
 * every step.  Only what step t+1 inherits depends on the decision: resampled, the MLP outputs of the drawn ancestor and the
 * weight -log N; not resampled, the particle's own MLP outputs and the normalised weight logW[t] - lse[t], which then enters
 * logW[t+1] (sum_t lse[t] stays the estimate of log Z in the mixed case).  X, Fm, P1, logW, lse keep meaning and layout.
 *
 *  forward, beyond the arguments of psvo_filter_forward:
 *    ess_frac          the threshold as a fraction of N; > 0.  >= 1 resamples at (almost) every step; a value above 1
 *                      resamples always, a tiny one never.
 *    rs_in  (T,B) int32  teacher-forced decisions (non-zero = resample) or NULL: the analogue of idx_in
 *    rs_out (T,B) int32  the decisions taken (1 = resampled), ess_out (T,B) the ESS they were taken from (also under rs_in)
 *  reverse, beyond the arguments of psvo_filter_backward:
 *    rs     (T,B) int32  the forward pass's rs_out: a constant of the reverse pass, like idx.  The ancestor of particle n at
 *                      step t is rs[t-1] ? idx[t-1][n] : n, and the gradient of the carried weight is applied for exactly the
 *                      steps with rs[t] == 0.  Always the persistent kernels (the affine scan assumes a gather at every
 *                      step); deterministic mode (PSVO_TUNE_DETERMINISTIC) holds as for psvo_filter_backward.
 *    sacc              workspace of psvo_filter_ws_floats(B, T, N, Dx, Dy) floats, as psvo_filter_backward
 *  Envelope of psvo_filter_forward / psvo_filter_backward (Dx 2..4, Dy 1..2, N <= 512, emission 0 / 1, one or two hidden
 *  layers, every wiring).  Refused before a device is touched: ess_frac not > 0 (NaN included), desc->resample == 0, NULL
 *  rs_out / ess_out / rs -- PSVO_ERR_INVALID; nparts > 1 or non-NULL dFm_ext / dlogW_ext (a backward simulation behind an
 *  adaptive filter) -- PSVO_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_forward_adaptive(const psvo_desc* desc,
                        const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                        const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                        const float* mu2,
                        const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                        const float* obs, const float* eps, const float* u, const int32_t* idx_in,
                        float* X, float* Xanc, float* Fm, float* P1, float* logW, int32_t* idx_out,
                        float* lse, float ess_frac, const int32_t* rs_in, int32_t* rs_out, float* ess_out, void* stream);
int psvo_filter_backward_adaptive(const psvo_desc* desc,
                         const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                         const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                         const float* mu2,
                         const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                         const float* obs, const float* eps,
                         const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                         const int32_t* idx,
                         const float* dlse, int nparts, const float* dFm_ext, const float* dlogW_ext,
                         float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                         float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                         float* sacc, const int32_t* rs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Wide observations ("wobs"): the forward filter, its reverse pass and MLP_g's weight gradient for 3 <= Dy <= 32
 * (psvo_amd/csrc/filter_wobs.hip; added within ABI 6 -- the entry points above keep Dy in {1, 2}).  For the filter objectives
 * (SVO, AESMC, IWAE); PSVO's backward simulation has its own wide entry points further down, PSVOwR's stays at Dy <= 2.
 * Envelope of the two filter entry points: 3 <= Dy <= 32 (a run-time bound, nothing is instantiated per width), Dx in {2,3,4},
 * H in {16,32,64} (narrower: zero-padded by the caller as above), N <= 512, one hidden layer (desc->layers <= 1), Gaussian and
 * Poisson emission and the count emission, every bootstrap / two_q wiring, resampling on or off.  Anything else -- Dy <= 2 and
 * Dy > 32 included -- returns PSVO_ERR_UNSUPPORTED before a device is touched.
 *
 * Count emission (desc->emission = 2; the wide entry points of this section and of the next, in their whole envelope).  With
 * r = MLP_g(x) and lam_e = softplus(r_e) + 1e-6 (the mean of emission 1, threshold 20):
 *     log g(y | x) = sum_{e = 0 .. Dy-1} [ y_e log lam_e - lam_e - log Gamma(y_e + 1) ]        (terms added in the order e = 0 .. Dy-1)
 *     d log g / d r_e = (y_e / lam_e - 1) * sigmoid(r_e)
 *   The log Gamma(y_e + 1) term is part of logW, lse, glp and so of the ELBO, which is then a Poisson log-likelihood bound.  It
 *   is computed once per (step, sequence, output) by the lanes that stage the observation row -- in fp64, rounded once: the
 *   fp32 nearest to the true value for every integer y, exactly 0 for y in {0, 1} -- and travels with the row through LDS.
 *   sig_g: pass ones (not read); dsig_g comes back as zeros.  Observations must be finite, non-negative and integer-valued;
 *   the caller checks that (psvo_amd/runner.py: check_counts).  For anything else the result is unspecified, but nothing is
 *   addressed with an observation's value: no read or write leaves its buffer.  psvo_mlp_wgrad_wobs consumes the d G rows as
 *   before.  Every other entry point that reads desc->emission answers PSVO_ERR_UNSUPPORTED for emission = 2.
 *
 * psvo_filter_forward_wobs: arguments, outputs, layouts and the draw rule of psvo_filter_forward (idx = the number of CDF
 *   entries <= u * total, clamped to N - 1; or teacher-forced idx_in), so that psvo_elbo_filter, psvo_ffbs_smooth and the host
 *   code consume the result unchanged.  One persistent workgroup per sequence, lane = particle.  MLP_g's output layer and the
 *   step's observation row are read from LDS at wave-uniform addresses (the row of step t+1 is in flight while step t
 *   computes); the emission log-density adds its Dy terms in the order e = 0 .. Dy-1.
 * psvo_filter_backward_wobs: reverse mode of it with the outputs of psvo_filter_backward (dP, dF, dG (T,B,Dy,N); dmu2, dm0,
 *   dfm0; dsig_q1, dsig_q2, dsig_f, dsig_g (Dy), dsig0, dfsig0) and its m0 / fm0 (sig0 / fsig0) aliasing rule.  Upstream
 *   gradient: dlse (T,B) only (NULL = 0).  ws: psvo_filter_wobs_ws_floats(B, T, N, Dx, Dy) floats (per-sequence sums, then the
 *   (T,B,Dx,N) rows of d mu2).  Every sum has one fixed order and there are no float atomics: a parent particle adds the
 *   gradients of its children in child order, sums over particles are per-lane columns folded in lane / wave order, sums over
 *   sequences in sequence order.  Two runs of the same inputs are bit-identical whatever PSVO_TUNE_DETERMINISTIC is.
 * psvo_mlp_wgrad_wobs: the contract of psvo_mlp_wgrad (grad = [dW1 | db1 | dW2 | db2], keras layout; X [S][Din][L],
 *   dOut [S][Dout][L]; accumulate != 0 adds into grad) for Din <= 4, H in {16,32,64}, 3 <= Dout <= 32.  dW2 = h^T dOut and
 *   dh = dOut W2^T run on v_mfma_f32_16x16x4_f32 over LDS tiles of 64 rows, dW1 / db1 / db2 and the relu mask on the vector
 *   ALU; rows past the end contribute nothing.  partial: psvo_mlp_wgrad_wobs_blocks(S*L) * len(grad) floats, one slice per
 *   workgroup, folded in workgroup order.
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_forward_wobs(const psvo_desc* desc,
                             const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                             const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                             const float* mu2,
                             const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                             const float* obs, const float* eps, const float* u, const int32_t* idx_in,
                             float* X, float* Xanc, float* Fm, float* P1, float* logW, int32_t* idx_out,
                             float* lse, void* stream);
long long psvo_filter_wobs_ws_floats(int B, int T, int N, int Dx, int Dy);
int psvo_filter_backward_wobs(const psvo_desc* desc,
                              const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                              const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                              const float* mu2,
                              const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                              const float* obs, const float* eps,
                              const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                              const int32_t* idx, const float* dlse,
                              float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                              float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                              float* ws, void* stream);
int psvo_mlp_wgrad_wobs_blocks(long long rows);
int psvo_mlp_wgrad_wobs(long long S, int L, int Din, int H, int Dout, const float* X, const float* dOut,
                        const psvo_mlp* w, float* partial, float* grad, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Adaptive resampling on wide observations (added within ABI 6: purely additive).  psvo_filter_forward_wobs /
 * psvo_filter_backward_wobs with the decision of "Adaptive resampling" above, word for word: ESS[t,b] = (sum_n w_n)^2 /
 * sum_n w_n^2 with w_n = exp(logW[t,b,n] - max_n logW[t,b,:]); the sequence resamples at t iff !(ESS[t,b] >= ess_frac * N) (a
 * NaN ESS resamples); the draw is made and written at every step (idx_out, Xanc; idx_in teacher-forces it) and only what step
 * t+1 inherits depends on the decision -- resampled: the drawn ancestor's MLP outputs and the weight -log N; kept: the
 * particle's own and logW[t] - lse[t].  ess_frac, rs_in, rs_out, ess_out and rs mean what they mean there.
 *  forward:  the arguments of psvo_filter_forward_wobs, then ess_frac, rs_in (T,B) int32 or NULL, rs_out (T,B) int32,
 *            ess_out (T,B).  With ess_frac > 1 every output equals psvo_filter_forward_wobs's with resample = 1 bit for bit;
 *            with a tiny ess_frac X, Fm, P1, logW, lse equal its outputs with resample = 0 bit for bit.
 *  reverse:  the arguments of psvo_filter_backward_wobs, then rs (T,B) int32, the forward pass's rs_out.  ws:
 *            psvo_filter_wobs_ws_floats(B, T, N, Dx, Dy) floats, unchanged.  Upstream gradient dlse only: nothing runs behind
 *            an adaptive filter under autograd.  One fixed order for every sum and no float atomics, as
 *            psvo_filter_backward_wobs; a step with rs[t-1] == 0 has no gather to reverse and skips the walk over the children.
 *  Envelope of the wide filter entry points (3 <= Dy <= 32, Dx in {2,3,4}, H in {16,32,64}, N <= 512, one hidden layer,
 *  emission 0 / 1 / 2, every bootstrap / two_q wiring).  Refused before a device is touched, the adaptive contract first:
 *  ess_frac not > 0 (NaN included), desc->resample == 0, NULL rs_out / ess_out / rs -- PSVO_ERR_INVALID; then whatever
 *  psvo_filter_forward_wobs / psvo_filter_backward_wobs refuse, with their statuses.
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_forward_wobs_adaptive(const psvo_desc* desc,
                             const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                             const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                             const float* mu2,
                             const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                             const float* obs, const float* eps, const float* u, const int32_t* idx_in,
                             float* X, float* Xanc, float* Fm, float* P1, float* logW, int32_t* idx_out,
                             float* lse, float ess_frac, const int32_t* rs_in, int32_t* rs_out, float* ess_out, void* stream);
int psvo_filter_backward_wobs_adaptive(const psvo_desc* desc,
                              const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                              const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                              const float* mu2,
                              const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                              const float* obs, const float* eps,
                              const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                              const int32_t* idx, const float* dlse,
                              float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                              float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                              float* ws, const int32_t* rs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Missing observations (added within ABI 6: purely additive).  psvo_filter_forward_wobs / psvo_filter_backward_wobs with one
 * change of meaning: a NaN in obs is an observation that was not made.  There is no mask array -- no further pointer, no
 * further stream from HBM; the observation row carries its own mask.  With o_e = (y_e == y_e):
 *     emission 0 / 1:  log g(y | x) = sum_{e: o_e} [ -1/2 z_e^2 - log sig_g[e] - 1/2 log 2 pi ],   z_e = (y_e - mean_e) / sig_g[e]
 *     emission 2:      log g(y | x) = sum_{e: o_e} [ y_e log lam_e - lam_e - log Gamma(y_e + 1) ]
 *   terms added in the order e = 0 .. Dy-1, the constant with its term; a step with nothing observed has log g = 0 exactly, so
 *   its weights are those of the transition over the proposal.  A NaN never reaches a sum: the term is computed and dropped by
 *   a select (the row is a broadcast, so the choice is the same in every lane; no branch, barrier or store depends on it).
 *   Every other value, +-inf included, is an observation as before.  lse, logW and the ELBO are then a bound on the log-density
 *   of the observed entries; X, Xanc, Fm, idx keep their meaning, so psvo_elbo_filter, psvo_ffbs_smooth and psvo_ffbs_sample
 *   consume the result unchanged.
 *  reverse:  dG[t,b,e,:] of a missing (t,b,e) is WRITTEN as 0 (psvo_mlp_wgrad / psvo_mlp_wgrad_wobs read the row back), and
 *            dsig_g[e] receives nothing from it; an output that is never observed gets exactly zero gradients in W2[:,e], b2[e]
 *            and sig_g[e].  Upstream gradient dlse only.  One fixed order for every sum and no float atomics: two runs are
 *            bit-identical.  ws: psvo_filter_wobs_ws_floats(B, T, N, Dx, Dy) floats, unchanged.
 *  The argument lists are those of psvo_filter_forward_wobs and psvo_filter_backward_wobs.  The weight gradient of MLP_g from
 *  the d G rows is psvo_mlp_wgrad_wobs for Dy >= 3 and the plain psvo_mlp_wgrad for Dy <= 2.
 *  Envelope: 1 <= Dy <= 32 (the widths of the plain kernels included), Dx in {2,3,4}, H in {16,32,64}, N <= 512, one hidden
 *  layer, emission 0 / 1 / 2, every bootstrap / two_q wiring, resampling on or off; anything else is PSVO_ERR_UNSUPPORTED.  A
 *  missing required pointer, B <= 0, T < 2 or N <= 0 is PSVO_ERR_INVALID.  Both come back before a device is touched.  The
 *  existing entry points keep their envelopes: psvo_filter_forward_wobs still refuses Dy < 3, psvo_mlp_wgrad_wobs Dout < 3.
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_forward_wobs_missing(const psvo_desc* desc,
                             const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                             const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                             const float* mu2,
                             const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                             const float* obs, const float* eps, const float* u, const int32_t* idx_in,
                             float* X, float* Xanc, float* Fm, float* P1, float* logW, int32_t* idx_out,
                             float* lse, void* stream);
int psvo_filter_backward_wobs_missing(const psvo_desc* desc,
                              const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                              const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                              const float* mu2,
                              const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                              const float* obs, const float* eps,
                              const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                              const int32_t* idx, const float* dlse,
                              float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                              float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                              float* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exogenous inputs (added within ABI 6: purely additive).  psvo_filter_forward_wobs_missing / psvo_filter_backward_wobs_missing
 * with input-driven transitions.  v (B,T,Di) is data, given and finite.  The first layer of the per-particle networks q1 and f
 * (one network under bootstrap) is W1 (Dx + Di, H), keras layout, applied to concat[x_t, v_t]:
 *     MLP(x_t[n]; v_t) = relu(x_t[n] W1[:Dx] + (b1 + v_t W1[Dx:])) W2 + b2
 *     x_{t+1} ~ f(. | x_t, v_t),   proposal q1(. | x_t, v_t),   Fm[t] = MLP_f(X_t; v_t),   P1[t] = MLP_q1(X_t; v_t)
 *   so v_t drives the step from t to t + 1, and v_{T-1} is read (into Fm[T-1]) but matters only to prediction.  The t = 0 terms
 *   m0 / fm0 are the caller's, evaluated with a zero input.  The emission, q0 and q2 do not see v.
 *   The kernels do not take v: the input's share of the hidden pre-activation does not depend on the particle, and the caller
 *   passes it as hb_q1, hb_f (T,B,H), hb[t,b,:] = v[b,t,:] W1[Dx:] (zero in hidden units beyond the model's width), with the
 *   psvo_mlp structs holding W1[:Dx] (Dx,H).  The effective first-layer bias of step t is b1[k] + hb[t,b,k]: ONE fp32 add per
 *   word, made by the lane that stages it, then used as b1 is; a reference that rounds b1 + hb once and adds x W1[:Dx] to it
 *   follows the kernels exactly, and hb = 0 reproduces the missing-observation pair bit for bit.
 *  forward:  the arguments of psvo_filter_forward_wobs_missing, then hb_q1, hb_f.  hb_q1 is required; hb_f is required unless
 *            desc->bootstrap, where it is ignored.  Same outputs and layouts.
 *  reverse:  the arguments of psvo_filter_backward_wobs_missing, then hb_q1, hb_f; upstream gradient dlse only.  The relu masks
 *            of step t use the bias row of step t.  dP / dF are the rows d MLP_q1 / d MLP_f as always; the gradients of W1[:Dx],
 *            b1, W2, b2 and of hb come from psvo_mlp_wgrad_rowbias below, and d W1[Dx:] = sum_{t,b} v[b,t,:]^T d hb[t,b,:],
 *            d v[b,t,:] = d hb[t,b,:] W1[Dx:]^T are plain matrix products of the caller.
 *  Envelope: that of the missing-observation pair (1 <= Dy <= 32, Dx in {2,3,4}, H in {16,32,64}, N <= 512, one hidden layer,
 *  emission 0 / 1 / 2; anything else PSVO_ERR_UNSUPPORTED; a missing required pointer, B <= 0, T < 2 or N <= 0
 *  PSVO_ERR_INVALID), both before a device is touched.
 *
 * psvo_mlp_wgrad_rowbias: psvo_mlp_wgrad (Din, Dout <= 4, H in {16,32,64}) for a first-layer bias that changes with the segment,
 *   hb (S,H): the hidden layer of segment s is recomputed with b1 + hb[s] (the same single add).  grad = [dW1|db1|dW2|db2] as
 *   before (db1 = sum over all rows of d pre; accumulate applies to grad only); dhb (S,H) = sum_l d pre[s,l,:] is written, never
 *   accumulated.  Orders: a lane adds its rows l = lane, lane + 64, .. in that order, a segment's sum folds the 64 lanes in lane
 *   order; grad folds lanes, then the four waves of a workgroup in wave order, then the workgroups in workgroup order.  No float
 *   atomics: two calls on the same inputs are bit-identical.  partial: psvo_mlp_wgrad_rowbias_blocks(S) * len(grad) floats.
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_forward_wobs_input(const psvo_desc* desc,
                             const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                             const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                             const float* mu2,
                             const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                             const float* obs, const float* eps, const float* u, const int32_t* idx_in,
                             float* X, float* Xanc, float* Fm, float* P1, float* logW, int32_t* idx_out,
                             float* lse, const float* hb_q1, const float* hb_f, void* stream);
int psvo_filter_backward_wobs_input(const psvo_desc* desc,
                              const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                              const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                              const float* mu2,
                              const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                              const float* obs, const float* eps,
                              const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                              const int32_t* idx, const float* dlse,
                              float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                              float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                              float* ws, const float* hb_q1, const float* hb_f, void* stream);
int psvo_mlp_wgrad_rowbias_blocks(long long S);
int psvo_mlp_wgrad_rowbias(long long S, int L, int Din, int H, int Dout, const float* X, const float* dOut,
                           const float* hb, const psvo_mlp* w, float* partial, float* grad, float* dhb,
                           int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exogenous inputs with adaptive resampling (added within ABI 6: purely additive).  The intersection of two sections above and
 * nothing new: psvo_filter_forward_wobs_input / psvo_filter_backward_wobs_input -- the first-layer bias of MLP_q1 / MLP_f at step t
 * is b1 + hb[t,b,:], one fp32 add -- with the decision of psvo_filter_forward_wobs_adaptive, word for word:
 * ESS[t,b] = (sum_n w_n)^2 / sum_n w_n^2 taken from the weights as they are, the sequence inherits the draw iff
 * !(ESS[t,b] >= ess_frac * N) or as rs_in says, and the draw is made and written at every step; a kept particle carries its own
 * means MLP_q1(x_t; v_t), MLP_f(x_t; v_t) and its normalised weight into the next step.
 *  forward:  the arguments of psvo_filter_forward_wobs_adaptive, then hb_q1, hb_f (ahead of stream).  hb = 0 gives the outputs of
 *            psvo_filter_forward_wobs_missing_adaptive bit for bit; ess_frac > 1 those of psvo_filter_forward_wobs_input with
 *            desc->resample = 1; a threshold no ESS falls below gives X, Fm, logW and lse of that call with desc->resample = 0.
 *  reverse:  the arguments of psvo_filter_backward_wobs_adaptive, then hb_q1, hb_f; upstream gradient dlse only; rs (T,B) is a
 *            constant.  dP / dF are the rows d MLP_q1 / d MLP_f; psvo_mlp_wgrad_rowbias turns them into the weight gradients and
 *            d hb, unchanged.
 *  Envelope: that of the input pair (1 <= Dy <= 32, every emission form, T >= 2) with the adaptive contract ahead of it
 *  (ess_frac > 0, desc->resample, rs_out and ess_out / rs: else PSVO_ERR_INVALID).  No EXT form.
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_forward_wobs_input_adaptive(const psvo_desc* desc,
                             const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                             const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                             const float* mu2,
                             const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                             const float* obs, const float* eps, const float* u, const int32_t* idx_in,
                             float* X, float* Xanc, float* Fm, float* P1, float* logW, int32_t* idx_out,
                             float* lse, float ess_frac, const int32_t* rs_in, int32_t* rs_out, float* ess_out,
                             const float* hb_q1, const float* hb_f, void* stream);
int psvo_filter_backward_wobs_input_adaptive(const psvo_desc* desc,
                              const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                              const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                              const float* mu2,
                              const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                              const float* obs, const float* eps,
                              const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                              const int32_t* idx, const float* dlse,
                              float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                              float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                              float* ws, const int32_t* rs, const float* hb_q1, const float* hb_f, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Adaptive resampling on missing observations (added within ABI 6: purely additive).  The intersection of the two sections
 * above and nothing new: psvo_filter_forward_wobs_missing / psvo_filter_backward_wobs_missing -- a NaN in obs is left out of
 * log g, a step with nothing observed has log g = 0 exactly -- with the decision of psvo_filter_forward_wobs_adaptive, word for
 * word: ESS[t,b] = (sum_n w_n)^2 / sum_n w_n^2 taken from the weights as the observed terms left them, the sequence inherits the
 * draw iff !(ESS[t,b] >= ess_frac * N) or as rs_in says, and the draw is made and written at every step.  A step with nothing
 * observed adds no information: in a bootstrap filter without q2 such a step behind a resampled one has ESS = N and is kept.
 *  forward:  the arguments of psvo_filter_forward_wobs_adaptive.  With rs_in all ones the count emission's outputs equal
 *            psvo_filter_forward_wobs_missing's bit for bit; with no NaN in obs they equal psvo_filter_forward_wobs_adaptive's
 *            bit for bit for the count emission and to rounding for the Gaussian forms (the constant travels with each term).
 *  reverse:  the arguments of psvo_filter_backward_wobs_adaptive; the decisions are constants; a missing entry writes dG = 0
 *            and adds nothing to dsig_g.  Upstream gradient dlse only.  One fixed order for every sum and no float atomics:
 *            two runs are bit-identical.  ws: psvo_filter_wobs_ws_floats(B, T, N, Dx, Dy) floats, unchanged.  The weight
 *            gradient of MLP_g is psvo_mlp_wgrad_wobs for Dy >= 3 and the plain psvo_mlp_wgrad for Dy <= 2.
 *  Refused before a device is touched, the adaptive contract first: ess_frac not > 0 (NaN included), desc->resample == 0, NULL
 *  rs_out / ess_out / rs -- PSVO_ERR_INVALID; then the missing pair's envelope with its statuses: 1 <= Dy <= 32, Dx in {2,3,4},
 *  H in {16,32,64}, N <= 512, one hidden layer, emission 0 / 1 / 2 (else PSVO_ERR_UNSUPPORTED); a missing required pointer,
 *  B <= 0, T < 2 or N <= 0 is PSVO_ERR_INVALID.  psvo_filter_forward_wobs_adaptive still refuses Dy < 3.
 * ------------------------------------------------------------------------------------------- */
int psvo_filter_forward_wobs_missing_adaptive(const psvo_desc* desc,
                             const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                             const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                             const float* mu2,
                             const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                             const float* obs, const float* eps, const float* u, const int32_t* idx_in,
                             float* X, float* Xanc, float* Fm, float* P1, float* logW, int32_t* idx_out,
                             float* lse, float ess_frac, const int32_t* rs_in, int32_t* rs_out, float* ess_out, void* stream);
int psvo_filter_backward_wobs_missing_adaptive(const psvo_desc* desc,
                              const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                              const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                              const float* mu2,
                              const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                              const float* obs, const float* eps,
                              const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                              const int32_t* idx, const float* dlse,
                              float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                              float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                              float* ws, const int32_t* rs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PSVO on wide observations: the backward simulation with proposal and its reverse pass for 3 <= Dy <= 32
 * (psvo_amd/csrc/bsim_wobs.hip), and the wide reverse filter with upstream gradients of Fm / logW (added within ABI 6).
 * The Dy <= 2 entry points are unchanged: psvo_bsim_forward, psvo_bsim_backward and psvo_bsim_backward_fold keep answering
 * PSVO_ERR_UNSUPPORTED for Dy = 3, and psvo_filter_backward_wobs keeps its signature and its results bit for bit.
 * Envelope of the two backward-simulation entry points: 3 <= Dy <= 32 (a run-time bound, nothing is instantiated per width),
 * Dx in {2,3,4}, H in {16,32,64}, M in {4,8,16,32}, N <= 512, one hidden layer (desc->layers in {0, 1}), state-independent
 * scales, Gaussian and Poisson emission and the count emission (desc->emission = 2, above).  A missing required pointer, B <= 0, T < 2 or N <= 0 is PSVO_ERR_INVALID whatever the
 * shape; anything else outside the envelope is PSVO_ERR_UNSUPPORTED; both come back before a device is touched.
 *
 * psvo_bsim_forward_wobs: contract, argument list, outputs and layouts of psvo_bsim_forward (bwX, flp, glp, Omega, sel_out,
 *   score and the optional saves lam2_all, om_all, mu1_all), same arithmetic and the same draw rule (sel = the number of CDF
 *   entries <= u * total over the chain's M sub-particles, clamped to M - 1; or teacher-forced sel_in), so that psvo_elbo_bsim
 *   and the host code consume the result unchanged.  Workgroup = 256 / M chains of one sequence, lane = (chain, sub-particle),
 *   persistent over t = T-1 .. 0; the filter term is an online log-sum-exp (log2 domain) over the forward particles in blocks
 *   of 8, j ascending; the emission log-density adds z_e^2 in the order e = 0 .. Dy-1.
 * psvo_bsim_backward_wobs: reverse mode of it, psvo_bsim_backward and psvo_bsim_backward_fold in one call.  Inputs as there;
 *   outputs: the rows xt, dFt (T,B,Dx,N,M), dGt (T,B,Dy,N,M), dmu1 (T,B,Dx,N); the per-chain rows dbmu2_rows (T,B,Dx,N),
 *   dminit_rows, dimean_rows (B,Dx,N); the folded dFm (T,B,Dx,N), dlogW (T,B,N), dlse (T,B) = -sum_n dlogW; the scale
 *   gradients dsig_f, dsig_q1inv, dsig_bq2, dsig_init, disig (Dx), dsig_g (Dy).
 *   ws: psvo_bsim_wobs_ws_floats(B, T, N, M, Dx, Dy) = T B nblk (Dx + 1) N + B nblk (7 Dx + Dy) floats with
 *   nblk = psvo_bsim_wobs_blocks(N, M) = ceil(N / (NT / M)), NT = min(256, 64 ceil(N M / 64)): the per-workgroup partials.
 *   No float atomics; every sum has one fixed order: a pair sum adds the 16 sub-particles of a lane row in lane order, rows by
 *   two swap-adds, waves in wave order, workgroups in workgroup order; sums over a chain's sub-particles are butterflies;
 *   scale sums are per-lane values folded lanes first (DPP scan), then waves, then (sequence, workgroup) rows in order;
 *   d sig_g[e] is one column per lane folded in lane order.  Two runs of the same inputs are bit-identical whatever
 *   PSVO_TUNE_DETERMINISTIC is.
 *   The fold behind the kernel is psvo_bsim_backward_fold's, with its alignment rule: 16-byte accesses when N % 4 == 0 and the
 *   partials carved out of `ws` (at ws and ws + T B nblk Dx N floats), dFm and dlogW are all 16-byte aligned, 4-byte accesses
 *   otherwise, with the same results.
 * psvo_filter_backward_wobs_ext: psvo_filter_backward_wobs with the upstream gradients dFm_ext (T,B,nparts,Dx,N) and
 *   dlogW_ext (T,B,nparts,N) of psvo_filter_backward (NULL = 0; nparts >= 1 when either is given), added in part order.
 *   With both NULL its outputs equal psvo_filter_backward_wobs bit for bit (that entry point forwards with 0, NULL, NULL).
 * ------------------------------------------------------------------------------------------- */
int psvo_bsim_forward_wobs(const psvo_desc* desc,
                           const float* X, const float* Fm, const float* logW, const float* lse,
                           const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                           const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
                           const float* bmu2, const float* minit, const float* sig_init,
                           const float* imean, const float* isig,
                           const float* obs, const float* eps_b, const float* u_b, const int32_t* sel_in,
                           float* bwX, float* flp, float* glp, float* Omega, int32_t* sel_out,
                           float* score,
                           float* lam2_all, float* om_all, float* mu1_all,
                           void* stream);
int psvo_bsim_wobs_blocks(int N, int M);
long long psvo_bsim_wobs_ws_floats(int B, int T, int N, int M, int Dx, int Dy);
int psvo_bsim_backward_wobs(const psvo_desc* desc,
                            const float* Fm, const float* logW, const float* lse,
                            const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                            const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
                            const float* bmu2, const float* minit, const float* sig_init,
                            const float* imean, const float* isig,
                            const float* obs, const float* eps_b,
                            const float* bwX, const int32_t* sel,
                            const float* lam2_all, const float* om_all, const float* mu1_all,
                            const float* dscore,
                            float* xt, float* dFt, float* dGt, float* dmu1,
                            float* dbmu2_rows, float* dminit_rows, float* dimean_rows,
                            float* dFm, float* dlogW, float* dlse,
                            float* dsig_f, float* dsig_g, float* dsig_q1inv, float* dsig_bq2, float* dsig_init,
                            float* disig, float* ws, void* stream);
int psvo_filter_backward_wobs_ext(const psvo_desc* desc,
                                  const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                  const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                                  const float* mu2,
                                  const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                                  const float* obs, const float* eps,
                                  const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                                  const int32_t* idx,
                                  const float* dlse, int nparts, const float* dFm_ext, const float* dlogW_ext,
                                  float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                                  float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                                  float* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PSVO on missing observations (added within ABI 6: purely additive).  The intersection of "Missing observations" and "PSVO on
 * wide observations" above and nothing new (psvo_amd/csrc/bsim_wobs_ms.hip: the text of bsim_wobs.hip compiled a second time).
 * A NaN in obs[t,b,e] is an entry that was not observed: with o_e = (y_e == y_e), log g(y_t | x) is the sum of the observed
 * terms in the order e = 0 .. Dy-1, the constant c_e = -(log sig_g[e] + 1/2 log 2 pi) of a Gaussian term included (an LDS row,
 * filled once); a step with nothing observed has glp == 0 exactly.  The select only feeds the sum: no branch, barrier or store
 * depends on the data.  The proposal-side inputs (bmu2, minit) are the caller's: it computes them from observations with the
 * missing entries set to 0.
 *
 * psvo_bsim_forward_wobs_missing: the argument list, outputs and layouts of psvo_bsim_forward_wobs.  With no NaN in obs the
 *   count emission's outputs equal psvo_bsim_forward_wobs's bit for bit; the Gaussian forms add c_e term by term, not once per
 *   launch, and differ by that rounding.
 * psvo_bsim_backward_wobs_missing: the argument list and outputs of psvo_bsim_backward_wobs.  dGt[t,b,e,:,:] of a missing
 *   (t,b,e) is WRITTEN as 0 (the weight gradient reads the row back) and the d sig_g column of the lane receives nothing: an
 *   output that is never observed has exactly zero gradient in its column of W2, in b2 and in dsig_g.  ws:
 *   psvo_bsim_wobs_ws_floats(B, T, N, M, Dx, Dy) floats with psvo_bsim_wobs_blocks(N, M), unchanged.  The sum orders are those
 *   of psvo_bsim_backward_wobs; two runs are bit-identical.  MLP_g's weight gradient from the d G rows is psvo_mlp_wgrad_wobs
 *   for Dy >= 3 and the plain psvo_mlp_wgrad for Dy <= 2.
 * psvo_filter_backward_wobs_missing_ext: psvo_filter_backward_wobs_missing with the upstream gradients dFm_ext / dlogW_ext /
 *   nparts of psvo_filter_backward_wobs_ext, added in part order.  With both NULL its outputs equal
 *   psvo_filter_backward_wobs_missing's bit for bit; that entry point keeps its signature and its kernels.
 *
 * Envelope of the backward-simulation pair: 1 <= Dy <= 32, Dx in {2,3,4}, H in {16,32,64}, M in {4,8,16,32}, N <= 512, one
 * hidden layer, emission 0 / 1 / 2.  The checks are those of psvo_bsim_forward_wobs / psvo_bsim_backward_wobs in the same
 * order with the same statuses: a bad desc->emission is PSVO_ERR_UNSUPPORTED, then a missing required pointer, B <= 0, T < 2 or
 * N <= 0 is PSVO_ERR_INVALID, then anything else outside the envelope is PSVO_ERR_UNSUPPORTED; all before a device is touched.
 * psvo_filter_backward_wobs_missing_ext has the envelope and statuses of psvo_filter_backward_wobs_missing, and nparts <= 0 with
 * an upstream gradient given is PSVO_ERR_INVALID.  psvo_bsim_forward_wobs / psvo_bsim_backward_wobs still refuse Dy < 3.
 * ------------------------------------------------------------------------------------------- */
int psvo_bsim_forward_wobs_missing(const psvo_desc* desc,
                                   const float* X, const float* Fm, const float* logW, const float* lse,
                                   const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                                   const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
                                   const float* bmu2, const float* minit, const float* sig_init,
                                   const float* imean, const float* isig,
                                   const float* obs, const float* eps_b, const float* u_b, const int32_t* sel_in,
                                   float* bwX, float* flp, float* glp, float* Omega, int32_t* sel_out,
                                   float* score,
                                   float* lam2_all, float* om_all, float* mu1_all,
                                   void* stream);
int psvo_bsim_backward_wobs_missing(const psvo_desc* desc,
                                    const float* Fm, const float* logW, const float* lse,
                                    const psvo_mlp* f, const psvo_mlp* g, const psvo_mlp* q1_inv,
                                    const float* sig_f, const float* sig_g, const float* sig_q1inv, const float* sig_bq2,
                                    const float* bmu2, const float* minit, const float* sig_init,
                                    const float* imean, const float* isig,
                                    const float* obs, const float* eps_b,
                                    const float* bwX, const int32_t* sel,
                                    const float* lam2_all, const float* om_all, const float* mu1_all,
                                    const float* dscore,
                                    float* xt, float* dFt, float* dGt, float* dmu1,
                                    float* dbmu2_rows, float* dminit_rows, float* dimean_rows,
                                    float* dFm, float* dlogW, float* dlse,
                                    float* dsig_f, float* dsig_g, float* dsig_q1inv, float* dsig_bq2, float* dsig_init,
                                    float* disig, float* ws, void* stream);
int psvo_filter_backward_wobs_missing_ext(const psvo_desc* desc,
                                          const psvo_mlp* q1, const psvo_mlp* f, const psvo_mlp* g,
                                          const float* sig_q1, const float* sig_q2, const float* sig_f, const float* sig_g,
                                          const float* mu2,
                                          const float* m0, const float* sig0, const float* fm0, const float* fsig0,
                                          const float* obs, const float* eps,
                                          const float* X, const float* Fm, const float* P1, const float* logW, const float* lse,
                                          const int32_t* idx,
                                          const float* dlse, int nparts, const float* dFm_ext, const float* dlogW_ext,
                                          float* dP, float* dF, float* dG, float* dmu2, float* dm0, float* dfm0,
                                          float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0, float* dfsig0,
                                          float* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One-hidden-layer MLP over plain rows (the hoisted per-(sequence, step) networks q0, q2, BSim_q2,
 * BSim_q_init): tf_mvn.mean of MLP_transformation, reference src/transformation/MLP.py:48-68 as called
 * from src/SMC/SVO.py:80-84,134-138 and src/SMC/PSVO.py:86-87,120-122.
 *   X (R,Din) row-major, out / dOut (R,Dout); Din <= 128, H in {16,32,64}, Dout <= 4.
 *   forward : out = relu(X W1 + b1) W2 + b2.
 *   backward: dX (R,Din) (NULL = not needed) and grad = [dW1 | db1 | dW2 | db2] (keras layout, flat;
 *             accumulate != 0 adds into it); partial: workspace, psvo_rows_mlp_blocks(R) * len(grad) floats.
 * ------------------------------------------------------------------------------------------- */
int psvo_rows_mlp_blocks(long long R);
int psvo_rows_mlp_forward(long long R, int Din, int H, int Dout, const float* X, const psvo_mlp* w,
                          float* out, void* stream);
int psvo_rows_mlp_backward(long long R, int Din, int H, int Dout, const float* X, const float* dOut,
                           const psvo_mlp* w, float* dX, float* partial, float* grad, int accumulate,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Parameter gradients of a one-hidden-layer MLP from per-row output gradients:
 *   grad = [dW1 (Din,H) | db1 (H) | dW2 (H,Dout) | db2 (Dout)]  (keras layout, flat)
 *   X [S][Din][L], dOut [S][Dout][L]: S segments of L rows ((T,B,D,N) tensors: S = T*B, L = N).
 *   partial: workspace, psvo_mlp_wgrad_blocks(S*L) * len(grad) floats.  accumulate != 0 adds into grad.
 * Replaces the dense-layer gradient ops TensorFlow autodiff emits for MLP_transformation
 * (reference src/transformation/MLP.py:48-68).
 * ------------------------------------------------------------------------------------------- */
int psvo_mlp_wgrad_blocks(long long rows);
int psvo_mlp_wgrad(long long S, int L, int Din, int H, int Dout, const float* X, const float* dOut,
                   const psvo_mlp* w, float* partial, float* grad, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same for a per-particle MLP with TWO hidden layers of width H in {32, 64} (psvo_desc.layers == 2;
 * TensorFlow autodiff of MLP_transformation.transform with *_layers = "H,H", reference
 * src/transformation/MLP.py:24-38,50-54; w->Wh, w->bh required):
 *   grad = [dW1 (Din,H) | db1 (H) | dWh (H,H) | dbh (H) | dW2 (H,Dout) | db2 (Dout)]  (keras order hidden_0,
 *   hidden_1, mu_layer; flat).  Rows as psvo_mlp_wgrad.  The three H x H products per row (second-layer
 *   pre-activations, their input gradient, dWh) run on v_mfma_f32_16x16x4_f32 over LDS tiles of 64 rows.
 *   partial: workspace, psvo_mlp2_wgrad_blocks(S*L) * len(grad) floats.  accumulate != 0 adds into grad.
 * ------------------------------------------------------------------------------------------- */
int psvo_mlp2_wgrad_blocks(long long rows);
int psvo_mlp2_wgrad(long long S, int L, int Din, int H, int Dout, const float* X, const float* dOut,
                    const psvo_mlp* w, float* partial, float* grad, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One bidirectional LSTMBlockCell layer over a batch of sequences -- the observation encoder
 * upstream of the particle path.  Replaces one layer of stack_bidirectional_dynamic_rnn over
 * tf.contrib.rnn.LSTMBlockCell (reference src/SMC/SVO.py:337-341, src/model.py:164-176).
 *   x (B,T,Din); W_fw / W_bw (Din+Dh, 4Dh) TF kernels, gate order (i, j, f, o); b_* (4Dh);
 *   forget_bias = 1.  out (B,T,2Dh) = concat(forward h, backward h).
 *   cs (2,B,T,Dh) cell states and gates (2,B,T,4Dh) activated gates are optional (NULL) saves
 *   for back-propagation through time.  Dh in {8,16,32,64}, Din <= 128.
 * ------------------------------------------------------------------------------------------- */
int psvo_bilstm_forward(int B, int T, int Din, int Dh, const float* x,
                        const float* W_fw, const float* b_fw, const float* W_bw, const float* b_bw,
                        float* out, float* cs, float* gates, void* stream);

/* Back-propagation through time of psvo_bilstm_forward (needs its cs / gates saves).
 *   dout (B,T,2Dh) = d loss / d out.  Outputs: dx_part (2,B,T,Din) per-direction input gradients
 *   (sum over axis 0), dW_part (B,2,Din+Dh,4Dh) and db_part (B,2,4Dh) per-sequence weight-gradient
 *   partials (sum over axis 0; index 0 = forward direction, 1 = backward). */
int psvo_bilstm_backward(int B, int T, int Din, int Dh, const float* x,
                         const float* W_fw, const float* W_bw,
                         const float* out, const float* cs, const float* gates, const float* dout,
                         float* dx_part, float* dW_part, float* db_part, void* stream);

/* Folds the per-sequence partials of psvo_bilstm_backward into the two cells' gradients, one launch, fixed order:
 *   g_fw / g_bw = [kernel (Din+Dh, 4Dh) | bias (4Dh)] of the forward / backward cell; accumulate != 0 adds into them. */
int psvo_bilstm_wgrad_fold(int B, int Din, int Dh, const float* dW_part, const float* db_part,
                           float* g_fw, float* g_bw, int accumulate, void* stream);

/* Fused Adam update of one flat fp32 parameter vector: tf.train.AdamOptimizer(lr).minimize(-log_ZSMC)
 * of the reference (src/trainer.py:115-118), TF 1.12 epsilon-hat form.  `step` counts from 1;
 * `grad_scale` multiplies the gradient first (-1/world_size for a summed all-reduce of d log_ZSMC). */
int psvo_adam_step(float* params, const float* grads, float* m, float* v, long long n, float lr,
                   float beta1, float beta2, float eps, long long step, float grad_scale, void* stream);

/* Guarded Adam step: clip the gradient by its global L2 norm and / or leave the step out when that norm is not finite, decided
 * on the device (two launches, no atomics, no allocation, no host read; every sum in a fixed order, so bit-reproducible).
 *
 * psvo_grad_norm_blocks(n) = G, the number of partial sums: min(256, ceil(n / 4096)), at least 1; a function of n alone.
 * psvo_grad_sumsq: workgroup k < G writes partial[k] = sum of grads[i]^2 over its slice i in [k S, min(n, (k + 1) S)),
 *   S = ceil(n / G) rounded up to a multiple of 4.  Accumulated in double (the product of two floats is exact there and
 *   the sum cannot overflow); a NaN or an infinity among the entries propagates into its slice's sum.
 * psvo_adam_step_guarded: every workgroup folds partial[0 .. G) in one fixed order and forms
 *       norm = |grad_scale| * sqrt(sum)        -- the L2 norm of the gradient Adam sees (after the 1/world_size), then
 *     norm not finite and skip_nonfinite != 0:  params, m and v are not written; state[2] and state[3] count the step;
 *     else clip_norm > 0 and norm > clip_norm:  g_i = (grads_i * grad_scale) * (float)(clip_norm / norm); state[1] counts it;
 *     else:                                     exactly psvo_adam_step, bit for bit (a factor of 1 is never multiplied in).
 *   (An infinite norm with skip_nonfinite == 0 and clip_norm > 0 takes the second row: the factor is 0.)
 *   lr_t is computed on the host from `step` exactly as in psvo_adam_step, and the caller advances `step` on EVERY call, a
 *   skipped one included: the unguarded case stays bit-identical to psvo_adam_step and host and device can never disagree
 *   about a count.  The price: after a skip the bias correction is marginally too small (lr_t as if one more step had been
 *   averaged in), which matters only during the first few thousand steps.
 *   state[8] (doubles: exact for counts up to 2^53) belongs to the caller, who zeroes it once; lane 0 of workgroup 0 updates it
 *   with ordinary stores:  [0] steps applied (clipped ones included), [1] steps clipped, [2] steps skipped, [3] steps
 *   skipped in a row up to now (0 after an applied step), [4] norm of the last call, [5] largest finite norm so far,
 *   [6], [7] reserved.  [0] + [2] = number of calls.
 *   `partial` must be the G sums psvo_grad_sumsq wrote for the same grads and n on the same stream.
 * PSVO_ERR_INVALID before any launch: a null pointer (stream excepted), n <= 0, step <= 0, clip_norm < 0 or not finite. */
int psvo_grad_norm_blocks(long long n);
int psvo_grad_sumsq(const float* grads, long long n, double* partial, void* stream);
int psvo_adam_step_guarded(float* params, const float* grads, float* m, float* v, long long n, float lr,
                           float beta1, float beta2, float eps, long long step, float grad_scale, float clip_norm,
                           int skip_nonfinite, const double* partial, double* state, void* stream);

/* out[p] (+)= sum_{r < nrows} part[r * stride + p], p < n: folds per-sequence / per-workgroup partial
 * gradients straight into the flat gradient buffer (deterministic, no atomics). */
int psvo_reduce_rows(const float* part, int nrows, long long stride, int n, float* out, int accumulate,
                     void* stream);

/* Scale vectors of all distributions at once: sigma = max(softplus(raw), min), NaN -> 0 first
 * (tf_mvn.get_sigma, reference src/distribution/mvn.py:80-90) and its gradient
 * graw (+)= dsig * sigmoid(raw) * [softplus(raw) >= min]. */
int psvo_sigma_forward(const float* raw, const float* mins, float* sig, int n, void* stream);
int psvo_sigma_backward(const float* raw, const float* mins, const float* dsig, float* graw, int n,
                        int accumulate, void* stream);

/* Diagnostic: runs the DPP / permlane cross-lane primitives the kernels are built on over one
 * wavefront of input (64 floats) and writes 9 x 64 results (xor 1..32, inclusive scan, sum, max). */
/* ---------------------------------------------------------------------------------------------
 * Dense layers over plain rows on v_mfma_f32_16x16x4_f32 (exact f32): the hoisted networks q0, q2, BSim_q2, BSim_q_init
 * (reference src/transformation/MLP.py:24-68) when they have more than one hidden layer or exceed psvo_rows_mlp_*'s
 * widths (Din <= 4096, Dout <= 4096 here).  Rows X (R, Din) row-major, W (Din, Dout) keras layout, b (Dout).
 *   forward : Y = relu ? max(X W + b, 0) : X W + b
 *   backward: dZ = relu ? dY * [Y > 0] : dY;  dX = dZ W^T (R, Din; may be null);  grad = [dW (Din, Dout) | db (Dout)],
 *             accumulated into `grad` when `accumulate`.  partial: psvo_dense_wgrad_slices(R) * (Din + 1) * Dout floats.
 * ------------------------------------------------------------------------------------------- */
int psvo_dense_wgrad_slices(long long R);
int psvo_dense_forward(long long R, int Din, int Dout, const float* X, const float* W, const float* b, int relu,
                       float* Y, void* stream);
int psvo_dense_backward(long long R, int Din, int Dout, const float* X, const float* Y, const float* dY, const float* W,
                        int relu, float* dX, float* partial, float* grad, int accumulate, void* stream);

/* Measurement aid: a one-thread launch that stores the device's constant-rate wall clock (100 MHz) into *slot when the
 * stream reaches it.  Captured into a hipGraph beside the real launches it gives the timeline of a REPLAYED step, which
 * HIP events cannot (event records inside a capture cannot be timed on ROCm) -- tools/replay_timeline.py. */
int psvo_debug_stamp(unsigned long long* slot, void* stream);

int psvo_selftest_lanes(const float* in64, float* out576, void* stream);
/* second self-test: swap-add stages over lane bits 5 / 4, 16-lane row sum, and the operand / accumulator layout of
 * v_mfma_f32_16x16x4_f32 as bsim_bwd2 uses it.  in: 3 x 64 floats (lo, hi, extra); out: 5 x 64 floats
 * (swap_add32, swap_add16, row_sum16, mfma D register 0, mfma D register 1). */
int psvo_selftest_lanes2(const float* in192, float* out320, void* stream);

/* Per-sequence ELBO reductions (no batch mean: the caller averages, so a batch shard can be
 * all-reduced).  filter: out[b] = sum_t lse[t,b] (SVO.compute_log_ZSMC, SVO.py:302-311);
 * bsim: out[b] = logsumexp_n score[b,n] - log N (PSVO.compute_log_ZSMC, PSVO.py:52-67). */
int psvo_elbo_filter(const psvo_desc* desc, const float* lse, float* out, void* stream);
int psvo_elbo_bsim(const psvo_desc* desc, const float* score, float* out, void* stream);

/* The PSVO training objective in one launch and its reverse: out[0] = mean_b psvo_elbo_bsim[b]
 * (PSVO.py:52-67 including the reduce_mean), dscore[b,n] = dz[0] / B * softmax_n(score[b,:]).
 * B is the local batch: a batch shard differentiates its own mean and the gradient all-reduce averages the shards. */
int psvo_elbo_bsim_mean(const psvo_desc* desc, const float* score, float* out, void* stream);
int psvo_elbo_bsim_mean_backward(const psvo_desc* desc, const float* score, const float* dz, float* dscore,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PSVO_HIP_H */
