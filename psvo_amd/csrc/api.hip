// Small entry points of the C ABI: version/status strings and the per-sequence ELBO reductions; and the small kernels that
// several units launch behind their own (row sum, partial folds, the finalize steps of the reverse passes: common.h).
#include "common.h"

namespace psvo {

// out[b] = sum_t lse[t, b]   (SVO.compute_log_ZSMC before the batch mean, reference SVO.py:302-311)
__global__ void elbo_filter_kernel(const float* __restrict__ lse, float* __restrict__ out, int T, int B) {
    const int b = blockIdx.x;
    float acc = 0.f;
    for (int t = threadIdx.x; t < T; t += 64) acc += lse[(size_t)t * B + b];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) out[b] = acc;
}

// out[b] = logsumexp_n score[b, n] - log N   (PSVO.compute_log_ZSMC, reference PSVO.py:52-67)
__global__ void elbo_bsim_kernel(const float* __restrict__ score, float* __restrict__ out, int N) {
    const int b = blockIdx.x;
    const float ninf = -__builtin_huge_valf();
    float mx = ninf;
    for (int n = threadIdx.x; n < N; n += 64) mx = fmaxf(mx, score[(size_t)b * N + n]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int n = threadIdx.x; n < N; n += 64) s += expf(score[(size_t)b * N + n] - mx);
    s = wave_sum(s);
    if (threadIdx.x == 0) out[b] = mx + logf(s) - logf((float)N);
}

// out[0] = mean_b [ logsumexp_n score[b, n] - log N ]: the training objective in one launch
// (one workgroup of 4 waves, sequences strided over the waves, fixed summation order)
__global__ void __launch_bounds__(256) elbo_bsim_mean_kernel(const float* __restrict__ score, float* __restrict__ out,
                                                             int B, int N) {
    __shared__ float part[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float ninf = -__builtin_huge_valf();
    float acc = 0.f;
    for (int b = wave; b < B; b += 4) {
        float mx = ninf;
        for (int n = lane; n < N; n += 64) mx = fmaxf(mx, score[(size_t)b * N + n]);
        mx = wave_max(mx);
        float s = 0.f;
        for (int n = lane; n < N; n += 64) s += expf(score[(size_t)b * N + n] - mx);
        s = wave_sum(s);
        acc += mx + logf(s);
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (part[0] + part[1] + part[2] + part[3]) / (float)B - logf((float)N);
}

// dscore[b, n] = dz[0] / B * softmax_n(score[b, :])   (reverse of elbo_bsim_mean_kernel)
__global__ void elbo_bsim_mean_bwd_kernel(const float* __restrict__ score, const float* __restrict__ dz,
                                          float* __restrict__ dscore, int B, int N) {
    const int b = blockIdx.x;
    const float ninf = -__builtin_huge_valf();
    float mx = ninf;
    for (int n = threadIdx.x; n < N; n += 64) mx = fmaxf(mx, score[(size_t)b * N + n]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int n = threadIdx.x; n < N; n += 64) s += expf(score[(size_t)b * N + n] - mx);
    s = wave_sum(s);
    const float a = dz[0] / ((float)B * s);
    for (int n = threadIdx.x; n < N; n += 64) dscore[(size_t)b * N + n] = a * expf(score[(size_t)b * N + n] - mx);
}

}  // namespace psvo

namespace psvo {
thread_local hipError_t g_last_hip_error = hipSuccess;
}

extern "C" int psvo_abi_version(void) { return PSVO_ABI_VERSION; }

extern "C" const char* psvo_last_hip_error(void) { return hipGetErrorString(psvo::g_last_hip_error); }

extern "C" const char* psvo_status_string(int status) {
    switch (status) {
        case PSVO_OK: return "ok";
        case PSVO_ERR_INVALID: return "invalid argument (null pointer, non-positive size or inconsistent descriptor)";
        case PSVO_ERR_UNSUPPORTED: return "unsupported configuration (Dx/Dy/H/M/N outside the instantiated kernel set)";
        case PSVO_ERR_HIP: return "HIP runtime error at kernel launch";
        default: return "unknown status";
    }
}

extern "C" int psvo_elbo_filter(const psvo_desc* desc, const float* lse, float* out, void* stream) {
    if (!desc || !lse || !out || desc->B <= 0 || desc->T <= 0) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    hipLaunchKernelGGL(psvo::elbo_filter_kernel, dim3(desc->B), dim3(64), 0, static_cast<hipStream_t>(stream), lse,
                       out, desc->T, desc->B);
    return psvo::launch_status();
}

extern "C" int psvo_elbo_bsim(const psvo_desc* desc, const float* score, float* out, void* stream) {
    if (!desc || !score || !out || desc->B <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    hipLaunchKernelGGL(psvo::elbo_bsim_kernel, dim3(desc->B), dim3(64), 0, static_cast<hipStream_t>(stream), score,
                       out, desc->N);
    return psvo::launch_status();
}

extern "C" int psvo_elbo_bsim_mean(const psvo_desc* desc, const float* score, float* out, void* stream) {
    if (!desc || !score || !out || desc->B <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    hipLaunchKernelGGL(psvo::elbo_bsim_mean_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), score,
                       out, desc->B, desc->N);
    return psvo::launch_status();
}

extern "C" int psvo_elbo_bsim_mean_backward(const psvo_desc* desc, const float* score, const float* dz,
                                            float* dscore, void* stream) {
    if (!desc || !score || !dz || !dscore || desc->B <= 0 || desc->N <= 0) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    hipLaunchKernelGGL(psvo::elbo_bsim_mean_bwd_kernel, dim3(desc->B), dim3(64), 0, static_cast<hipStream_t>(stream),
                       score, dz, dscore, desc->B, desc->N);
    return psvo::launch_status();
}

// ---------------------------------------------------------------------------------------------
// small host-overhead killers: at C* the persistent kernels leave ~1 ms of a training step to
// ~300 tiny launches, so groups of them are fused here.
// ---------------------------------------------------------------------------------------------
namespace psvo {

// out[p] (+)= sum_r part[r * stride + p]   (one wave per output element, fixed order)
__global__ void reduce_rows_kernel(const float* __restrict__ part, int nrows, long long stride, int n,
                                   float* __restrict__ out, int accumulate) {
    const int p = blockIdx.x;
    float s = 0.f;
    for (int r = threadIdx.x; r < nrows; r += 64) s += part[(size_t)r * stride + p];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[p] = accumulate ? out[p] + s : s;
}
void launch_reduce_rows(const float* part, int nrows, long long stride, int n, float* out, int accumulate, hipStream_t stream) {
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(n), dim3(64), 0, stream, part, nrows, stride, n, out, accumulate);
}

// out[r] = sum_l in[r * L + l]: one wave per row, lanes stride over the row and fold with the DPP scan
__global__ void __launch_bounds__(256) row_sum_kernel(const float* __restrict__ in, long long rows, int L,
                                                      float* __restrict__ out) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int l = lane; l < L; l += 64) s += in[r * L + l];
    s = wave_sum(s);
    if (lane == 0) out[r] = s;
}
void launch_row_sum(const float* in, long long rows, int L, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(row_sum_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, in, rows, L, out);
}

// sacc[b][i] = sum_t part[t][b][i]: one wave per (b, i) strides over t and sums its lanes in a fixed order
__global__ void __launch_bounds__(256) step_fold_kernel(const float* __restrict__ part, int T, int B, int NACC,
                                                        float* __restrict__ sacc) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < NACC; i += 4) {
        float v = 0.f;
        for (int t = lane; t < T; t += 64) v += part[((size_t)t * B + b) * NACC + i];
        v = wave_sum(v);
        if (lane == 0) sacc[(size_t)b * NACC + i] = v;
    }
}
void launch_step_fold(const float* part, int T, int B, int nacc, float* sacc, hipStream_t stream) {
    hipLaunchKernelGGL(step_fold_kernel, dim3(B), dim3(256), 0, stream, part, T, B, nacc, sacc);
}

// Filter reverse passes: fold the (B, 10 Dx + Dy) sums into gradients of the scale vectors, sequences in order.
//   two_q: the product-of-Gaussians step (common.h: pog_scale_grad), sig_q2 collecting both sets;  else: d s1 = Sc
template <int DX>
__global__ void filter_bwd_finalize(const float* __restrict__ sacc, int B, int Dy, int two_q, int bootstrap,
                                    const float* sig_q1, const float* sig_q2, const float* sig0, int same0,
                                    float* dsig_q1, float* dsig_q2, float* dsig_f, float* dsig_g, float* dsig0,
                                    float* dfsig0) {
    using AC = FAcc<DX>;
    const int NACC = AC::kSg + Dy;
    // one lane per slot: its total is the serial sum over the sequences, in order; the Dx lanes below take them from LDS
    // (with the ten sums of a dimension walked by its own lane the filter-only step measured 1 % longer:
    //  profiles/shared_reverse_helpers.md)
    __shared__ float tot[10 * DX + 32];
    for (int i = threadIdx.x; i < NACC; i += 64) {
        float v = 0.f;
        for (int b = 0; b < B; ++b) v += sacc[(size_t)b * NACC + i];
        tot[i] = v;
    }
    __syncthreads();
    const int d = threadIdx.x;
    if (d < DX) {
        float ds2 = 0.f;
        for (int set = 0; set < 2; ++set) {  // set 0: t = 0 (sig0), set 1: t >= 1 (sig_q1)
            const int P = set * AC::kSet;
            const float s1 = set ? sig_q1[d] : sig0[d];
            float ds1;
            if (two_q) {
                float d2;
                pog_scale_grad(s1, sig_q2[d], tot[P + AC::kSc + d], tot[P + AC::kSmm1 + d], tot[P + AC::kSmb + d],
                               tot[P + AC::kSmm + d], ds1, d2);
                ds2 += d2;
            } else {
                ds1 = tot[P + AC::kSc + d];
            }
            const float dfs = tot[P + AC::kSfs + d];
            if (set) {
                dsig_q1[d] = ds1 + (bootstrap ? dfs : 0.f);
                dsig_f[d] = bootstrap ? 0.f : dfs;
            } else {
                dsig0[d] = same0 ? ds1 + dfs : ds1;      // (fsig0 aliasing sig0: the sum, as for m0 / fm0)
                dfsig0[d] = same0 ? 0.f : dfs;
            }
        }
        dsig_q2[d] = ds2;
    }
    if (d < Dy) dsig_g[d] = tot[AC::kSg + d];
}
int launch_filter_bwd_finalize(int Dx, const FilterFinalizeArgs& a, hipStream_t stream) {
    return pick_dx(Dx, [&](auto dx) {
        hipLaunchKernelGGL((filter_bwd_finalize<dx()>), dim3(1), dim3(64), 0, stream, a.sacc, a.B, a.Dy, a.two_q,
                           a.bootstrap, a.sig_q1, a.sig_q2, a.sig0, a.same0, a.dsig_q1, a.dsig_q2, a.dsig_f, a.dsig_g,
                           a.dsig0, a.dfsig0);
        return PSVO_OK;
    });
}

// Backward-simulation reverse passes, ONE launch behind the reverse kernel: blocks [0, nfold) add the per-workgroup partials
// of d Fm / d logW (what the filter's reverse pass waits for) in workgroup order; blocks [nfold, gridDim.x - 1) form d lse;
// the last block folds the (rows, 7 Dx + Dy) partial sums, rows in (sequence, workgroup) order, into the scale gradients.
// VEC4: four outputs per thread with 16-byte accesses (the launcher sized the grid for it and checked N % 4 == 0 and the
// alignment of the four arrays); every output adds its workgroups in the same order either way.
template <int DX>
__global__ void __launch_bounds__(256) bsim_bwd_fold_finalize(
    const float* __restrict__ dFm_part, const float* __restrict__ dlogW_part, long long TB, int nblk, int N, int Dy,
    float* __restrict__ dFm, float* __restrict__ dlogW, const float* __restrict__ sacc, int rows, const float* sig_q1inv,
    const float* sig_bq2, float* dsig_f, float* dsig_g, float* dsig_q1inv, float* dsig_bq2, float* dsig_init,
    float* disig, float* __restrict__ dlse, unsigned nfold, int vec4) {
    using AC = BAcc<DX>;
    if (blockIdx.x >= nfold && blockIdx.x + 1 < gridDim.x) {
        // d lse[t, b] = -sum_j d logW^[t, b, j]: the normaliser's share of the filter term's gradient (W^ = logW - lse).  It is
        // zero analytically (sum_j d W^_j = sum_m d Lambda_m = 0 per chain) and ~1e-7 of the terms in fp32; TF's autodiff --
        // like any autodiff of the reference's graph -- carries it, and it is what keeps the filter's reverse pass
        // well-conditioned when the forward particles have left the data range (the softmax-weighted subtraction in
        // psvo_filter_backward then cancels the common part of d logW_j exactly instead of to 1e-7: measured on
        // tests/golden/fhn_illconditioned_state.npz, the emission network's gradient error drops 100 x to the fp32 oracle's).
        // One wave per (t, b) row, straight from the per-workgroup partials, concurrently with the fold blocks.
        const long long tb = (long long)(blockIdx.x - nfold) * 4 + (threadIdx.x >> 6);
        if (tb < TB) {
            const float* p = dlogW_part + tb * nblk * N;
            float v = 0.f;
            for (int i = threadIdx.x & 63; i < nblk * N; i += 64) v += p[i];
            v = wave_sum(v);
            if ((threadIdx.x & 63) == 0) dlse[tb] = -v;
        }
        return;
    }
    if (blockIdx.x + 1 < gridDim.x) {
        const long long rowF = (long long)DX * N, nF = TB * rowF, nW = TB * N;
        long long e = (long long)blockIdx.x * 256 + threadIdx.x;
        if (vec4) {
            e *= 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < nF) {
                const long long tb = e / rowF;
                const float* p = dFm_part + tb * nblk * rowF + (e - tb * rowF);
                for (int k = 0; k < nblk; ++k) {
                    const float4 q = *reinterpret_cast<const float4*>(p + k * rowF);
                    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                }
                *reinterpret_cast<float4*>(dFm + e) = v;
            } else if (e < nF + nW) {
                e -= nF;
                const long long tb = e / N;
                const float* p = dlogW_part + tb * nblk * N + (e - tb * N);
                for (int k = 0; k < nblk; ++k) {
                    const float4 q = *reinterpret_cast<const float4*>(p + (long long)k * N);
                    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                }
                *reinterpret_cast<float4*>(dlogW + e) = v;
            }
            return;
        }
        if (e < nF) {            // d Fm (T, B, Dx, N) from (T, B, nblk, Dx, N)
            const long long tb = e / rowF;
            const float* p = dFm_part + tb * nblk * rowF + (e - tb * rowF);
            float v = 0.f;
            for (int k = 0; k < nblk; ++k) v += p[k * rowF];
            dFm[e] = v;
        } else if (e < nF + nW) {   // d logW (T, B, N) from (T, B, nblk, N)
            e -= nF;
            const long long tb = e / N;
            const float* p = dlogW_part + tb * nblk * N + (e - tb * N);
            float v = 0.f;
            for (int k = 0; k < nblk; ++k) v += p[(long long)k * N];
            dlogW[e] = v;
        }
        return;
    }
    __shared__ float tot[7 * DX + 32];
    const int NACC = AC::kSg + Dy;
    const int d = threadIdx.x, lane = d & 63, wave = d >> 6;
    for (int k = wave; k < NACC; k += 4) {  // lanes stride over the (sequence, workgroup) rows
        float v = 0.f;
        for (int r = lane; r < rows; r += 64) v += sacc[(size_t)r * NACC + k];
        v = wave_sum(v);
        if (lane == 0) tot[k] = v;
    }
    __syncthreads();
    if (d < DX) {
        pog_scale_grad(sig_q1inv[d], sig_bq2[d], tot[AC::kSc + d], tot[AC::kSmm1 + d], tot[AC::kSmb + d], tot[AC::kSmm + d],
                       dsig_q1inv[d], dsig_bq2[d]);
        dsig_f[d] = tot[AC::kSf + d];
        dsig_init[d] = tot[AC::kSinit + d];
        disig[d] = tot[AC::kSiota + d];
    }
    if (d < Dy) dsig_g[d] = tot[AC::kSg + d];
}
int launch_bsim_bwd_fold_finalize(int Dx, const BsimFoldArgs& a, hipStream_t stream) {
    // the 16-byte path only where it can be seen to be sound: whole float4s per row and all four arrays aligned
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a.dFm_part) | reinterpret_cast<uintptr_t>(a.dlogW_part) |
                           reinterpret_cast<uintptr_t>(a.dFm) | reinterpret_cast<uintptr_t>(a.dlogW);
    const int vec4 = (a.N & 3) == 0 && (bits & 15) == 0;
    const long long TB = (long long)a.T * a.B;
    const long long n = TB * (Dx + 1) * a.N / (vec4 ? 4 : 1);
    const unsigned nfold = (unsigned)((n + 255) / 256), nrow = a.dlse ? (unsigned)((TB + 3) / 4) : 0u;
    return pick_dx(Dx, [&](auto dx) {
        hipLaunchKernelGGL((bsim_bwd_fold_finalize<dx()>), dim3(nfold + nrow + 1), dim3(256), 0, stream, a.dFm_part,
                           a.dlogW_part, TB, a.nblk, a.N, a.Dy, a.dFm, a.dlogW, a.sacc, a.rows, a.sig_q1inv, a.sig_bq2,
                           a.dsig_f, a.dsig_g, a.dsig_q1inv, a.dsig_bq2, a.dsig_init, a.disig, a.dlse, nfold, vec4);
        return PSVO_OK;
    });
}

// sigma = max(softplus(raw), min) with NaN -> 0 first (reference src/distribution/mvn.py:80-90)
__global__ void sigma_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ mins, float* __restrict__ sig,
                                 int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float r = raw[i];
    float s = r > 20.f ? r : log1pf(expf(r));   // softplus (same threshold as torch / TF for fp32)
    if (s != s) s = 0.f;
    sig[i] = fmaxf(s, mins[i]);
}

// graw (+)= dsig * sigmoid(raw) * [softplus(raw) >= min]
__global__ void sigma_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ mins,
                                 const float* __restrict__ dsig, float* __restrict__ graw, int n, int accumulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float r = raw[i];
    const float s = r > 20.f ? r : log1pf(expf(r));
    const float g = (s == s && s >= mins[i]) ? dsig[i] / (1.f + expf(-r)) : 0.f;
    graw[i] = accumulate ? graw[i] + g : g;
}

}  // namespace psvo

extern "C" int psvo_reduce_rows(const float* part, int nrows, long long stride, int n, float* out, int accumulate,
                                void* stream) {
    if (!part || !out || nrows <= 0 || n <= 0) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    psvo::launch_reduce_rows(part, nrows, stride, n, out, accumulate, static_cast<hipStream_t>(stream));
    return psvo::launch_status();
}

extern "C" int psvo_sigma_forward(const float* raw, const float* mins, float* sig, int n, void* stream) {
    if (!raw || !mins || !sig || n <= 0) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    hipLaunchKernelGGL(psvo::sigma_fwd_kernel, dim3((n + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), raw,
                       mins, sig, n);
    return psvo::launch_status();
}

extern "C" int psvo_sigma_backward(const float* raw, const float* mins, const float* dsig, float* graw, int n,
                                   int accumulate, void* stream) {
    if (!raw || !mins || !dsig || !graw || n <= 0) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    hipLaunchKernelGGL(psvo::sigma_bwd_kernel, dim3((n + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), raw,
                       mins, dsig, graw, n, accumulate);
    return psvo::launch_status();
}


// ---------------------------------------------------------------------------------------------
// on-device self-test of the cross-lane primitives in common.h (tests/test_gpu_parity.py)
// out rows: xor 1,2,4,8,16,32 | inclusive scan | sum | max   -> 9 x 64 floats
// ---------------------------------------------------------------------------------------------
namespace psvo {
__global__ void lane_selftest_kernel(const float* __restrict__ in, float* __restrict__ out) {
    const int l = threadIdx.x;
    const float v = in[l];
    out[0 * 64 + l] = xor_lane<1>(v);
    out[1 * 64 + l] = xor_lane<2>(v);
    out[2 * 64 + l] = xor_lane<4>(v);
    out[3 * 64 + l] = xor_lane<8>(v);
    out[4 * 64 + l] = xor_lane<16>(v);
    out[5 * 64 + l] = xor_lane<32>(v);
    out[6 * 64 + l] = wave_incl_scan(v, l);
    out[7 * 64 + l] = wave_sum(v);
    out[8 * 64 + l] = wave_max(v);
}
}  // namespace psvo

#include "bsim_bwd2_impl.h"
namespace psvo {
__global__ void lane_selftest2_kernel(const float* __restrict__ in, float* __restrict__ out) {
    const int l = threadIdx.x;
    const float lo = in[l], hi = in[64 + l], ex = in[128 + l];
    out[0 * 64 + l] = swap_add32(lo, hi);
    out[1 * 64 + l] = swap_add16(lo, hi);
    out[2 * 64 + l] = row_sum16(lo);
    // D[i][j] = sum_k A[i][k] B[k][j], A operand: lane l holds A[l & 15][l >> 4]; B: B[l >> 4][l & 15];
    // D: lane l holds rows 4 (l >> 4) + reg of column l & 15
    f4v acc = f4v{0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(lo, hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ex, hi, acc, 0, 0, 0);
    out[3 * 64 + l] = acc[0];
    out[4 * 64 + l] = acc[1];
}
}  // namespace psvo

namespace psvo {
__global__ void stamp_kernel(unsigned long long* slot) { *slot = wall_clock64(); }
}  // namespace psvo

extern "C" int psvo_debug_stamp(unsigned long long* slot, void* stream) {
    if (!slot) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    hipLaunchKernelGGL(psvo::stamp_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), slot);
    return psvo::launch_status();
}

extern "C" int psvo_selftest_lanes2(const float* in192, float* out320, void* stream) {
    if (!in192 || !out320) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    hipLaunchKernelGGL(psvo::lane_selftest2_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), in192, out320);
    return psvo::launch_status();
}

extern "C" int psvo_selftest_lanes(const float* in64, float* out576, void* stream) {
    if (!in64 || !out576) return PSVO_ERR_INVALID;
    psvo::clear_hip_error();
    hipLaunchKernelGGL(psvo::lane_selftest_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), in64, out576);
    return psvo::launch_status();
}
