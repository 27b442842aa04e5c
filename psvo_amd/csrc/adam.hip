// Fused Adam step on one flat fp32 parameter vector (every trainable variable of the model lives
// in a single contiguous buffer so that the data-parallel gradient all-reduce and the optimizer
// are one collective and one launch).  Restates tf.train.AdamOptimizer(lr) as used by the
// reference (src/trainer.py:115-118; TF 1.12 "epsilon-hat" form):
//     lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
//     theta -= lr_t * m / (sqrt(v) + eps)
// The reference minimises -log_ZSMC; `grad_scale` folds that sign and the 1/world_size of the
// all-reduced (summed) gradient.
//
// The guarded step (psvo_grad_sumsq + psvo_adam_step_guarded, contract in include/psvo_hip.h) clips that gradient by its global
// norm and leaves a step with a non-finite norm out, without the host ever reading the norm: launch 1 writes G per-workgroup
// sums of squares, launch 2 has EVERY workgroup fold them in the same order (so all agree on the decision) and then runs the
// update above.  All sums are double and tree-shaped in a fixed order: no atomics, bit-reproducible.
#include <cmath>

#include "common.h"

namespace psvo {
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long long n, float lr_t, float b1, float b2, float eps,
                            float grad_scale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i] * grad_scale;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
}

constexpr int kNormThreads = 256;        // workgroup of both guard kernels (the fold below is written for exactly four waves)
constexpr int kNormMaxBlocks = 256;      // G <= one partial per lane of the folding workgroup
constexpr long long kNormSlice = 4096;   // floats per workgroup while G < 256: 16 per lane, four 16-byte loads

inline int norm_blocks(long long n) {
    const long long g = (n + kNormSlice - 1) / kNormSlice;
    return (int)(g < 1 ? 1 : g > kNormMaxBlocks ? kNormMaxBlocks : g);
}
inline long long norm_slice(long long n, int G) { return ((n + G - 1) / G + 3) / 4 * 4; }

// Sum of one double per lane over the 256 lanes of the workgroup, the same value in every lane: xor butterfly inside each wave
// (both partners add the same two numbers, so all lanes of a wave hold bit-identical sums), then the four waves in index order.
__device__ __forceinline__ double block_sum_256(double x, double* lds4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) lds4[threadIdx.x / kWave] = x;
    __syncthreads();
    const double s = ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(kNormThreads) void grad_sumsq_kernel(const float* __restrict__ g, long long n, long long slice,
                                                                  double* __restrict__ partial) {
    __shared__ double lds4[kNormThreads / kWave];
    const long long lo = (long long)blockIdx.x * slice;
    const long long hi = lo + slice < n ? lo + slice : n;          // (lo >= n: an empty slice, sum 0)
    double acc = 0.0;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {               // slice is a multiple of 4: every slice starts 16-byte aligned
        long long i = lo + 4LL * threadIdx.x;
        for (; i + 4 <= hi; i += 4LL * kNormThreads) {
            const float4 q = *reinterpret_cast<const float4*>(g + i);
            acc += (double)q.x * (double)q.x;
            acc += (double)q.y * (double)q.y;
            acc += (double)q.z * (double)q.z;
            acc += (double)q.w * (double)q.w;
        }
        for (; i < hi; ++i) acc += (double)g[i] * (double)g[i];     // (the one lane that holds the ragged end of the vector)
    } else {
        for (long long i = lo + threadIdx.x; i < hi; i += kNormThreads) acc += (double)g[i] * (double)g[i];
    }
    const double s = block_sum_256(acc, lds4);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(kNormThreads) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                    float* __restrict__ m, float* __restrict__ v, long long n,
                                                                    float lr_t, float b1, float b2, float eps, float grad_scale,
                                                                    float clip_norm, int skip_nonfinite,
                                                                    const double* __restrict__ partial, int G,
                                                                    double* __restrict__ state) {
    __shared__ double lds4[kNormThreads / kWave];
    const double sum = block_sum_256((int)threadIdx.x < G ? partial[threadIdx.x] : 0.0, lds4);
    const double norm = fabs((double)grad_scale) * sqrt(sum);
    const bool finite = norm <= 1.79769313486231570815e308;         // (false for NaN and for +inf)
    const bool skip = !finite && skip_nonfinite != 0;
    const bool clip = !skip && clip_norm > 0.f && norm > (double)clip_norm;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (skip) {
            state[2] += 1.0;
            state[3] += 1.0;
        } else {
            state[0] += 1.0;
            if (clip) state[1] += 1.0;
            state[3] = 0.0;
        }
        state[4] = norm;
        if (finite && norm > state[5]) state[5] = norm;
    }
    if (skip) return;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float gi = g[i] * grad_scale;
    if (clip) gi *= (float)((double)clip_norm / norm);              // (never a multiplication by 1 on the unclipped path)
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
}
}  // namespace psvo

extern "C" int psvo_adam_step(float* params, const float* grads, float* m, float* v, long long n, float lr,
                              float beta1, float beta2, float eps, long long step, float grad_scale,
                              void* stream) {
    using namespace psvo;
    if (!params || !grads || !m || !v || n <= 0 || step <= 0) return PSVO_ERR_INVALID;
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
    clear_hip_error();
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       params, grads, m, v, n, (float)lr_t, beta1, beta2, eps, grad_scale);
    return launch_status();
}

extern "C" int psvo_grad_norm_blocks(long long n) { return psvo::norm_blocks(n); }

extern "C" int psvo_grad_sumsq(const float* grads, long long n, double* partial, void* stream) {
    using namespace psvo;
    if (!grads || !partial || n <= 0) return PSVO_ERR_INVALID;
    const int G = norm_blocks(n);
    clear_hip_error();
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)G), dim3(kNormThreads), 0, static_cast<hipStream_t>(stream), grads, n,
                       norm_slice(n, G), partial);
    return launch_status();
}

extern "C" int psvo_adam_step_guarded(float* params, const float* grads, float* m, float* v, long long n, float lr,
                                      float beta1, float beta2, float eps, long long step, float grad_scale,
                                      float clip_norm, int skip_nonfinite, const double* partial, double* state,
                                      void* stream) {
    using namespace psvo;
    if (!params || !grads || !m || !v || !partial || !state || n <= 0 || step <= 0) return PSVO_ERR_INVALID;
    if (!(clip_norm >= 0.f) || !std::isfinite(clip_norm)) return PSVO_ERR_INVALID;
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
    clear_hip_error();
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)((n + kNormThreads - 1) / kNormThreads)), dim3(kNormThreads), 0,
                       static_cast<hipStream_t>(stream), params, grads, m, v, n, (float)lr_t, beta1, beta2, eps, grad_scale,
                       clip_norm, skip_nonfinite, partial, norm_blocks(n), state);
    return launch_status();
}
