// The device functions the activation-range kernels share (dfq_act.hip: one network, one launch per operation;
// dfq_act_batch.hip: a batch of networks, every operation of a quantiser in one workgroup): NaN-propagating min / max, the
// workgroup fold to (min, max), and the moments of N(beta, gamma^2) behind ReLU / ReLU6 (utils/layer_transform.py:403-418).
// Float32 arithmetic in the reference's operation order; pdf / cdf in float64 rounded to float32 (normal_pdf_cdf).
#pragma once

#include "dfq_common.hpp"

namespace dfq {

// torch.min / torch.max propagate NaN
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* sh) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        mn = nan_min(mn, __shfl_xor(mn, m));
        mx = nan_max(mx, __shfl_xor(mx, m));
    }
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) { sh[2 * wave] = mn; sh[2 * wave + 1] = mx; }
    __syncthreads();
    mn = sh[0]; mx = sh[1];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) { mn = nan_min(mn, sh[2 * w]); mx = nan_max(mx, sh[2 * w + 1]); }
}

// sd = sqrt(var + eps) of an accumulated variance (:533-540, :571-573), the one statement of all four sites that take it.  The
// float32 ReLU6 variance of a narrow channel on the ceiling (w = 1.04e-3, b = 5.99877: -6.8e-6, in truth 8.7e-7) cancels to a
// number below -eps, and the reference's sqrt is NaN there: the whole quantiser's range.  The radicand is clamped at 0 -- by
// a comparison, not fmaxf, so that a NaN variance still propagates.  Bit-identical to the reference wherever that is finite.
__device__ __forceinline__ float sd_of(float var, float eps) {
    const float r = var + eps;
    return sqrtf((r < 0.0f) ? 0.0f : r);
}

// calculate_mean / calculate_var (:407-410)
__device__ __forceinline__ void moments_relu(float w, float b, float& mean, float& var) {
    const float t = (-b) / w;
    float pdf, cdf;
    normal_pdf_cdf(t, pdf, cdf);
    const float one_m = 1.0f - cdf;
    mean = w * pdf + b * one_m;
    const float poly = ((b * b + w * w) + mean * mean) - (2.0f * mean) * b;
    const float t1 = one_m * poly;
    const float t2 = (w * (b - 2.0f * mean)) * pdf;
    const float t3 = (mean * mean) * cdf;
    var = (t1 + t2) + t3;
}

// calculate_mean_6 / calculate_var_6 (:411-418)
__device__ __forceinline__ void moments_relu6(float w, float b, float& mean, float& var) {
    const float lo = (-b) / w;
    const float hi = (6.0f - b) / w;
    float pdf_lo, cdf_lo, pdf_hi, cdf_hi;
    normal_pdf_cdf(lo, pdf_lo, cdf_lo);
    normal_pdf_cdf(hi, pdf_hi, cdf_hi);
    const float dp = pdf_lo - pdf_hi;
    const float dc = cdf_hi - cdf_lo;
    const float top = 1.0f - cdf_hi;
    mean = (w * dp + b * dc) + 6.0f * top;
    const float poly = ((b * b + w * w) + mean * mean) - (2.0f * mean) * b;
    const float t1 = dc * poly;
    const float t2 = (w * -6.0f) * pdf_hi;
    const float t3 = (w * (b - 2.0f * mean)) * dp;
    const float t4 = (mean * mean) * cdf_lo;
    const float d6 = 6.0f - mean;
    const float t5 = (d6 * d6) * top;
    var = (((t1 + t2) + t3) + t4) + t5;
}

__device__ __forceinline__ void moments_of(int mode, float w, float b, float& mean, float& var) {
    if (mode == 1) moments_relu(w, b, mean, var);
    else if (mode == 2) moments_relu6(w, b, mean, var);
    else { mean = b; var = w * w; }                     // :505-507
}

}  // namespace dfq
