// The NaN-skipping (min, max) reductions of the library, once: every range outside the equalisation engines (dfq_le*.hip,
// dfq_le_cf.hpp, which weave their folds into their tiles) is taken through the functions below.  The rule is the one
// include/dfq_hip.h states under "Special values" and "NaN rule of the channel ranges": a NaN of any payload, quiet or
// signalling, is SKIPPED, and a range of nothing but NaN keeps the identities (+inf, -inf).  range_fold* are the only places
// where a value straight from memory meets a raw v_min_f32 / v_max_f32 (dfq_common.hpp: a signalling NaN operand would make
// the instruction return a NaN and cost the lane what it had accumulated), so they quiet it first.  Everything behind them --
// butterflies, the LDS hop, the atomics -- sees results of those instructions, which are never signalling.
// All min / max are selections: every result is exact, whatever the order of the folds.
// NOT here: block_minmax and nan_min / nan_max of dfq_act_shared.hpp.  They PROPAGATE NaN on purpose (torch's rule for
// activation ranges); that is a different reduction.
// Device functions only.
#pragma once

#include "dfq_common.hpp"

namespace dfq {

// ---- one value from memory into a lane's running range ---------------------------------------------------------------
__device__ __forceinline__ void range_fold(float v, float& mn, float& mx) {
    v = quiet_nan(v);
    mn = vmin_raw(mn, v);
    mx = vmax_raw(mx, v);
}
__device__ __forceinline__ void range_fold4(const fvec4& v, float& mn, float& mx) {
    const float x0 = quiet_nan(v[0]), x1 = quiet_nan(v[1]), x2 = quiet_nan(v[2]), x3 = quiet_nan(v[3]);
    mn = vmin_raw(vmin_raw(mn, x0), vmin_raw(x1, vmin_raw(x2, x3)));
    mx = vmax_raw(vmax_raw(mx, x0), vmax_raw(x1, vmax_raw(x2, x3)));
}
// |v| into a running max|.| that starts at 0.0f (a run of nothing but NaN stays 0)
__device__ __forceinline__ void range_fold_abs(float v, float& m) { m = vmax_raw(m, fabsf(quiet_nan(v))); }
// two accumulated ranges (results of the folds above, never signalling)
__device__ __forceinline__ void range_merge(float& mn, float& mx, float omn, float omx) {
    mn = vmin_raw(mn, omn);
    mx = vmax_raw(mx, omx);
}

// ---- a workgroup over a contiguous span: thread t folds the 16-byte vectors t, t + kBlock, ... -----------------------------
// IN_FLIGHT independent 16-byte loads per trip (a read-only pass with one load in flight per lane leaves most of the memory
// pipeline idle), then four, then one, then the up-to-three floats behind the last vector; a span that does not start on
// 16 bytes is read float by float.  The rule is the same on every path.
template <int IN_FLIGHT>
__device__ __forceinline__ void range_span(const float* __restrict__ p, int64_t len, float& mn, float& mx) {
    const int tid = threadIdx.x;
    int64_t tail = tid;
    if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const int64_t n4 = len >> 2;
        const fvec4* p4 = reinterpret_cast<const fvec4*>(p);
        int64_t i = tid;
        for (; i + (IN_FLIGHT - 1) * kBlock < n4; i += IN_FLIGHT * kBlock) {
            fvec4 v[IN_FLIGHT];
#pragma unroll
            for (int u = 0; u < IN_FLIGHT; ++u) v[u] = kReadNt ? DFQ_NT_LOAD(p4 + i + u * kBlock) : p4[i + u * kBlock];
#pragma unroll
            for (int u = 0; u < IN_FLIGHT; ++u) range_fold4(v[u], mn, mx);
        }
        if constexpr (IN_FLIGHT > 4) {
            for (; i + 3 * kBlock < n4; i += 4 * kBlock) {
                fvec4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = p4[i + u * kBlock];
#pragma unroll
                for (int u = 0; u < 4; ++u) range_fold4(v[u], mn, mx);
            }
        }
        for (; i < n4; i += kBlock) range_fold4(p4[i], mn, mx);
        tail += n4 << 2;
    }
    for (int64_t i = tail; i < len; i += kBlock) range_fold(p[i], mn, mx);
}

// ---- one wave over a row: lane l folds elements l, l + kWave, ...; the row's range in every lane ---------------------------
// (P: const float* or a pointer into the global address space)
template <typename P>
__device__ __forceinline__ void wave_row_range(P row, int64_t len, float& mn, float& mx) {
    mn = INFINITY;
    mx = -INFINITY;
    for (int64_t i = threadIdx.x % kWave; i < len; i += kWave) range_fold(row[i], mn, mx);
    wave_minmax(mn, mx);
}

// ---- the lanes' ranges into the workgroup's: butterfly, one LDS hop over the four waves; the result in every thread ------------
// `sh` holds 2 * kBlock / kWave floats; a caller that comes back rewrites it and puts a __syncthreads() in between.
__device__ __forceinline__ void block_range(float& mn, float& mx, float* sh) {
    wave_minmax(mn, mx);
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x % kWave) == 0) { sh[2 * wave + 0] = mn; sh[2 * wave + 1] = mx; }
    __syncthreads();
    mn = sh[0];
    mx = sh[1];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) range_merge(mn, mx, sh[2 * w + 0], sh[2 * w + 1]);
}
__device__ __forceinline__ void block_range(float& mn, float& mx) {
    __shared__ float sh[2 * (kBlock / kWave)];
    block_range(mn, mx, sh);
}

// ---- a range into its pair of order-preserving words (dfq_common.hpp: ~enc_ord(min), enc_ord(max), identity 0) ----------------
// For ONE thread of those that hold the range.  A range of nothing but NaN has kept the identities and is left out; the
// words may be global memory or an LDS table.
__device__ __forceinline__ void range_publish(float mn, float mx, uint32_t* min_word, uint32_t* max_word) {
    if (mn <= mx) {
        atomicMax(min_word, ~enc_ord(mn));
        atomicMax(max_word, enc_ord(mx));
    }
}

// largest s with begin[s] <= item: the segment (tensor, layer) of a workgroup or row, from the table of first items
__device__ __forceinline__ int find_segment(const int32_t* __restrict__ begin, int n_segs, int item) {
    int lo = 0, hi = n_segs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (begin[mid] <= item) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace dfq
