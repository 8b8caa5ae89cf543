// MX block-scaled quantisation along any axis of a contiguous tensor (dfq_mx_axis; the activations' side of the MX formats).
// The DEFINITION is in include/dfq_hip.h ("MX block-scaled"); the result is dfq_mx_rows on the tensor with the axis moved last.
//
// x is [outer, len, inner] and the blocks run along len, so a block's elements lie `inner` floats apart.  ONE LANE OWNS A
// BLOCK: work item p = (o * bpa + j) * inner + i, i fastest, so for a fixed t the 64 lanes of a wave read 64 consecutive floats
// wherever inner >= 64 -- every load and store is a coalesced line.  The lane issues its 32 loads before the first use (an
// element past len reads the block's last element again, a valid address, and is replaced by +0.0f), takes the unsigned max of
// the magnitude patterns in its own registers, and encodes and stores element by element.  S(e): the definition's xor tree over
// t is adjacent pairwise summation -- (0+1), (2+3), then pairs of pairs -- which a lane forms from its own registers as a
// fully unrolled recursion; with `search` both S(e0) and S(e0 + 1) in one descent.  No LDS, no cross-lane exchange, no barrier,
// no atomic, no workgroup waits for another; a lane past the last item returns at once, nothing collective follows.
// IN PLACE (y == x): a lane reads its whole block before it writes any of it (every store depends on the block's largest
// magnitude, which depends on every load), and the blocks of different lanes are disjoint.
// The format is a template parameter, so that its shifts and limits are constants (measured against the format as an argument
// of the launch: 6 to 9 % of the time at [64, 96, 112, 112]); so is what is summed: nothing (no search, no
// err: no float64 arithmetic at all), S(e) of the one exponent, or the search's two sums.
#include "dfq_mx.hpp"

namespace dfq {
namespace {

typedef DFQ_GLOBAL_AS uint8_t mxa_guint8;
typedef DFQ_GLOBAL_AS double mxa_gdouble;

enum { kMxaPlain = 0, kMxaSum = 1, kMxaSearch = 2 };

struct MxAxisArgs {
    const float* x;
    float* y;
    uint8_t* codes;
    uint8_t* scales;
    double* err;
    int64_t inner;                // the distance of two elements of a block, floats
    uint32_t total, inner32, bpa; // total = outer * bpa * inner work items (at most kMxMost)
    int32_t len;
};

struct MxAxisLane {               // what a lane knows of its block
    gfloat* y;                    // at the block's first element, or null
    mxa_guint8* codes;
    int64_t step, at;             // floats between two elements of the block; where the next element to store lies
    int n;                        // elements the block really has
    bool bad;
};

// The elements of a block are independent, and left alone the compiler interleaves the 32 conversions of the search's descent:
// 256 VGPRs, one wave per SIMD.  A scheduling fence behind every group of kMxaGroup elements keeps a group's temporaries from
// outliving it.  The group's own partial sums are pinned in front of the fence (an empty asm that redefines them): their
// additions otherwise sink to where the sums are used, behind the last group, and every group leaves its 8 squares alive until
// then (210 VGPRs).  With both: 90 for the search, 59 for the one sum, 64 without sums; no scratch.
constexpr int kMxaGroup = 4;
__device__ __forceinline__ void mxa_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}
__device__ __forceinline__ void mxa_fence(double& s) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(s));
#endif
    mxa_fence();
}

// element t of the block at exponent e (the elements come in rising t): stores the weight and the code byte, returns the stored
// pattern
template <int kFmt>
__device__ __forceinline__ uint32_t mxa_put(MxAxisLane& B, int t, float w, int e) {
    const MxFmt F = mx_fmt(kFmt);
    const MxElem L = mx_split(w);
    const uint32_t k = B.bad ? 0u : mx_encode(L, e, F);
    const uint32_t stored = mx_value_bits(k, e, F) | L.sign;
    if (t < B.n) {
        if (B.y) B.y[B.at] = __uint_as_float(B.bad ? kMxQuietNan : stored);
        if (B.codes) B.codes[B.at] = (uint8_t)(B.bad ? 0u : (k | (L.sign >> (32 - F.bits))));
    }
    B.at += B.step;
    return stored;
}

// S(e) over elements [kLo, kLo + kN) as the definition's tree, the elements stored on the way
template <int kFmt, int kLo, int kN>
__device__ __forceinline__ double mxa_put_sum(MxAxisLane& B, const float (&w)[kMxBlock], int e) {
    if constexpr (kN == 1) {
        return mx_sq_error(mxa_put<kFmt>(B, kLo, w[kLo], e), w[kLo]);
    } else {
        const double a = mxa_put_sum<kFmt, kLo, kN / 2>(B, w, e);
        const double b = mxa_put_sum<kFmt, kLo + kN / 2, kN / 2>(B, w, e);
        double s = a + b;
        if (kN == kMxaGroup) mxa_fence(s);
        return s;
    }
}

// S(e0) and S(e0 + 1) over elements [kLo, kLo + kN), nothing stored
template <int kFmt, int kLo, int kN>
__device__ __forceinline__ void mxa_two_sums(const float (&w)[kMxBlock], int e0, double& s0, double& s1) {
    if constexpr (kN == 1) {
        const MxFmt F = mx_fmt(kFmt);
        const MxElem L = mx_split(w[kLo]);
        s0 = mx_sq_error(mx_value_bits(mx_encode(L, e0, F), e0, F) | L.sign, L.w);
        s1 = mx_sq_error(mx_value_bits(mx_encode(L, e0 + 1, F), e0 + 1, F) | L.sign, L.w);
    } else {
        double a0, a1, b0, b1;
        mxa_two_sums<kFmt, kLo, kN / 2>(w, e0, a0, a1);
        mxa_two_sums<kFmt, kLo + kN / 2, kN / 2>(w, e0, b0, b1);
        s0 = a0 + b0;
        s1 = a1 + b1;
        if (kN == kMxaGroup) { mxa_fence(s0); mxa_fence(s1); }
    }
}

template <int kFmt, int kMode>
__global__ __launch_bounds__(kBlock) void mx_axis_kernel(MxAxisArgs a) {
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (p >= a.total) return;
    const uint32_t q = p / a.inner32, i = p - q * a.inner32;
    const uint32_t o = q / a.bpa, j = q - o * a.bpa;
    const int64_t first = ((int64_t)o * a.len + (int64_t)j * kMxBlock) * a.inner + i;
    const int left = a.len - (int)(j * kMxBlock);          // >= 1
    MxAxisLane B;
    B.n = left < kMxBlock ? left : kMxBlock;
    B.step = a.inner;
    B.at = 0;
    B.y = a.y ? (gfloat*)a.y + first : nullptr;
    B.codes = a.codes ? (mxa_guint8*)a.codes + first : nullptr;

    const gfloat* x = (const gfloat*)a.x + first;
    float w[kMxBlock];
#pragma unroll
    for (int t = 0; t < kMxBlock; ++t) w[t] = x[(t < B.n ? t : B.n - 1) * B.step];
    uint32_t amax = 0;
#pragma unroll
    for (int t = 0; t < kMxBlock; ++t) {
        w[t] = t < B.n ? w[t] : 0.0f;
        const uint32_t aw = __float_as_uint(w[t]) & 0x7fffffffu;
        amax = aw > amax ? aw : amax;                      // (the patterns of non-negative floats are ordered as the values, NaN on top)
    }
    B.bad = amax >= 0x7f800000u;
    const MxFmt F = mx_fmt(kFmt);
    const int E = (int)(amax >> 23) - 127;
    const int e0 = E - F.emax > -127 ? E - F.emax : -127;
    int e = e0;
    double S = 0.0;
    if constexpr (kMode == kMxaSearch) {
        double S1;
        mxa_two_sums<kFmt, 0, kMxBlock>(w, e0, S, S1);
        if (S1 < S) { e = e0 + 1; S = S1; }                // (a tie, and a NaN on either side, keep e0)
#if defined(__HIP_DEVICE_COMPILE__)
        // the store pass splits every element again, and only once e is known: with the 32 (sign, M, Ex) carried over from the
        // descent the kernel takes 154 VGPRs instead of 90
#pragma unroll
        for (int t = 0; t < kMxBlock; ++t) asm("" : "+v"(w[t]) : "v"(e));
#endif
    }
    if constexpr (kMode == kMxaSum) {
        S = mxa_put_sum<kFmt, 0, kMxBlock>(B, w, e);
    } else {
#pragma unroll
        for (int t = 0; t < kMxBlock; ++t) {
            mxa_put<kFmt>(B, t, w[t], e);
            if (t % kMxaGroup == kMxaGroup - 1) mxa_fence();
        }
    }
    if (a.scales) ((mxa_guint8*)a.scales)[p] = (uint8_t)(B.bad ? 255 : e + 127);
    if (kMode != kMxaPlain && a.err) ((mxa_gdouble*)a.err)[p] = B.bad ? __builtin_nan("") : S;
}

template <int kMode>
void mx_axis_launch(int32_t format, dim3 grid, hipStream_t st, const MxAxisArgs& a) {
    switch (format) {
        case DFQ_MX_E2M1: hipLaunchKernelGGL((mx_axis_kernel<DFQ_MX_E2M1, kMode>), grid, dim3(kBlock), 0, st, a); break;
        case DFQ_MX_E2M3: hipLaunchKernelGGL((mx_axis_kernel<DFQ_MX_E2M3, kMode>), grid, dim3(kBlock), 0, st, a); break;
        case DFQ_MX_E3M2: hipLaunchKernelGGL((mx_axis_kernel<DFQ_MX_E3M2, kMode>), grid, dim3(kBlock), 0, st, a); break;
        case DFQ_MX_E4M3: hipLaunchKernelGGL((mx_axis_kernel<DFQ_MX_E4M3, kMode>), grid, dim3(kBlock), 0, st, a); break;
        default: hipLaunchKernelGGL((mx_axis_kernel<DFQ_MX_E5M2, kMode>), grid, dim3(kBlock), 0, st, a); break;
    }
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_mx_axis(const float* x, float* y, int64_t outer, int64_t len, int64_t inner, int32_t format, int32_t search,
                           uint8_t* codes, uint8_t* scales, double* err, void* stream) {
    const char* me = "dfq_mx_axis";
    if (format < DFQ_MX_E2M1 || format > DFQ_MX_E5M2) return fail_arg("%s: unknown format %d", me, (int)format);
    if (!x) return fail_arg("%s: null x", me);
    if ((uintptr_t)x % 4 != 0) return fail_arg("%s: x is not 4-byte aligned", me);
    if (outer <= 0 || len <= 0 || inner <= 0)
        return fail_arg("%s: empty tensor (outer %lld, len %lld, inner %lld)", me, (long long)outer, (long long)len, (long long)inner);
    if (len > 0x7fffffffll) return fail_arg("%s: len %lld above 2^31 - 1", me, (long long)len);
    const int64_t bpa = (len + kMxBlock - 1) / kMxBlock;
    if (outer > kMxMost / bpa || inner > kMxMost / (outer * bpa)) return fail_arg("%s: more than 2^29 blocks", me);
    if (inner == 1) return dfq_mx_rows(x, y, outer, len, format, search, codes, scales, err, stream);      // the row case
    MxAxisArgs a{};
    a.x = x; a.y = y; a.codes = codes; a.scales = scales; a.err = err;
    a.inner = inner;
    a.total = (uint32_t)(outer * bpa * inner); a.inner32 = (uint32_t)inner; a.bpa = (uint32_t)bpa;
    a.len = (int32_t)len;
    const dim3 grid((a.total + kBlock - 1) / kBlock);
    const hipStream_t st = as_stream(stream);
    if (search) mx_axis_launch<kMxaSearch>(format, grid, st, a);
    else if (err) mx_axis_launch<kMxaSum>(format, grid, st, a);
    else mx_axis_launch<kMxaPlain>(format, grid, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}
