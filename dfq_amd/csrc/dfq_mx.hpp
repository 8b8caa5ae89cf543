// What the MX block-scaled kernels share (dfq_mx_batch.hip: half a wave to a block along rows; dfq_mx_axis.hip: a lane to a block
// along any axis): the format table and the conversion between float32 and a format's codes.  The DEFINITION is in
// include/dfq_hip.h ("MX block-scaled").  The conversion is integer arithmetic on the float32 bit pattern in both directions:
// nothing here depends on how the hardware treats subnormals, and the CPU emulation runs the same code.  How a block's largest
// magnitude and its error sum are formed is each kernel's own; everything here works on one element.
#pragma once

#include "dfq_common.hpp"

namespace dfq {

constexpr int kMxBlock = DFQ_MX_BLOCK;
constexpr uint32_t kMxQuietNan = 0x7fc00000u;
constexpr int64_t kMxMost = 0x7fffffff / 4;           // blocks of a tensor, workgroups of a launch

struct MxFmt {
    int mbits, bias, cmax, emax, bits;
};

__host__ __device__ inline MxFmt mx_fmt(int id) {
    switch (id) {
        case DFQ_MX_E2M1: return MxFmt{1, 1, 7, 2, 4};
        case DFQ_MX_E2M3: return MxFmt{3, 1, 31, 2, 6};
        case DFQ_MX_E3M2: return MxFmt{2, 3, 31, 4, 6};
        case DFQ_MX_E4M3: return MxFmt{3, 7, 126, 8, 8};
        default: return MxFmt{2, 15, 123, 15, 8};              // DFQ_MX_E5M2
    }
}

// ---- conversion, on the bit patterns ---------------------------------------------------------------------------------------------
struct MxElem {
    float w;
    uint32_t sign;                // w's sign bit, in place
    uint32_t M;                   // |w| = M 2^(Ex - 150): bit 23 set (a subnormal is normalised), or 0 for a zero
    int32_t Ex;
    int32_t E;                    // of the block: amax's exponent field - 127
    bool bad;                     // the block holds a NaN or an Inf
};

// the element's own fields (w, sign, M, Ex); what belongs to the block (E, bad) is the caller's to fill from its largest magnitude
__device__ __forceinline__ MxElem mx_split(float w) {
    MxElem L;
    const uint32_t u = __float_as_uint(w), aw = u & 0x7fffffffu;
    L.w = w;
    L.sign = u & 0x80000000u;
    const uint32_t field = aw >> 23, mant = aw & 0x7fffffu;
    const int lz = mant ? __builtin_clz(mant) - 8 : 0;
    L.M = field ? (mant | 0x800000u) : (mant << lz);
    L.Ex = field ? (int32_t)field : 1 - lz;
    L.E = 0;
    L.bad = false;
    return L;
}

// the magnitude code nearest to |w| 2^-e, ties to the even code, saturated at cmax
__device__ __forceinline__ uint32_t mx_encode(const MxElem& L, int e, const MxFmt& f) {
    int ce = L.Ex - 127 - e + f.bias;                 // the exponent field the value would take
    ce = ce > 64 ? 64 : ce;                           // (far above cmax already; keeps the shift below in 32 bits)
    int sh = 23 - f.mbits + (ce < 1 ? 1 - ce : 0);
    sh = sh > 31 ? 31 : sh;
    const uint32_t val = L.M + ((uint32_t)(ce > 1 ? ce - 1 : 0) << 23);          // field | mantissa, 23 fraction bits
    const uint32_t k = (val + ((1u << (sh - 1)) - 1u) + ((val >> sh) & 1u)) >> sh;
    return L.M == 0 ? 0u : (k > (uint32_t)f.cmax ? (uint32_t)f.cmax : k);
}

// float32 pattern of value(k) 2^e, exact (subnormal results included); 2^128 and above: +Inf
__device__ __forceinline__ uint32_t mx_value_bits(uint32_t k, int e, const MxFmt& f) {
    const uint32_t ce = k >> f.mbits, cm = k & ((1u << f.mbits) - 1u);
    const uint32_t Mi = ce ? (cm | (1u << f.mbits)) : cm;
    const int p = (int)(ce ? ce : 1u) - f.bias - f.mbits + e;                     // value = Mi 2^p
    const int hb = 31 - __builtin_clz(Mi | 1u);
    const int field = p + hb + 127;
    uint32_t bits;
    if (field >= 255) bits = 0x7f800000u;
    else if (field >= 1) bits = ((uint32_t)field << 23) | ((Mi << (23 - hb)) & 0x7fffffu);
    else bits = Mi << (p + 149 > 0 ? p + 149 : 0);
    return Mi ? bits : 0u;
}

__device__ __forceinline__ double mx_sq_error(uint32_t stored, float w) {
    const double d = (double)__uint_as_float(stored) - (double)w;
    return d * d;
}

}  // namespace dfq
