// Dense bit-packing of the integer codes of a whole batch of networks, every tensor of every network at its own width, and the
// way back to codes and float32 weights (extension; what a mixed-precision calibration hands over: dfq_mixed_batch.hip chooses
// the widths, dfq_quant_batch.hip / dfq_squant_batch.hip / dfq_mixed_batch.hip leave one byte or four per weight, this leaves
// b / 8).  The definition -- unsigned code, stream, offsets, status, unpack -- is the comment of dfq_batch_pack_plan_create
// (include/dfq_hip.h).  The plans hold ONE network's tensor table, like the other batch plans, and cut every tensor into chunks
// of kPackChunk elements: a chunk is a multiple of 32 elements, so at every width it starts on a word boundary (and, 128 b
// words long, on a 16-byte one), the chunks of a tensor are independent and the grid depends on the element counts alone -- the
// host never learns a width.  A workgroup takes a span of kPackSpan consecutive chunks of one tensor, one after the other, the
// loads of later chunks issued before the current one is worked on ("Packed codes", has the measurements behind
// this shape).  Launches, none with a wait inside:
//   pack 0. pk_offsets_kernel, one workgroup per network: every width checked, then the extents scanned into the offsets
//           (a block-wide inclusive scan per 256 tensors, a carry between them) and the status (2: a bad width, nothing else
//           written; 1: the network does not fit its packed row).
//   pack 1. pk_pack_kernel: a workgroup reads its network's status and its tensor's width and offset once.  Per chunk the
//           codes, loaded coalesced 16 bytes per lane where the address allows, become u = (q - qmin) & (2^b - 1) and are
//           staged in the LDS -- a byte per code up to 8 bits, two above, zero behind the tensor's end.  Then 128 lanes take 32
//           consecutive codes each, which fill exactly b whole words: the width is workgroup-uniform, a switch picks the
//           instantiation in which it is a constant, and word j ORs the codes i with -b < i b - 32 j < 32 (at most
//           ceil(32 / b) + 1 of them) at constant shifts.  The words go through a second LDS array and all lanes store them
//           coalesced, 16 bytes per lane: no two lanes on one word, no atomic, and the tail, the zero padding up to the 4-word
//           extent and tensors shorter than a chunk take this same path.
//   unpack. pk_unpack_kernel: EVERY workgroup checks its network's widths and offsets against the extents (T loads from the
//           cache; nothing waits for a verdict of another workgroup; the network's first workgroup stores the status), loads
//           the chunk's words into the LDS, and every lane takes groups of four elements: u from the two words the element can
//           touch, q = u + qmin, and y = (float)q * scale + min_value with the QParams of the tensor's range -- or of the row's,
//           staged in the LDS once per quarter of a chunk (a float64 division per row, not per element).
// A code is read once and b / 8 bytes written; unpack reads b / 8 bytes and writes 4 (plus the code).
#include <limits.h>

#include <vector>

#include "dfq_batch_shared.hpp"

namespace dfq {

constexpr int kPackPerThread = 16;
constexpr int kPackChunk = kBlock * kPackPerThread;      // elements of a tensor one workgroup takes
constexpr int kPackMaxBits = 16;
constexpr int kPackMaxWords = kPackChunk / 32 * kPackMaxBits;   // words of a chunk at the widest width
constexpr int kPackSpan = 4;                             // consecutive chunks of one tensor a workgroup takes, one after the other
static_assert(kPackChunk % 32 == 0 && (kPackChunk / 32) % 4 == 0, "a chunk ends on a 16-byte boundary at every width");

typedef DFQ_GLOBAL_AS int32_t gint32p;
typedef DFQ_GLOBAL_AS uint32_t guint32p;
typedef DFQ_GLOBAL_AS uint8_t guint8p;
typedef DFQ_GLOBAL_AS int64_t gint64p;
typedef uint32_t uvec4 __attribute__((vector_size(16)));
typedef DFQ_GLOBAL_AS uvec4 guvec4;

struct PkTensorDev {
    float* data;                  // unpack: the weight in network 0, or null
    int64_t code_off, n, range_off;
    uint32_t row_len;             // unpack: elements of a row
    int32_t num_bits, width_index, symmetric, per_row;
    int32_t span_begin;           // its first span within one network
};

struct PkArgs {
    const PkTensorDev* tensors;
    const int32_t* span_tensor;   // tensor of every span of one network
    const int64_t* delta;         // unpack: bases[n] - bases[0], bytes
    unsigned char* codes;         // pack reads them, unpack writes them (or null)
    const int32_t* widths;
    uint32_t* words;              // pack writes them, unpack reads them
    int64_t* offsets;             // [n_nets, n_tensors + 1]
    int32_t* status;
    const float* ranges;
    int64_t code_stride, width_stride, word_stride, range_stride;
    int32_t code_bytes, n_tensors, spans_pn, pad;
};

__host__ __device__ __forceinline__ int64_t pk_extent(int64_t n, int b) { return (((n * b + 31) >> 5) + 3) & ~(int64_t)3; }

__device__ __forceinline__ int pk_width(const PkArgs& a, const PkTensorDev& T, int net) {
    return T.num_bits ? T.num_bits : ((const gint32p*)a.widths)[(int64_t)net * a.width_stride + T.width_index];
}

__device__ __forceinline__ bool pk_width_ok(int b, int code_bytes) { return b >= 1 && b <= (code_bytes == 1 ? 8 : kPackMaxBits); }

// pack, launch 0: one workgroup per network
__global__ __launch_bounds__(kBlock) void pk_offsets_kernel(PkArgs a) {
    __shared__ int64_t scan[kBlock];
    __shared__ int bad;
    const int net = (int)blockIdx.x;
    const int t = (int)threadIdx.x;
    const int nt = a.n_tensors;
    if (t == 0) bad = 0;
    __syncthreads();
    for (int i = t; i < nt; i += kBlock)
        if (!pk_width_ok(pk_width(a, a.tensors[i], net), a.code_bytes)) bad = 1;      // (every writer stores the same value)
    __syncthreads();
    if (bad) {                                         // (block-uniform)
        if (t == 0) a.status[net] = 2;
        return;
    }
    gint64p* off = (gint64p*)a.offsets + (int64_t)net * (nt + 1);
    int64_t carry = 0;
    for (int first = 0; first < nt; first += kBlock) {
        const int i = first + t;
        int64_t e = 0;
        if (i < nt) {
            const PkTensorDev T = a.tensors[i];
            e = pk_extent(T.n, pk_width(a, T, net));
        }
        __syncthreads();                               // the previous round's last reads of `scan`
        scan[t] = e;
        __syncthreads();
        for (int d = 1; d < kBlock; d <<= 1) {
            const int64_t below = t >= d ? scan[t - d] : 0;
            __syncthreads();
            scan[t] += below;
            __syncthreads();
        }
        if (i < nt) off[i + 1] = carry + scan[t];
        carry += scan[kBlock - 1];
    }
    if (t == 0) {
        off[0] = 0;
        a.status[net] = carry > a.word_stride ? 1 : 0;
    }
}

// four unsigned codes from element e on (e % 4 == 0) into the staging area
template <bool WIDE>
__device__ __forceinline__ void pk_stage4(uint32_t* stage, int e, const uint32_t (&u)[4]) {
    if constexpr (WIDE) {
        stage[(e >> 1) + 0] = u[0] | (u[1] << 16);
        stage[(e >> 1) + 1] = u[2] | (u[3] << 16);
    } else {
        stage[e >> 2] = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
    }
}


// the codes of one chunk as a lane loads them: 1-byte codes, 16 of them in r[0] (one 16-byte load); int32 codes, 4 in every r[j]
template <int CB>
struct PkCodes {
    uint32_t r[CB == 1 ? 1 : kPackPerThread / 4][4];
};

// c.r[i / 4][i % 4] = v for a slot known at run time only: selects, so that the codes stay in registers
template <int CB>
__device__ __forceinline__ void pk_put(PkCodes<CB>& c, int i, uint32_t v) {
#pragma unroll
    for (int s = 0; s < (CB == 1 ? 4 : kPackPerThread); ++s) c.r[s >> 2][s & 3] = s == i ? v : c.r[s >> 2][s & 3];
}

// every load of a chunk back to back (src: its first code; count: its codes), nothing used yet
template <int CB>
__device__ __forceinline__ void pk_load_codes(const unsigned char* src, int count, PkCodes<CB>& c) {
    const int t = (int)threadIdx.x;
    const bool aligned = ((uintptr_t)src & 15u) == 0;              // (block-uniform)
    if constexpr (CB == 1) {
        const int e0 = 16 * t;
#pragma unroll
        for (int k = 0; k < 4; ++k) c.r[0][k] = 0u;
        if (aligned && e0 + 16 <= count) {
            const uvec4 v = *(const guvec4*)(src + e0);
            c.r[0][0] = v[0]; c.r[0][1] = v[1]; c.r[0][2] = v[2]; c.r[0][3] = v[3];
        } else {                                       // (a caller's odd code offset, or the tensor's end: a rolled loop, few registers)
#pragma unroll 1
            for (int i = 0; i < 4; ++i) {
                uint32_t v = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e0 + 4 * i + k < count) v |= (uint32_t)((const guint8p*)src)[e0 + 4 * i + k] << (8 * k);
                pk_put(c, i, v);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPackPerThread / 4; ++j) {
            const int e0 = 4 * (j * kBlock + t);
#pragma unroll
            for (int k = 0; k < 4; ++k) c.r[j][k] = 0u;
            if (aligned && e0 + 4 <= count) {
                const uvec4 v = *(const guvec4*)(src + 4 * (int64_t)e0);
                c.r[j][0] = v[0]; c.r[j][1] = v[1]; c.r[j][2] = v[2]; c.r[j][3] = v[3];
            }
        }
        if (!aligned || (count & 3) != 0) {            // (block-uniform) what the vector loads left out, in a rolled loop
#pragma unroll 1
            for (int i = 0; i < kPackPerThread; ++i) {
                const int e = 4 * ((i >> 2) * kBlock + t) + (i & 3);
                const int e0 = e - (i & 3);
                if (e < count && !(aligned && e0 + 4 <= count)) pk_put(c, i, ((const guint32p*)src)[e]);
            }
        }
    }
}

// u = (q + bias) & mask of every loaded code into the staging area, zero behind the chunk's count
template <bool WIDE, int CB>
__device__ __forceinline__ void pk_stage_codes(const PkCodes<CB>& c, int count, uint32_t bias, uint32_t mask, uint32_t* stage) {
    const int t = (int)threadIdx.x;
    if constexpr (CB == 1) {                           // (a signed byte comes zero-extended: the mask has at most 8 bits)
        const int e0 = 16 * t;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t u[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) u[k] = e0 + 4 * j + k < count ? (((c.r[0][j] >> (8 * k)) & 0xffu) + bias) & mask : 0u;
            pk_stage4<WIDE>(stage, e0 + 4 * j, u);
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPackPerThread / 4; ++j) {
            const int e0 = 4 * (j * kBlock + t);
            uint32_t u[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) u[k] = e0 + k < count ? (c.r[j][k] + bias) & mask : 0u;
            pk_stage4<WIDE>(stage, e0, u);
        }
    }
}

// The 32 codes from chunk element 32 g on fill exactly B words, the words g B .. g B + B - 1 of the chunk.  B is a constant here:
// word j takes the codes i with -B < i B - 32 j < 32, each at a constant 32-bit shift (to the right for the one that began in
// word j - 1), and everything else folds away.  Every word is formed on its own: one accumulator over all 32 codes would be
// re-associated into a tree that holds every code at once.
template <int B, bool WIDE>
__device__ __forceinline__ void pk_compose32(const uint32_t* stage, int g, uint32_t* words) {
    constexpr int kDwords = WIDE ? 16 : 8;
    uint32_t d[kDwords];
#pragma unroll
    for (int i = 0; i < kDwords; ++i) d[i] = stage[kDwords * g + i];
#pragma unroll
    for (int j = 0; j < B; ++j) {
        uint32_t w = 0u;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int sh = i * B - 32 * j;
            if (sh > -B && sh < 32) {
                const uint32_t u = WIDE ? (d[i >> 1] >> (16 * (i & 1))) & 0xffffu : (d[i >> 2] >> (8 * (i & 3))) & 0xffu;
                w |= sh >= 0 ? u << (sh >= 0 ? sh : 0) : u >> (sh < 0 ? -sh : 0);
            }
        }
        words[g * B + j] = w;
    }
}

template <bool WIDE>
__device__ __forceinline__ void pk_compose(const uint32_t* stage, int b, int g, uint32_t* words) {
    constexpr int O = WIDE ? 8 : 0;
    switch (b - O) {                                   // (block-uniform)
        case 1: pk_compose32<O + 1, WIDE>(stage, g, words); break;
        case 2: pk_compose32<O + 2, WIDE>(stage, g, words); break;
        case 3: pk_compose32<O + 3, WIDE>(stage, g, words); break;
        case 4: pk_compose32<O + 4, WIDE>(stage, g, words); break;
        case 5: pk_compose32<O + 5, WIDE>(stage, g, words); break;
        case 6: pk_compose32<O + 6, WIDE>(stage, g, words); break;
        case 7: pk_compose32<O + 7, WIDE>(stage, g, words); break;
        default: pk_compose32<O + 8, WIDE>(stage, g, words); break;
    }
}

// words of chunk ci of a tensor of n elements at b bits: 128 b, less at the tensor's end (the extent's padding included)
__device__ __forceinline__ int pk_chunk_words(int64_t n, int b, int ci) {
    const int64_t full = (int64_t)(kPackChunk / 32) * b;
    const int64_t left = pk_extent(n, b) - (int64_t)ci * full;
    return (int)(left < full ? left : full);
}

__device__ __forceinline__ int pk_chunk_count(int64_t n, int ci) {
    const int64_t left = n - (int64_t)ci * kPackChunk;
    return (int)(left < kPackChunk ? left : kPackChunk);
}

// The chunks [c0, c1) of tensor T of network `net` at b bits, c1 - c0 <= kPackSpan.  The loads run ahead of the barriers:
// 1-byte codes, 4 registers a chunk, are all loaded before the first chunk is staged; int32 codes, 16 registers a chunk, one
// chunk ahead.
template <bool WIDE, int CB>
__device__ __forceinline__ void pk_pack_span(const PkArgs& a, const PkTensorDev& T, int net, int c0, int c1, int b, guint32p* tensor_words,
                                             uint32_t* stage, uint32_t* words) {
    const uint32_t mask = (1u << b) - 1u;
    const uint32_t bias = T.symmetric ? 1u << (b - 1) : 0u;        // -qmin
    const unsigned char* codes = a.codes + ((int64_t)net * a.code_stride + T.code_off) * CB;
    constexpr int kHeld = CB == 1 ? kPackSpan : 2;     // chunks whose codes a lane holds
    PkCodes<CB> held[kHeld];
#pragma unroll
    for (int i = 0; i < kHeld; ++i)
        if (c0 + i < c1) pk_load_codes<CB>(codes + (int64_t)(c0 + i) * kPackChunk * CB, pk_chunk_count(T.n, c0 + i), held[i]);
#pragma unroll
    for (int i = 0; i < kPackSpan; ++i) {              // (unrolled: the register slots are constants)
        const int c = c0 + i;
        if (c >= c1) break;                            // (block-uniform)
        pk_stage_codes<WIDE, CB>(held[i % kHeld], pk_chunk_count(T.n, c), bias, mask, stage);
        __syncthreads();
        if (kHeld < kPackSpan && c + kHeld < c1)
            pk_load_codes<CB>(codes + (int64_t)(c + kHeld) * kPackChunk * CB, pk_chunk_count(T.n, c + kHeld), held[i % kHeld]);
        const int t = (int)threadIdx.x;
        if (t < kPackChunk / 32) pk_compose<WIDE>(stage, b, t, words);         // (whole waves; behind the tensor's end the codes are zero)
        __syncthreads();
        // the chunk's words, coalesced; `stage` is free for the next chunk, and `words` is written again only behind its barrier
        guint32p* dst = tensor_words + (int64_t)c * (kPackChunk / 32) * b;
        const int nw = pk_chunk_words(T.n, b, c);
        if (((uintptr_t)dst & 15u) == 0) {             // (block-uniform; nw is a multiple of 4)
            for (int w = 4 * t; w < nw; w += 4 * kBlock) {
                uvec4 v;
                v[0] = words[w + 0]; v[1] = words[w + 1]; v[2] = words[w + 2]; v[3] = words[w + 3];
                *(guvec4*)(dst + w) = v;
            }
        } else {
            for (int w = t; w < nw; w += kBlock) dst[w] = words[w];
        }
    }
}

// pack, launch 1: one workgroup per span of kPackSpan chunks of one tensor of one network
__global__ __launch_bounds__(kBlock, 5) void pk_pack_kernel(PkArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[kPackChunk / 2];         // the unsigned codes of a chunk
    __shared__ __attribute__((aligned(16))) uint32_t words[kPackMaxWords];          // and its words
    const int net = (int)blockIdx.x / a.spans_pn;
    const int lp = (int)blockIdx.x - net * a.spans_pn;
    if (((const gint32p*)a.status)[net] != 0) return;  // (block-uniform) a bad width, or a row too short: nothing of it is written
    const int ti = a.span_tensor[lp];
    const PkTensorDev T = a.tensors[ti];
    const int b = pk_width(a, T, net);
    const int c0 = (lp - T.span_begin) * kPackSpan;
    const int n_chunks = (int)((T.n + kPackChunk - 1) / kPackChunk);
    const int c1 = c0 + kPackSpan < n_chunks ? c0 + kPackSpan : n_chunks;
    const int64_t toff = ((const gint64p*)a.offsets)[(int64_t)net * (a.n_tensors + 1) + ti];
    guint32p* tensor_words = (guint32p*)a.words + (int64_t)net * a.word_stride + toff;
    if (a.code_bytes == 1) pk_pack_span<false, 1>(a, T, net, c0, c1, b, tensor_words, stage, words);      // (uniform over the launch)
    else if (b > 8) pk_pack_span<true, 4>(a, T, net, c0, c1, b, tensor_words, stage, words);
    else pk_pack_span<false, 4>(a, T, net, c0, c1, b, tensor_words, stage, words);
}

// the words of one chunk as a lane loads them: word 4 (j kBlock + t) + k in r[j][k]
struct PkWords {
    uint32_t r[kPackMaxWords / (4 * kBlock)][4];
};

__device__ __forceinline__ void pk_load_words(const guint32p* src, int nw, PkWords& x) {
    const int t = (int)threadIdx.x;
    const bool aligned = ((uintptr_t)src & 15u) == 0;              // (block-uniform; nw is a multiple of 4)
#pragma unroll
    for (int j = 0; j < kPackMaxWords / (4 * kBlock); ++j) {
        const int w = 4 * (j * kBlock + t);
#pragma unroll
        for (int k = 0; k < 4; ++k) x.r[j][k] = 0u;
        if (w >= nw) continue;
        if (aligned) {
            const uvec4 v = *(const guvec4*)(src + w);
            x.r[j][0] = v[0]; x.r[j][1] = v[1]; x.r[j][2] = v[2]; x.r[j][3] = v[3];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) x.r[j][k] = src[w + k];
        }
    }
}

// unpack: one launch, one workgroup per span
__global__ __launch_bounds__(kBlock) void pk_unpack_kernel(PkArgs a) {
    constexpr int kQuarter = 4 * kBlock;               // elements of one round of 4 per lane; a quarter touches at most kQuarter rows
    __shared__ __attribute__((aligned(16))) uint32_t stage[kPackMaxWords + 4];
    __shared__ float row_scale[kQuarter], row_min[kQuarter];
    __shared__ int bad_width, bad_extent;
    const int t = (int)threadIdx.x;
    const int net = (int)blockIdx.x / a.spans_pn;
    const int lp = (int)blockIdx.x - net * a.spans_pn;
    const int nt = a.n_tensors;
    // the network's verdict, formed by every workgroup for itself
    if (t == 0) { bad_width = 0; bad_extent = 0; }
    __syncthreads();
    const gint64p* off = (const gint64p*)a.offsets + (int64_t)net * (nt + 1);
    for (int i = t; i < nt; i += kBlock) {
        const PkTensorDev Ti = a.tensors[i];
        const int bi = pk_width(a, Ti, net);
        if (!pk_width_ok(bi, a.code_bytes)) bad_width = 1;         // (every writer stores the same value)
        else if (off[i + 1] - off[i] != pk_extent(Ti.n, bi)) bad_extent = 1;
    }
    if (t == 0 && (off[0] != 0 || off[nt] > a.word_stride)) bad_extent = 1;
    __syncthreads();
    const int verdict = bad_width ? 2 : bad_extent ? 1 : 0;        // (block-uniform)
    if (lp == 0 && t == 0) a.status[net] = verdict;
    if (verdict) return;

    const int ti = a.span_tensor[lp];
    const PkTensorDev T = a.tensors[ti];
    const int b = pk_width(a, T, net);
    const int c0 = (lp - T.span_begin) * kPackSpan;
    const int n_chunks = (int)((T.n + kPackChunk - 1) / kPackChunk);
    const int c1 = c0 + kPackSpan < n_chunks ? c0 + kPackSpan : n_chunks;
    const guint32p* tensor_words = (const guint32p*)a.words + (int64_t)net * a.word_stride + off[ti];
    const uint32_t mask = (1u << b) - 1u;
    const int32_t qmin = T.symmetric ? -(int32_t)(1u << (b - 1)) : 0;
    unsigned char* tensor_codes = a.codes ? a.codes + ((int64_t)net * a.code_stride + T.code_off) * a.code_bytes : nullptr;
    gfloat* tensor_y = T.data ? (gfloat*)(float*)((char*)T.data + a.delta[net]) : nullptr;
    const gfloat* rg = (const gfloat*)a.ranges + (int64_t)net * a.range_stride + T.range_off;
    float scale = 0.0f, min_value = 0.0f;
    if (tensor_y && !T.per_row) {                      // (block-uniform) the tensor's own pair
        const QParams p = qparams_double((double)rg[0], (double)rg[1], b, T.symmetric);
        scale = p.scale;
        min_value = p.min_value;
    }
    PkWords cur;
    pk_load_words(tensor_words + (int64_t)c0 * (kPackChunk / 32) * b, pk_chunk_words(T.n, b, c0), cur);
    for (int c = c0; c < c1; ++c) {                    // (block-uniform bounds)
        const int64_t start = (int64_t)c * kPackChunk;
        const int count = pk_chunk_count(T.n, c);
        const int nw = pk_chunk_words(T.n, b, c);
#pragma unroll
        for (int j = 0; j < kPackMaxWords / (4 * kBlock); ++j) {
            const int w = 4 * (j * kBlock + t);
            if (w < nw) { stage[w + 0] = cur.r[j][0]; stage[w + 1] = cur.r[j][1]; stage[w + 2] = cur.r[j][2]; stage[w + 3] = cur.r[j][3]; }
        }
        if (t == 0) stage[nw] = 0u;                    // the word behind the last: read, never used
        __syncthreads();
        if (c + 1 < c1) pk_load_words(tensor_words + (int64_t)(c + 1) * (kPackChunk / 32) * b, pk_chunk_words(T.n, b, c + 1), cur);
        unsigned char* codes = tensor_codes ? tensor_codes + start * a.code_bytes : nullptr;
        const bool codes_aligned = ((uintptr_t)codes & (a.code_bytes == 1 ? 3u : 15u)) == 0;       // (block-uniform)
        gfloat* y = tensor_y ? tensor_y + start : nullptr;
#pragma unroll 1
        for (int j = 0; j < kPackPerThread / 4; ++j) {
            if (j * kQuarter >= count) break;          // (block-uniform)
            uint32_t rem = 0;
            if (y && T.per_row) {                      // (block-uniform) a pair per row this quarter touches, a float64 division each
                const int64_t first = start + (int64_t)j * kQuarter;
                const int64_t first_row = first / T.row_len;
                rem = (uint32_t)(first - first_row * T.row_len);
                const int here = count - j * kQuarter < kQuarter ? count - j * kQuarter : kQuarter;
                const int n_rows = (int)((rem + (uint32_t)here - 1u) / T.row_len) + 1;
                __syncthreads();                       // the previous quarter's reads
                for (int r = t; r < n_rows; r += kBlock) {
                    const QParams p = qparams_double((double)rg[2 * (first_row + r) + 0], (double)rg[2 * (first_row + r) + 1], b, T.symmetric);
                    row_scale[r] = p.scale;
                    row_min[r] = p.min_value;
                }
                __syncthreads();
            }
            const int e0 = j * kQuarter + 4 * t;
            if (e0 >= count) continue;
            const bool whole = e0 + 4 <= count;
            int32_t q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {              // (elements behind the tensor's end read the zero padding, or the next word)
                const uint32_t bit = (uint32_t)(e0 + k) * (uint32_t)b;
                const uint32_t wi = bit >> 5;
                const uint64_t pair = (uint64_t)stage[wi] | ((uint64_t)stage[wi + 1] << 32);
                q[k] = (int32_t)((uint32_t)(pair >> (bit & 31u)) & mask) + qmin;
            }
            if (codes) {
                if (a.code_bytes == 4) {
                    if (whole && codes_aligned) {
                        uvec4 v;
                        v[0] = (uint32_t)q[0]; v[1] = (uint32_t)q[1]; v[2] = (uint32_t)q[2]; v[3] = (uint32_t)q[3];
                        *(guvec4*)(codes + 4 * (int64_t)e0) = v;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (e0 + k < count) ((gint32p*)codes)[e0 + k] = q[k];
                    }
                } else {                               // the int32 code's low byte: uint8 (asymmetric) / int8 (symmetric)
                    if (whole && codes_aligned) {
                        *(guint32p*)(codes + e0) = ((uint32_t)q[0] & 0xffu) | (((uint32_t)q[1] & 0xffu) << 8) |
                                                   (((uint32_t)q[2] & 0xffu) << 16) | (((uint32_t)q[3] & 0xffu) << 24);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (e0 + k < count) ((guint8p*)codes)[e0 + k] = (uint8_t)q[k];
                    }
                }
            }
            if (y) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float sc = scale, mv = min_value;
                    if (T.per_row) {
                        const uint32_t r = (rem + (uint32_t)(4 * t + k)) / T.row_len;      // (< kQuarter also behind the tensor's end)
                        sc = row_scale[r];
                        mv = row_min[r];
                    }
                    v[k] = (float)q[k] * sc;           // two roundings (the build never contracts them)
                    v[k] = v[k] + mv;
                }
                if (whole) {                           // (the weight is 16-byte aligned, a chunk starts 16 KB further on)
                    *(gfvec4*)(y + e0) = fvec4{v[0], v[1], v[2], v[3]};
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e0 + k < count) y[e0 + k] = v[k];
                }
            }
        }
        __syncthreads();                               // the staging area is the next chunk's
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// one tensor of either table as the checks and the device see it
struct PkTensorHost {
    float* data;
    int64_t rows, row_len, code_offset, numel, range_offset;
    int32_t num_bits, width_index, symmetric, per_row;
};

// what both creates check and build: the device table and the span table, the arguments filled as far as both plans share them
inline int pk_prepare(const char* me, const std::vector<PkTensorHost>& tensors, const void* const* bases, int32_t n_nets, bool with_codes,
                      int32_t code_bytes, int64_t code_stride, const int32_t* widths, int64_t width_stride, int64_t word_stride,
                      std::vector<PkTensorDev>& dev, std::vector<int32_t>& span_tensor) {
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    for (int n = 1; n < n_nets; ++n)
        if (((uintptr_t)bases[n] - (uintptr_t)bases[0]) % 16 != 0) return fail_arg("%s: network %d is not 16-byte aligned to network 0", me, n);
    if (with_codes && code_bytes != 1 && code_bytes != 4) return fail_arg("%s: code width %d bytes (1 or 4)", me, (int)code_bytes);
    if (code_stride < 0 || width_stride < 0 || word_stride < 0) return fail_arg("%s: negative stride", me);
    int64_t total = 0, spans = 0;
    for (size_t i = 0; i < tensors.size(); ++i) {
        const PkTensorHost& t = tensors[i];
        if (t.numel <= 0) return fail_arg("%s: tensor %d: %lld elements", me, (int)i, (long long)t.numel);
        if (t.numel > INT64_MAX / 64 - total) return fail_arg("%s: too many codes for a 64-bit count of bits", me);
        total += t.numel;
        if (t.num_bits != 0 && (t.num_bits < 1 || t.num_bits > kPackMaxBits))
            return fail_arg("%s: tensor %d: a width of %d bits (1..%d, or 0 for the width block)", me, (int)i, (int)t.num_bits, kPackMaxBits);
        if (with_codes && code_bytes == 1 && t.num_bits > 8) return fail_arg("%s: tensor %d: 1-byte codes of %d bits", me, (int)i, (int)t.num_bits);
        if (t.num_bits == 0) {
            if (!widths) return fail_arg("%s: tensor %d reads its width from the width block, which is null", me, (int)i);
            if (t.width_index < 0 || t.width_index >= width_stride)
                return fail_arg("%s: tensor %d: width index %d outside the width stride %lld", me, (int)i, (int)t.width_index, (long long)width_stride);
        }
        if (with_codes && (t.code_offset < 0 || t.code_offset > code_stride - t.numel))
            return fail_arg("%s: tensor %d: codes outside the code stride", me, (int)i);
        PkTensorDev d{};
        d.data = t.data;
        d.code_off = with_codes ? t.code_offset : 0;
        d.n = t.numel;
        d.range_off = t.range_offset;
        d.row_len = (uint32_t)t.row_len;
        d.num_bits = t.num_bits;
        d.width_index = t.width_index;
        d.symmetric = t.symmetric ? 1 : 0;
        d.per_row = t.per_row ? 1 : 0;
        d.span_begin = (int32_t)spans;
        const int64_t k = (t.numel + (int64_t)kPackSpan * kPackChunk - 1) / ((int64_t)kPackSpan * kPackChunk);
        spans += k;
        if (spans * n_nets > 0x7fffffff) return fail_arg("%s: too much work for one launch", me);
        span_tensor.insert(span_tensor.end(), (size_t)k, (int32_t)i);
        dev.push_back(d);
    }
    return DFQ_OK;
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_pack_plan {
    DevSlab mem;
    PkArgs args{};
    int n_nets = 0;
};

struct dfq_batch_unpack_plan {
    DevSlab mem;
    PkArgs args{};
    int n_nets = 0;
};

extern "C" {

int64_t dfq_batch_pack_chunk_elements(void) { return kPackChunk; }

int32_t dfq_batch_pack_plan_launches(const dfq_batch_pack_plan* p) { return p ? 2 : 0; }

int32_t dfq_batch_unpack_plan_launches(const dfq_batch_unpack_plan* p) { return p ? 1 : 0; }

void dfq_batch_pack_plan_destroy(dfq_batch_pack_plan* p) { batch_plan_destroy(p); }

void dfq_batch_unpack_plan_destroy(dfq_batch_unpack_plan* p) { batch_plan_destroy(p); }

int dfq_batch_pack_plan_create(const dfq_batch_pack_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                               const void* codes, int32_t code_bytes, int64_t code_stride, const int32_t* widths, int64_t width_stride,
                               uint32_t* packed, int64_t word_stride, int64_t* offsets, int32_t* status, dfq_batch_pack_plan** out_plan) {
    const char* me = "dfq_batch_pack_plan_create";
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (!tensors || n_tensors <= 0) return fail_arg("%s: the tensor table is null or empty (n_tensors %d)", me, (int)n_tensors);
    if (!codes || !packed || !offsets || !status) return fail_arg("%s: a null block (codes, packed, offsets, status)", me);
    std::vector<PkTensorHost> host;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_pack_tensor& t = tensors[i];
        host.push_back(PkTensorHost{nullptr, 1, t.numel, t.code_offset, t.numel, -1, t.num_bits, t.width_index, t.symmetric, 0});
    }
    std::vector<PkTensorDev> dev;
    std::vector<int32_t> span_tensor;
    if (const int rc = pk_prepare(me, host, bases, n_nets, true, code_bytes, code_stride, widths, width_stride, word_stride, dev, span_tensor))
        return rc;
    dfq_batch_pack_plan* p = new dfq_batch_pack_plan();
    PkArgs& a = p->args;
    a.codes = (unsigned char*)const_cast<void*>(codes);
    a.widths = widths;
    a.words = packed;
    a.offsets = offsets;
    a.status = status;
    a.code_stride = code_stride;
    a.width_stride = width_stride;
    a.word_stride = word_stride;
    a.code_bytes = code_bytes;
    a.n_tensors = n_tensors;
    a.spans_pn = (int32_t)span_tensor.size();
    p->n_nets = n_nets;
    BatchUpload up{p->mem};
    a.tensors = up.put(dev);
    a.span_tensor = up.put(span_tensor);
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch pack plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_pack_plan_run(dfq_batch_pack_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_pack_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    const PkArgs& a = p->args;
    hipLaunchKernelGGL(pk_offsets_kernel, dim3(p->n_nets), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(pk_pack_kernel, dim3(a.spans_pn * p->n_nets), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

int dfq_batch_unpack_plan_create(const dfq_batch_unpack_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                                 const uint32_t* words, int64_t word_stride, const int64_t* offsets, const int32_t* widths,
                                 int64_t width_stride, const float* ranges, int64_t range_stride, void* codes, int32_t code_bytes,
                                 int64_t code_stride, int32_t* status, dfq_batch_unpack_plan** out_plan) {
    const char* me = "dfq_batch_unpack_plan_create";
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (!tensors || n_tensors <= 0) return fail_arg("%s: the tensor table is null or empty (n_tensors %d)", me, (int)n_tensors);
    if (!words || !offsets || !status) return fail_arg("%s: a null block (words, offsets, status)", me);
    if (range_stride < 0) return fail_arg("%s: negative stride", me);
    std::vector<PkTensorHost> host;
    bool any_weight = false;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_unpack_tensor& t = tensors[i];
        if (t.data) {
            any_weight = true;
            if ((uintptr_t)t.data % 16 != 0) return fail_arg("%s: tensor %d: the weight is not 16-byte aligned", me, i);
            if (t.rows <= 0 || t.row_len <= 0 || t.row_len > 0x7fffffff || t.numel <= 0 || t.numel / t.rows != t.row_len || t.numel % t.rows != 0)
                return fail_arg("%s: tensor %d: a shape of [%lld, %lld] for %lld elements", me, i, (long long)t.rows, (long long)t.row_len,
                                (long long)t.numel);
            if (!ranges) return fail_arg("%s: tensor %d writes its weight, but the range block is null", me, i);
            if (t.range_offset < 0 || t.range_offset > range_stride - 2 * (t.per_row ? t.rows : 1))
                return fail_arg("%s: tensor %d: ranges outside the range stride", me, i);
        }
        host.push_back(PkTensorHost{t.data, t.rows, t.row_len, t.code_offset, t.numel, t.range_offset, t.num_bits, t.width_index, t.symmetric, t.per_row});
    }
    if (!codes && !any_weight) return fail_arg("%s: neither a code block nor a weight to write", me);
    std::vector<PkTensorDev> dev;
    std::vector<int32_t> span_tensor;
    if (const int rc = pk_prepare(me, host, bases, n_nets, codes != nullptr, code_bytes, code_stride, widths, width_stride, word_stride, dev, span_tensor))
        return rc;
    dfq_batch_unpack_plan* p = new dfq_batch_unpack_plan();
    PkArgs& a = p->args;
    a.codes = (unsigned char*)codes;
    a.widths = widths;
    a.words = const_cast<uint32_t*>(words);
    a.offsets = const_cast<int64_t*>(offsets);
    a.status = status;
    a.ranges = ranges;
    a.code_stride = code_stride;
    a.width_stride = width_stride;
    a.word_stride = word_stride;
    a.range_stride = range_stride;
    a.code_bytes = codes ? code_bytes : 4;
    a.n_tensors = n_tensors;
    a.spans_pn = (int32_t)span_tensor.size();
    p->n_nets = n_nets;
    BatchUpload up{p->mem};
    a.tensors = up.put(dev);
    a.span_tensor = up.put(span_tensor);
    a.delta = up.put(batch_delta(bases, n_nets));
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch unpack plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_unpack_plan_run(dfq_batch_unpack_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_unpack_plan_run: null plan");
    const PkArgs& a = p->args;
    hipLaunchKernelGGL(pk_unpack_kernel, dim3(a.spans_pn * p->n_nets), dim3(kBlock), 0, as_stream(stream), a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
