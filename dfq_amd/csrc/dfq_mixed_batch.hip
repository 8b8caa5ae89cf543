// Mixed-precision weight quantisation of a whole batch of networks of one architecture (extension; the per-layer bit
// allocation under a size budget that ZeroQ is known for, on top of the quantiser of dfq_quant_batch.hip).  The definition --
// errors, allocation, quantisation -- is the comment of dfq_batch_mixed_plan_create (include/dfq_hip.h).  The plan holds
// network 0's tensor table and one byte offset per network, like the other batch plans, and cuts the work as the quant plan
// does: a per-row tensor, or a per-tensor one of at most kMixRegElems elements (a single row), goes row by row, L lanes per
// row, L in {4, 8, 16, 32, 64} by the row length, a lane's share of the row in registers; rows longer than kMixRegElems get a
// looping wave; longer per-tensor tensors are cut into chunks of kMixChunk elements, one workgroup each.  Launches, none with
// a wait inside:
//   0. (only with chunked tensors) bm_chunk_minmax_kernel: every chunk's (min, max) into its tensor's pair of cleared
//      order-preserving words (atomicMax of enc_ord: min and max do not depend on the order of the merges).
//   1. bm_error_kernel: the unit's range (from its registers, or the tensor's words), the range block, and under EVERY
//      candidate width the sum of e^2 over the elements the lane holds -- B float64 accumulators per lane next to the unit's
//      registers, the widths in the outer loop, the elements in the inner one: a weight is read once for all B errors.  A lane
//      adds in the order (row set, register slot); wave_sum (a fixed butterfly) gives the wave's sums, block_sum a chunk's;
//      they go to the plan's scratch [n_nets, parts, B], a part being a wave of the row tensors or a chunk.
//   2. bm_alloc_kernel, one workgroup per network: a thread per (tensor, width) adds the tensor's parts in rising order (the
//      errors block; cost = sensitivity * error, or * the caller's cost after set_costs, into LDS), then the first wave walks
//      the greedy allocation.  Lane l owns the
//      tensors l, l + 64, ...: their current index and their cached next step (g, k) lie in LDS and are touched by the owner
//      alone, so the walk needs no barrier: per step a scan of the owned tensors, a butterfly argmax of (g, tensor) over the
//      wave, a broadcast of the step's size from the owner, the budget test (the same in every lane), and the owner's
//      recomputation of one next step (B - 1 float64 divisions).  The walk is a chain of at most T (B - 1) dependent steps
//      whatever runs it; on the device the 64 networks of a batch walk side by side on 64 compute units, and nothing goes to
//      the host between the errors and the quantisation.
//   3. (only with `apply`) bm_quant_kernel: dfq_quant_batch.hip's quantising launch, the width read per network and tensor
//      from the bits block: qparams_double + fake_quant_one on the same range, so weight and code are bit for bit the quant
//      plan's.
// A weight is read twice (three times in chunks and long rows) and written once.  No floating-point atomic anywhere: two runs
// are bit-identical, and network n's values depend on nothing but its weights.  NaN is skipped by every range (range_fold,
// dfq_range.hpp); an element that is NaN has e = NaN, so a tensor holding one gets NaN errors, in its own slots only, and
// takes no step (g > 0 is false).
// A CLIPPED plan (dfq_batch_mixed_plan_create_clipped) is the same plan object with other launches in front of and behind
// bm_alloc_kernel, which it uses as it is: dfq_mixed_clip.hpp, included below, holds them and says how they are cut.  The stages
// (dfq_batch_mixed_plan_run_stages) of a plan without clipping are the launches above plus bm_state_kernel of that header.
#include <limits.h>
#include <math.h>

#include <vector>

#include "dfq_batch_shared.hpp"
#include "dfq_range.hpp"

namespace dfq {

constexpr int kMixMaxWidths = 8;
constexpr int kMixMaxEntries = 4096;                   // T * B the allocation's LDS table holds
constexpr int kMixMaxTensors = kMixMaxEntries / 2;     // (B >= 2)
constexpr int kMixRegPerLane = 24;                     // register slots per lane of the 64-lane class (kRegPerLane of dfq_quant_batch.hip)
constexpr int64_t kMixRegElems = (int64_t)kWave * kMixRegPerLane;   // longest unit kept in registers
constexpr int kMixSmallPerLane = 4;                    // the classes L < 64 hold rows of at most 4 L elements,
constexpr int kMixGroupRows = 4;                       // kMixGroupRows of them per lane group
constexpr int kMixChunkPerThread = 16;
constexpr int kMixChunk = kBlock * kMixChunkPerThread; // elements of a per-tensor tensor one workgroup owns

typedef DFQ_GLOBAL_AS int32_t gint32m;
typedef DFQ_GLOBAL_AS uint8_t guint8m;
typedef DFQ_GLOBAL_AS double gdouble;

struct BmRowDev {                 // a tensor taken row by row (a per-tensor one of <= kMixRegElems elements: one row)
    float* data;                  // network 0
    int64_t code_off, range_off;  // into one network's block, -1 = none
    int32_t rows, len;
    int32_t cls;                  // 0: one wave per row, looping; c > 0: L = 2 << c lanes per row
    int32_t wave_begin;           // first wave (within one network)
    int32_t tensor, pad;          // its place in the caller's table
};

struct BmChunkDev {               // a per-tensor tensor of more than kMixRegElems elements
    float* data;
    int64_t code_off, range_off;
    int64_t n;
    int32_t chunk_begin, n_chunks;   // its chunks within one network
    int32_t tensor, pad;
};

struct BmAllocDev {               // a tensor as the allocation sees it, in the caller's order
    int64_t n;                    // rows * row_len
    double sens;
    int32_t part_begin, n_parts;  // its partial sums within one network
    int32_t fixed, pad;           // index of the width it is pinned to, -1 = free
};

struct BmArgs {
    const BmRowDev* rows;
    const int32_t* wave_tensor;   // row tensor of every wave of network 0
    const BmChunkDev* chunks;
    const int32_t* chunk_tensor;  // chunk tensor of every chunk of network 0
    const BmAllocDev* alloc;
    const int32_t* width_tab;     // the widths once more, for the indexed reads of the allocation
    const int64_t* delta;         // bases[n] - bases[0], bytes
    uint32_t* slots;              // [n_nets, chunk_tensors, 2]: ~enc_ord(min), enc_ord(max)
    double* partial;              // [n_nets, parts_pn, n_widths]
    int32_t* bits;                // [n_nets, n_tensors]
    double* errors;               // [n_nets, n_tensors, n_widths]
    const double* costs;          // [n_nets, n_tensors, n_widths] the allocation weighs in place of the errors, or null (set_costs)
    int64_t* used;                // [n_nets, 2]
    double* cost;                 // [n_nets]
    unsigned char* codes;
    float* ranges;
    int64_t code_stride, range_stride, budget;
    int32_t widths[kMixMaxWidths];
    int32_t n_widths, symmetric, code_bytes, n_tensors;
    int32_t row_wpn, row_waves;
    int32_t chunks_pn, chunk_blocks, chunk_tensors, parts_pn;
};

__device__ __forceinline__ void bm_store_code(unsigned char* codes, int code_bytes, int64_t i, float code) {
    if (code_bytes == 4) ((gint32m*)codes)[i] = (int32_t)code;
    else ((guint8m*)codes)[i] = (uint8_t)(int32_t)code;  // the int32 code's low byte: uint8 (asymmetric) / int8 (symmetric)
}

// e^2 of one element, in float64 (the product of two float32 is exact there)
__device__ __forceinline__ double bm_sq(float w, const QParams& q) {
    float code;
    const double e = (double)(fake_quant_one(w, q, &code) - w);
    return e * e;
}

// R sets of 64 / L rows of one tensor from first_row on (row first_row + j * 64 / L + lane / L), L lanes each, K register slots
// per lane and row (len <= K * L).  QUANT: the rows quantised at num_bits; else their ranges stored and their e^2 under every
// width added to acc.
template <int L, int K, int R, bool QUANT>
__device__ __forceinline__ void bm_rows(const BmArgs& a, const BmRowDev& T, float* x, unsigned char* codes, float* ranges, int first_row,
                                        int num_bits, double (&acc)[kMixMaxWidths]) {
    constexpr int G = kWave / L;
    const int lane = threadIdx.x % kWave;
    const int g = lane % L;
    const int r0 = first_row + lane / L;
    const int len = T.len;
    gfloat* xr0 = (gfloat*)x;
    float v[R][K];                                     // every load first, the folds after them (see bq_rows)
#pragma unroll
    for (int j = 0; j < R; ++j) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[j][k] = 0.0f;
        if (first_row + j * G >= T.rows) break;        // (wave-uniform)
        const int r = r0 + j * G;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k * L >= len) break;                   // (wave-uniform)
            const int i = g + k * L;
            if (r < T.rows && i < len) v[j][k] = xr0[(int64_t)r * len + i];
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (first_row + j * G >= T.rows) break;
        const int r = r0 + j * G;
        const bool live = r < T.rows;
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k * L >= len) break;
            const int i = g + k * L;
            if (live && i < len) range_fold(v[j][k], mn, mx);
        }
        if constexpr (L > 1) xor_lane_minmax<1>(mn, mx);
        if constexpr (L > 2) xor_lane_minmax<2>(mn, mx);
        if constexpr (L > 4) xor_lane_minmax<4>(mn, mx);
        if constexpr (L > 8) xor_lane_minmax<8>(mn, mx);
        if constexpr (L > 16) xor_lane_minmax<16>(mn, mx);
        if constexpr (L > 32) xor_lane_minmax<32>(mn, mx);
        if (!live) continue;
        if constexpr (QUANT) {
            const QParams p = qparams_double((double)mn, (double)mx, num_bits, a.symmetric);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (k * L >= len) break;
                const int i = g + k * L;
                if (i < len) {
                    float code;
                    xr0[(int64_t)r * len + i] = fake_quant_one(v[j][k], p, &code);
                    if (codes) bm_store_code(codes, a.code_bytes, (int64_t)r * len + i, code);
                }
            }
        } else {
            if (ranges && g == 0) { ((gfloat*)ranges)[2 * r + 0] = mn; ((gfloat*)ranges)[2 * r + 1] = mx; }
#pragma unroll
            for (int b = 0; b < kMixMaxWidths; ++b) {
                if (b >= a.n_widths) break;            // (uniform over the launch)
                const QParams p = qparams_double((double)mn, (double)mx, a.widths[b], a.symmetric);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (k * L >= len) break;
                    const int i = g + k * L;
                    if (i < len) acc[b] += bm_sq(v[j][k], p);
                }
            }
        }
    }
}

// one row longer than kMixRegElems: one wave, the row read for its range and once more (from the cache) for all the errors,
// or for the quantisation
template <bool QUANT>
__device__ __forceinline__ void bm_long_row(const BmArgs& a, const BmRowDev& T, float* x, unsigned char* codes, float* ranges, int r,
                                            int num_bits, double (&acc)[kMixMaxWidths]) {
    const int lane = threadIdx.x % kWave;
    const int len = T.len;
    gfloat* xr = (gfloat*)x + (int64_t)r * len;
    float mn, mx;
    wave_row_range(xr, len, mn, mx);
    if constexpr (QUANT) {
        const QParams p = qparams_double((double)mn, (double)mx, num_bits, a.symmetric);
        for (int i = lane; i < len; i += kWave) {
            float code;
            xr[i] = fake_quant_one(xr[i], p, &code);
            if (codes) bm_store_code(codes, a.code_bytes, (int64_t)r * len + i, code);
        }
    } else {
        if (ranges && lane == 0) { ((gfloat*)ranges)[2 * r + 0] = mn; ((gfloat*)ranges)[2 * r + 1] = mx; }
        QParams q[kMixMaxWidths];
#pragma unroll
        for (int b = 0; b < kMixMaxWidths; ++b)            // (constant indices: the table stays in registers)
            q[b] = qparams_double((double)mn, (double)mx, b < a.n_widths ? a.widths[b] : a.widths[0], a.symmetric);
        for (int i = lane; i < len; i += kWave) {
            const float w = xr[i];
#pragma unroll
            for (int b = 0; b < kMixMaxWidths; ++b) {
                if (b >= a.n_widths) break;
                acc[b] += bm_sq(w, q[b]);
            }
        }
    }
}

// launch 0 (only with per-tensor tensors longer than kMixRegElems): every chunk of every network folded into its tensor's slots
__global__ __launch_bounds__(kBlock) void bm_chunk_minmax_kernel(BmArgs a) {
    const int net = (int)blockIdx.x / a.chunks_pn;
    const int c = (int)blockIdx.x - net * a.chunks_pn;
    const int t = a.chunk_tensor[c];
    const BmChunkDev T = a.chunks[t];
    const gfloat* x = (const gfloat*)(const float*)((const char*)T.data + a.delta[net]);
    const int64_t b = (int64_t)(c - T.chunk_begin) * kMixChunk;
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kMixChunkPerThread; ++j) {
        const int64_t i = b + j * kBlock + threadIdx.x;
        if (i < T.n) range_fold(x[i], mn, mx);
    }
    block_range(mn, mx);
    if (threadIdx.x == 0) {                            // (nothing for a chunk of NaNs)
        uint32_t* slot = a.slots + 2 * ((int64_t)net * a.chunk_tensors + t);
        range_publish(mn, mx, slot + 0, slot + 1);
    }
}

// launches 1 and 3: the chunks of the long per-tensor tensors (their tensor's range from its slots), then the row groups
template <bool QUANT>
__device__ __forceinline__ void bm_units(const BmArgs& a, double* sh) {
    double acc[kMixMaxWidths];
#pragma unroll
    for (int b = 0; b < kMixMaxWidths; ++b) acc[b] = 0.0;
    if ((int)blockIdx.x < a.chunk_blocks) {            // (block-uniform)
        const int net = (int)blockIdx.x / a.chunks_pn;
        const int c = (int)blockIdx.x - net * a.chunks_pn;
        const int t = a.chunk_tensor[c];
        const BmChunkDev T = a.chunks[t];
        const uint32_t* slot = a.slots + 2 * ((int64_t)net * a.chunk_tensors + t);
        const float mn = slot_min(slot[0]);
        const float mx = slot_max(slot[1]);
        const int ci = c - T.chunk_begin;
        gfloat* x = (gfloat*)(float*)((char*)T.data + a.delta[net]);
        const int64_t base = (int64_t)ci * kMixChunk;
        float v[kMixChunkPerThread];
#pragma unroll
        for (int j = 0; j < kMixChunkPerThread; ++j) {
            const int64_t i = base + j * kBlock + threadIdx.x;
            v[j] = i < T.n ? x[i] : 0.0f;
        }
        if constexpr (QUANT) {
            const int num_bits = a.bits[(int64_t)net * a.n_tensors + T.tensor];
            const QParams p = qparams_double((double)mn, (double)mx, num_bits, a.symmetric);
            unsigned char* codes = T.code_off >= 0 ? a.codes + ((int64_t)net * a.code_stride + T.code_off) * a.code_bytes : nullptr;
#pragma unroll
            for (int j = 0; j < kMixChunkPerThread; ++j) {
                const int64_t i = base + j * kBlock + threadIdx.x;
                if (i < T.n) {
                    float code;
                    x[i] = fake_quant_one(v[j], p, &code);
                    if (codes) bm_store_code(codes, a.code_bytes, i, code);
                }
            }
        } else {
            if (ci == 0 && threadIdx.x == 0 && T.range_off >= 0) {
                gfloat* rg = (gfloat*)a.ranges + (int64_t)net * a.range_stride + T.range_off;
                rg[0] = mn;
                rg[1] = mx;
            }
            gdouble* part = (gdouble*)a.partial + ((int64_t)net * a.parts_pn + a.row_wpn + c) * a.n_widths;
#pragma unroll
            for (int b = 0; b < kMixMaxWidths; ++b) {
                if (b >= a.n_widths) break;            // (uniform over the launch)
                const QParams p = qparams_double((double)mn, (double)mx, a.widths[b], a.symmetric);
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < kMixChunkPerThread; ++j) {
                    const int64_t i = base + j * kBlock + threadIdx.x;
                    if (i < T.n) s += bm_sq(v[j], p);
                }
                s = block_sum(s, sh);
                if (threadIdx.x == 0) part[b] = s;
            }
        }
        return;
    }
    const int w = ((int)blockIdx.x - a.chunk_blocks) * (kBlock / kWave) + (int)threadIdx.x / kWave;
    if (w >= a.row_waves) return;                      // (wave-uniform)
    const int net = w / a.row_wpn;
    const int lw = w - net * a.row_wpn;
    const BmRowDev T = a.rows[a.wave_tensor[lw]];
    float* x = (float*)((char*)T.data + a.delta[net]);
    unsigned char* codes = nullptr;
    float* ranges = nullptr;
    int num_bits = 0;
    if constexpr (QUANT) {
        codes = T.code_off >= 0 ? a.codes + ((int64_t)net * a.code_stride + T.code_off) * a.code_bytes : nullptr;
        num_bits = a.bits[(int64_t)net * a.n_tensors + T.tensor];
    } else {
        ranges = T.range_off >= 0 ? a.ranges + (int64_t)net * a.range_stride + T.range_off : nullptr;
    }
    const int wi = lw - T.wave_begin;
    switch (T.cls) {
        case 1: bm_rows<4, kMixSmallPerLane, kMixGroupRows, QUANT>(a, T, x, codes, ranges, wi * 16 * kMixGroupRows, num_bits, acc); break;
        case 2: bm_rows<8, kMixSmallPerLane, kMixGroupRows, QUANT>(a, T, x, codes, ranges, wi * 8 * kMixGroupRows, num_bits, acc); break;
        case 3: bm_rows<16, kMixSmallPerLane, kMixGroupRows, QUANT>(a, T, x, codes, ranges, wi * 4 * kMixGroupRows, num_bits, acc); break;
        case 4: bm_rows<32, kMixSmallPerLane, kMixGroupRows, QUANT>(a, T, x, codes, ranges, wi * 2 * kMixGroupRows, num_bits, acc); break;
        case 5: bm_rows<64, kMixRegPerLane, 1, QUANT>(a, T, x, codes, ranges, wi, num_bits, acc); break;
        default: bm_long_row<QUANT>(a, T, x, codes, ranges, wi, num_bits, acc); break;
    }
    if constexpr (!QUANT) {
        gdouble* part = (gdouble*)a.partial + ((int64_t)net * a.parts_pn + lw) * a.n_widths;
#pragma unroll
        for (int b = 0; b < kMixMaxWidths; ++b) {
            if (b >= a.n_widths) break;
            const double s = wave_sum(acc[b]);
            if (threadIdx.x % kWave == 0) part[b] = s;
        }
    }
}

__global__ __launch_bounds__(kBlock) void bm_error_kernel(BmArgs a) {
    __shared__ double sh[kBlock / kWave];
    bm_units<false>(a, sh);
}

__global__ __launch_bounds__(kBlock) void bm_quant_kernel(BmArgs a) {
    bm_units<true>(a, nullptr);
}

// the next step of a free tensor standing at width j: the k > j of greatest g = (c[j] - c[k]) / (n (b_k - b_j)) > 0, the largest
// such k on a tie; k = -1 if there is none
__device__ __forceinline__ void bm_next(const double* c, const int32_t* width, int nb, int j, int64_t n, double& g_out, int& k_out) {
    double best = 0.0;
    int kb = -1;
    for (int k = j + 1; k < nb; ++k) {
        const double g = (c[j] - c[k]) / (double)(n * (int64_t)(width[k] - width[j]));
        if (g > 0.0 && g >= best) { best = g; kb = k; }            // (false for NaN)
    }
    g_out = best;
    k_out = kb;
}

// launch 2: one workgroup per network -- the parts folded into the errors, then the greedy walk
__global__ __launch_bounds__(kBlock) void bm_alloc_kernel(BmArgs a) {
    __shared__ double cost[kMixMaxEntries];            // sensitivity * error of (tensor, width)
    __shared__ double next_g[kMixMaxTensors];          // the cached next step of a tensor: its g
    __shared__ int8_t next_k[kMixMaxTensors];          //   and its width index, -1 = finished or pinned
    __shared__ uint8_t at[kMixMaxTensors];             // the width index a tensor stands at
    const int net = (int)blockIdx.x;
    const int t = (int)threadIdx.x;
    const int nb = a.n_widths;
    const int nt = a.n_tensors;
    for (int i = t; i < nt * nb; i += kBlock) {
        const int ti = i / nb;
        const int j = i - ti * nb;
        const BmAllocDev D = a.alloc[ti];
        const gdouble* part = (const gdouble*)a.partial + ((int64_t)net * a.parts_pn + D.part_begin) * nb + j;
        double s = 0.0;
#pragma unroll 8
        for (int q = 0; q < D.n_parts; ++q) s += part[(int64_t)q * nb];
        ((gdouble*)a.errors)[((int64_t)net * nt + ti) * nb + j] = s;
        cost[i] = D.sens * (a.costs ? ((const gdouble*)a.costs)[((int64_t)net * nt + ti) * nb + j] : s);
    }
    __syncthreads();
    long long used = 0;
    int steps = 0;
    if (t < kWave) {                                   // (wave-uniform: the first wave walks, the others wait below)
        const int lane = t;
        for (int ti = lane; ti < nt; ti += kWave) {
            const BmAllocDev D = a.alloc[ti];
            const int j = D.fixed >= 0 ? D.fixed : 0;
            at[ti] = (uint8_t)j;
            used += (long long)D.n * a.width_tab[j];
            double g = 0.0;
            int k = -1;
            if (D.fixed < 0) bm_next(cost + ti * nb, a.width_tab, nb, j, D.n, g, k);
            next_g[ti] = g;
            next_k[ti] = (int8_t)k;
        }
#pragma unroll
        for (int m = kWave / 2; m > 0; m >>= 1) used += __shfl_xor(used, m);
        for (;;) {
            double g = 0.0;
            int bt = INT_MAX;
            for (int ti = lane; ti < nt; ti += kWave) {
                const double gg = next_g[ti];
                if (next_k[ti] >= 0 && gg > g) { g = gg; bt = ti; }      // (rising ti: the lowest on a tie)
            }
#pragma unroll
            for (int m = kWave / 2; m > 0; m >>= 1) {
                const double og = __shfl_xor(g, m);
                const int ot = __shfl_xor(bt, m);
                if (og > g || (og == g && ot < bt)) { g = og; bt = ot; }
            }
            if (bt == INT_MAX) break;                  // every free tensor is finished
            const int owner = bt % kWave;
            long long d = 0;
            int j = 0, k = 0;
            int64_t n = 0;
            if (lane == owner) {
                j = at[bt];
                k = next_k[bt];
                n = a.alloc[bt].n;
                d = (long long)n * (a.width_tab[k] - a.width_tab[j]);
            }
            d = __shfl(d, owner);
            if (used + d > (long long)a.budget) break; // the walk ENDS at the first step that does not fit
            used += d;
            ++steps;
            if (lane == owner) {
                at[bt] = (uint8_t)k;
                double ng;
                int nk;
                bm_next(cost + bt * nb, a.width_tab, nb, k, n, ng, nk);
                next_g[bt] = ng;
                next_k[bt] = (int8_t)nk;
            }
        }
    }
    __syncthreads();
    for (int ti = t; ti < nt; ti += kBlock) ((gint32m*)a.bits)[(int64_t)net * nt + ti] = a.width_tab[at[ti]];
    if (t == 0) {
        double c = 0.0;
        for (int ti = 0; ti < nt; ++ti) c += cost[ti * nb + at[ti]];
        a.cost[net] = c;
        a.used[2 * net + 0] = used;
        a.used[2 * net + 1] = steps;
    }
}

// lane class of a row of `len` elements: the fewest lanes that hold it in kMixSmallPerLane slots, 64 up to kMixRegElems, else 0
inline int bm_class(int len) {
    for (int c = 1; c <= 4; ++c)
        if (len <= (int64_t)(2 << c) * kMixSmallPerLane) return c;
    return len <= kMixRegElems ? 5 : 0;
}

}  // namespace dfq

#include "dfq_mixed_clip.hpp"      // the kernels of a clipped plan and of the stages (this file alone includes it)

using namespace dfq;

struct dfq_batch_mixed_plan {
    DevSlab mem;
    BmArgs args{};
    int n_nets = 0, apply = 0, launches = 0;
    int32_t* state = nullptr;     // [n_nets, n_tensors]: the index j_t the last ALLOCATE stage left
    bool allocated = false;       // an ALLOCATE stage has run since creation
    bool clipped = false;
    BxArgs cx{};                  // a clipped plan's own arguments
    size_t word_bytes = 0;
    int row_blocks = 0, piece_blocks = 0, fold_blocks = 0, finish_blocks = 0;
};

namespace {

// what both entry points refuse and build; `clip` null: dfq_batch_mixed_plan_create, as it always was
int bm_create(const char* me, const dfq_batch_mixed_tensor* tensors, int32_t n_tensors, const dfq_batch_mixed_config* config,
              const void* const* bases, int32_t n_nets, int32_t* bits, double* errors, int64_t* used, double* cost, void* codes,
              int64_t code_stride, float* ranges, int64_t range_stride, const dfq_batch_mixed_clip* clip, bool clipped,
              dfq_batch_mixed_plan** out_plan) {
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (!tensors || n_tensors <= 0) return fail_arg("%s: the tensor table is null or empty (n_tensors %d)", me, (int)n_tensors);
    if (!config) return fail_arg("%s: no configuration", me);
    const dfq_batch_mixed_config cfg = *config;
    const int nb = cfg.n_widths;
    if (nb < 2 || nb > kMixMaxWidths) return fail_arg("%s: %d candidate widths (2..%d)", me, nb, kMixMaxWidths);
    for (int j = 0; j < nb; ++j) {
        if (cfg.widths[j] < 2 || cfg.widths[j] > 16) return fail_arg("%s: width %d is %d, outside [2, 16]", me, j, (int)cfg.widths[j]);
        if (j > 0 && cfg.widths[j] <= cfg.widths[j - 1])
            return fail_arg("%s: the widths do not rise (%d behind %d)", me, (int)cfg.widths[j], (int)cfg.widths[j - 1]);
    }
    if ((int64_t)n_tensors * nb > kMixMaxEntries)
        return fail_arg("%s: %d tensors x %d widths, the allocation's table holds %d entries", me, (int)n_tensors, nb, kMixMaxEntries);
    if (cfg.budget_bits < 0) return fail_arg("%s: a negative budget (%lld bits)", me, (long long)cfg.budget_bits);
    if (cfg.code_bytes != 0 && cfg.code_bytes != 1 && cfg.code_bytes != 4) return fail_arg("%s: code width %d bytes (0, 1 or 4)", me, (int)cfg.code_bytes);
    if (cfg.code_bytes == 1 && cfg.widths[nb - 1] > 8) return fail_arg("%s: 1-byte codes of up to %d bits", me, (int)cfg.widths[nb - 1]);
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    for (int n = 1; n < n_nets; ++n)
        if (((uintptr_t)bases[n] - (uintptr_t)bases[0]) % 16 != 0) return fail_arg("%s: network %d is not 16-byte aligned to network 0", me, n);
    if (!bits || !errors || !used || !cost) return fail_arg("%s: a null output block (bits, errors, used, cost)", me);
    if (code_stride < 0 || range_stride < 0) return fail_arg("%s: negative stride", me);
    const int per_row = cfg.per_row ? 1 : 0;
    int K = 0;
    if (clipped) {
        if (!clip) return fail_arg("%s: no clip description", me);
        K = clip->candidates;
        if (K < 1 || K > kMxMaxCand) return fail_arg("%s: %d candidates (1..%d)", me, K, kMxMaxCand);
        if (!(clip->alpha_min > 0.0 && clip->alpha_min <= 1.0)) return fail_arg("%s: alpha_min %g is not in (0, 1]", me, clip->alpha_min);
        if (nb * K > kMxMaxPairs) return fail_arg("%s: %d widths x %d candidates, at most %d pairs", me, nb, K, kMxMaxPairs);
        if (!clip->clip_ranges || !clip->clip_chosen) return fail_arg("%s: the block of the clip ranges or of the choices is null", me);
        if (!clip->unit_offsets) return fail_arg("%s: no unit offsets", me);
        if (clip->unit_stride <= 0) return fail_arg("%s: unit stride %lld", me, (long long)clip->unit_stride);
        if (clip->unit_stride > INT64_MAX / 16 / nb / n_nets)
            return fail_arg("%s: blocks of %d x %lld units", me, (int)n_nets, (long long)clip->unit_stride);
    }

    std::vector<BmRowDev> rows;
    std::vector<BmChunkDev> chunks;
    std::vector<BmAllocDev> alloc;
    std::vector<int32_t> wave_tensor, chunk_tensor;
    std::vector<BxRowDev> xrows;
    std::vector<BxFlatDev> xflats;
    std::vector<BxTensorDev> xtensors;
    std::vector<int32_t> piece_tensor, part_tensor;
    int64_t waves = 0, nchunks = 0, total = 0, parts = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_mixed_tensor& t = tensors[i];
        if (!t.data) return fail_arg("%s: tensor %d: null weight", me, i);
        if (t.rows <= 0 || t.row_len <= 0 || t.row_len > INT64_MAX / 64 / t.rows)
            return fail_arg("%s: tensor %d: a shape of [%lld, %lld]", me, i, (long long)t.rows, (long long)t.row_len);
        if ((uintptr_t)t.data % 16 != 0) return fail_arg("%s: tensor %d: the weight is not 16-byte aligned", me, i);
        const int64_t numel = t.rows * t.row_len;
        total += numel;
        if (total > INT64_MAX / 64) return fail_arg("%s: too many weights for a 64-bit count of bits", me);
        if (!(t.sensitivity >= 0.0) || !(t.sensitivity <= 1.79769313486231570e308))
            return fail_arg("%s: tensor %d: a sensitivity of %g (finite, >= 0)", me, i, t.sensitivity);
        int fixed = -1;
        if (t.fixed_bits != 0) {
            for (int j = 0; j < nb; ++j)
                if (cfg.widths[j] == t.fixed_bits) fixed = j;
            if (fixed < 0) return fail_arg("%s: tensor %d: fixed_bits %d is not a candidate width", me, i, (int)t.fixed_bits);
        }
        if (t.code_offset < -1 || t.range_offset < -1) return fail_arg("%s: tensor %d: negative offset", me, i);
        if (t.code_offset >= 0) {
            if (!codes) return fail_arg("%s: tensor %d writes codes, but the code block is null", me, i);
            if (cfg.code_bytes == 0) return fail_arg("%s: tensor %d writes codes, but code_bytes is 0", me, i);
            if (t.code_offset > code_stride - numel) return fail_arg("%s: tensor %d: codes overflow the code stride", me, i);
        }
        if (t.range_offset >= 0) {
            if (!ranges) return fail_arg("%s: tensor %d writes ranges, but the range block is null", me, i);
            if (t.range_offset > range_stride - 2 * (per_row ? t.rows : 1)) return fail_arg("%s: tensor %d: ranges overflow the range stride", me, i);
        }
        BmAllocDev A{numel, t.sensitivity, 0, 0, fixed, 0};
        if (clipped) {                                 // the clip plan's cut: a unit is a part of the allocation's fold
            const int64_t units = per_row ? t.rows : 1, uo = clip->unit_offsets[i];
            if (t.rows > 0x7fffffff - kWave || t.row_len > 0x7fffffff - 2 * kBatchPiece || t.rows > (0x7fffffff - 2 * kBatchPiece) / t.row_len)
                return fail_arg("%s: tensor %d: a shape of [%lld, %lld]", me, i, (long long)t.rows, (long long)t.row_len);
            if (uo < 0 || uo > clip->unit_stride - units)
                return fail_arg("%s: tensor %d: %lld units at %lld lie outside the unit stride %lld", me, i, (long long)units, (long long)uo,
                                (long long)clip->unit_stride);
            if ((parts + units) * n_nets > 0x7fffffff / 2 / nb) return fail_arg("%s: too much work for one launch", me);
            A.part_begin = (int32_t)parts;
            A.n_parts = (int32_t)units;
            xtensors.push_back(BxTensorDev{uo, t.range_offset, (int32_t)parts, 0});
            part_tensor.insert(part_tensor.end(), (size_t)units, (int32_t)i);
            if (!per_row && numel > kMixRegElems) {
                BxFlatDev f{t.data, numel, uo, t.code_offset, t.range_offset, (int32_t)numel, 0, 0, (int32_t)xflats.size(), i, (int32_t)parts};
                const int64_t begin = batch_add_pieces(piece_tensor, (int32_t)xflats.size(), numel, 0x7fffffff / n_nets / (nb * K));
                if (begin < 0) return fail_arg("%s: too much work for one launch", me);
                f.piece_begin = (int32_t)begin;
                f.n_pieces = (int32_t)((int64_t)piece_tensor.size() - begin);
                xflats.push_back(f);
            } else {
                BxRowDev r;
                r.data = t.data; r.unit_off = uo; r.code_off = t.code_offset; r.range_off = t.range_offset;
                r.rows = (int32_t)units;
                r.len = (int32_t)(per_row ? t.row_len : numel);
                r.cls = bm_class(r.len);
                r.wave_begin = (int32_t)waves;
                r.tensor = i; r.part_begin = (int32_t)parts;
                const int64_t per_wave = r.cls == 5 || r.cls == 0 ? 1 : kWave / (2 << r.cls) * kMixGroupRows;
                const int64_t w = (r.rows + per_wave - 1) / per_wave;
                if ((waves + w) * n_nets > 0x7fffffff - kBlock) return fail_arg("%s: too much work for one launch", me);
                wave_tensor.insert(wave_tensor.end(), (size_t)w, (int32_t)xrows.size());
                xrows.push_back(r);
                waves += w;
            }
            parts += units;
        } else if (!per_row && numel > kMixRegElems) {
            BmChunkDev c;
            c.data = t.data; c.code_off = t.code_offset; c.range_off = t.range_offset; c.n = numel;
            c.chunk_begin = (int32_t)nchunks;
            const int64_t k = (numel + kMixChunk - 1) / kMixChunk;
            if (k * n_nets > 0x7fffffff / 2 / nb) return fail_arg("%s: too much work for one launch", me);
            c.n_chunks = (int32_t)k;
            c.tensor = i; c.pad = 0;
            A.part_begin = -1 - (int32_t)nchunks;      // (behind the waves: fixed below)
            A.n_parts = (int32_t)k;
            chunk_tensor.insert(chunk_tensor.end(), (size_t)k, (int32_t)chunks.size());
            chunks.push_back(c);
            nchunks += k;
        } else {
            BmRowDev r;
            r.data = t.data; r.code_off = t.code_offset; r.range_off = t.range_offset;
            const int64_t rr = per_row ? t.rows : 1, len = per_row ? t.row_len : numel;
            if (rr > 0x7fffffff - kWave || len > 0x7fffffff - kWave) return fail_arg("%s: tensor %d: too many rows or a row too long", me, i);
            r.rows = (int32_t)rr;
            r.len = (int32_t)len;
            r.cls = bm_class(r.len);
            r.wave_begin = (int32_t)waves;
            r.tensor = i; r.pad = 0;
            const int64_t per_wave = r.cls == 5 ? 1 : r.cls ? kWave / (2 << r.cls) * kMixGroupRows : 1;
            const int64_t w = (r.rows + per_wave - 1) / per_wave;
            if (w * n_nets > 0x7fffffff / 2 / nb) return fail_arg("%s: too much work for one launch", me);
            A.part_begin = (int32_t)waves;
            A.n_parts = (int32_t)w;
            wave_tensor.insert(wave_tensor.end(), (size_t)w, (int32_t)rows.size());
            rows.push_back(r);
            waves += w;
        }
        if (!clipped && (waves + nchunks) * n_nets > 0x7fffffff / 2 / nb) return fail_arg("%s: too much work for one launch", me);
        alloc.push_back(A);
    }
    if (!clipped) {
        for (BmAllocDev& A : alloc)
            if (A.part_begin < 0) A.part_begin = (int32_t)(waves + (-1 - A.part_begin));
        parts = waves + nchunks;
    }
    const int64_t row_blocks = (waves * n_nets + kBlock / kWave - 1) / (kBlock / kWave);
    if (row_blocks + nchunks * n_nets > 0x7fffffff) return fail_arg("%s: too much work for one launch", me);
    if (clipped && (int64_t)xflats.size() * n_nets > 0x7fffffff) return fail_arg("%s: too much work for one launch", me);

    dfq_batch_mixed_plan* p = new dfq_batch_mixed_plan();
    BmArgs& a = p->args;
    a.bits = bits;
    a.errors = errors;
    a.used = used;
    a.cost = cost;
    a.codes = (unsigned char*)codes;
    a.ranges = ranges;
    a.code_stride = code_stride;
    a.range_stride = range_stride;
    a.budget = cfg.budget_bits;
    for (int j = 0; j < kMixMaxWidths; ++j) a.widths[j] = j < nb ? cfg.widths[j] : 0;
    a.n_widths = nb;
    a.symmetric = cfg.symmetric ? 1 : 0;
    a.code_bytes = cfg.code_bytes;
    a.n_tensors = n_tensors;
    a.row_wpn = (int32_t)waves;
    a.row_waves = (int32_t)(waves * n_nets);
    a.chunks_pn = (int32_t)nchunks;
    a.chunk_blocks = (int32_t)(nchunks * n_nets);
    a.chunk_tensors = (int32_t)chunks.size();
    a.parts_pn = (int32_t)parts;
    p->n_nets = n_nets;
    p->apply = cfg.apply ? 1 : 0;
    p->clipped = clipped;
    BatchUpload up{p->mem};
    a.rows = up.put(rows);
    if (!clipped) a.wave_tensor = up.put(wave_tensor);
    a.chunks = up.put(chunks);
    a.chunk_tensor = up.put(chunk_tensor);
    a.alloc = up.put(alloc);
    a.width_tab = up.put(std::vector<int32_t>(cfg.widths, cfg.widths + nb));
    a.delta = up.put(batch_delta(bases, n_nets));
    a.slots = (uint32_t*)up.raw(nullptr, sizeof(uint32_t) * 2 * (size_t)a.chunk_tensors * n_nets);
    a.partial = (double*)up.raw(nullptr, sizeof(double) * (size_t)a.parts_pn * (size_t)n_nets * (size_t)nb);
    p->state = (int32_t*)up.raw(nullptr, sizeof(int32_t) * (size_t)n_tensors * (size_t)n_nets);
    if (!clipped) {
        p->launches = (chunks.empty() ? 0 : 1) + 2 + p->apply;
    } else {
        BxArgs& x = p->cx;
        const int64_t pieces = (int64_t)piece_tensor.size();
        std::vector<double> alpha(K);
        for (int k = 0; k < K; ++k) alpha[k] = K == 1 ? 1.0 : 1.0 - (double)k * (1.0 - clip->alpha_min) / (double)(K - 1);
        x.rows = up.put(xrows);
        x.wave_tensor = up.put(wave_tensor);
        x.flats = up.put(xflats);
        x.piece_tensor = up.put(piece_tensor);
        x.tensors = up.put(xtensors);
        x.part_tensor = up.put(part_tensor);
        x.width_tab = a.width_tab;
        x.delta = a.delta;
        x.alpha = up.put(alpha);
        p->word_bytes = sizeof(uint32_t) * 2 * xflats.size() * (size_t)n_nets;
        x.words = (uint32_t*)up.raw(nullptr, p->word_bytes);
        x.scratch = (double*)up.raw(nullptr, sizeof(double) * (size_t)pieces * (size_t)n_nets * (size_t)(nb * K));
        x.partial = a.partial;
        x.clip_ranges = clip->clip_ranges;
        x.clip_chosen = clip->clip_chosen;
        x.unit_errors = clip->unit_errors;
        x.bits = bits;
        x.state = p->state;
        x.codes = (unsigned char*)codes;
        x.ranges = ranges;
        x.code_stride = code_stride;
        x.range_stride = range_stride;
        x.unit_stride = clip->unit_stride;
        x.n_widths = nb;
        x.symmetric = a.symmetric;
        x.code_bytes = cfg.code_bytes;
        x.n_tensors = n_tensors;
        x.K = K;
        x.row_wpn = (int32_t)waves;
        x.row_waves = (int32_t)(waves * n_nets);
        x.pieces_pn = (int32_t)pieces;
        x.n_flats = (int32_t)xflats.size();
        x.parts_pn = (int32_t)parts;
        x.n_nets = n_nets;
        p->row_blocks = (int)row_blocks;
        p->piece_blocks = (int)(pieces * n_nets);
        p->fold_blocks = (int)((int64_t)xflats.size() * n_nets);
        p->finish_blocks = (int)((parts * n_nets + kBlock - 1) / kBlock);
        p->launches = (p->piece_blocks ? 3 : 0) + (p->row_blocks ? 1 : 0) + 2 + p->apply * ((p->piece_blocks ? 1 : 0) + (p->row_blocks ? 1 : 0));
    }
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch mixed plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

// ranges, errors, allocation; the plan's state with `keep`
int bm_allocate(dfq_batch_mixed_plan* p, hipStream_t st, bool keep) {
    const BmArgs& a = p->args;
    if (p->clipped) {
        const BxArgs& x = p->cx;
        if (p->piece_blocks > 0) {
            DFQ_HIP_TRY(hipMemsetAsync(x.words, 0, p->word_bytes, st));
            hipLaunchKernelGGL(bx_range_kernel, dim3(p->piece_blocks), dim3(kBlock), 0, st, x);
            DFQ_CHECK_LAUNCH();
            hipLaunchKernelGGL(bx_search_kernel, dim3(p->piece_blocks), dim3(kBlock), 0, st, x);
            DFQ_CHECK_LAUNCH();
            hipLaunchKernelGGL(bx_fold_kernel, dim3(p->fold_blocks), dim3(kWave), 0, st, x);
            DFQ_CHECK_LAUNCH();
        }
        if (p->row_blocks > 0) {
            hipLaunchKernelGGL(bx_row_kernel, dim3(p->row_blocks), dim3(kBlock), 0, st, x);
            DFQ_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(bm_alloc_kernel, dim3(p->n_nets), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
        hipLaunchKernelGGL(bx_finish_kernel, dim3(p->finish_blocks), dim3(kBlock), 0, st, x);
        DFQ_CHECK_LAUNCH();
        p->allocated = true;
        return DFQ_OK;
    }
    if (a.chunk_blocks > 0) {
        DFQ_HIP_TRY(hipMemsetAsync(a.slots, 0, sizeof(uint32_t) * 2 * (size_t)a.chunk_tensors * (size_t)p->n_nets, st));
        hipLaunchKernelGGL(bm_chunk_minmax_kernel, dim3(a.chunk_blocks), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
    }
    const int blocks = a.chunk_blocks + (a.row_waves + kBlock / kWave - 1) / (kBlock / kWave);
    hipLaunchKernelGGL(bm_error_kernel, dim3(blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(bm_alloc_kernel, dim3(p->n_nets), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    if (keep) {
        const int64_t n = (int64_t)p->n_nets * a.n_tensors;
        hipLaunchKernelGGL(bm_state_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.width_tab, a.n_widths, a.bits, p->state,
                           n, 0);
        DFQ_CHECK_LAUNCH();
        p->allocated = true;
    }
    return DFQ_OK;
}

// clamp (clipped plans), or clamp and quantise, at the widths of the plan's state
int bm_apply(dfq_batch_mixed_plan* p, hipStream_t st, bool quantise, bool restore) {
    const BmArgs& a = p->args;
    if (p->clipped) {
        const BxArgs& x = p->cx;
        if (p->piece_blocks > 0) {
            if (quantise) hipLaunchKernelGGL(bx_quant_flat_kernel, dim3(p->piece_blocks), dim3(kBlock), 0, st, x);
            else hipLaunchKernelGGL(bx_clamp_flat_kernel, dim3(p->piece_blocks), dim3(kBlock), 0, st, x);
            DFQ_CHECK_LAUNCH();
        }
        if (p->row_blocks > 0) {
            if (quantise) hipLaunchKernelGGL(bx_quant_kernel, dim3(p->row_blocks), dim3(kBlock), 0, st, x);
            else hipLaunchKernelGGL(bx_clamp_kernel, dim3(p->row_blocks), dim3(kBlock), 0, st, x);
            DFQ_CHECK_LAUNCH();
        }
        return DFQ_OK;
    }
    if (restore) {
        const int64_t n = (int64_t)p->n_nets * a.n_tensors;
        hipLaunchKernelGGL(bm_state_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.width_tab, a.n_widths, a.bits, p->state,
                           n, 1);
        DFQ_CHECK_LAUNCH();
    }
    const int blocks = a.chunk_blocks + (a.row_waves + kBlock / kWave - 1) / (kBlock / kWave);
    hipLaunchKernelGGL(bm_quant_kernel, dim3(blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // namespace

extern "C" {

int32_t dfq_batch_mixed_plan_launches(const dfq_batch_mixed_plan* p) { return p ? p->launches : 0; }

void dfq_batch_mixed_plan_destroy(dfq_batch_mixed_plan* p) { batch_plan_destroy(p); }

int dfq_batch_mixed_plan_create(const dfq_batch_mixed_tensor* tensors, int32_t n_tensors, const dfq_batch_mixed_config* config,
                                const void* const* bases, int32_t n_nets, int32_t* bits, double* errors, int64_t* used, double* cost,
                                void* codes, int64_t code_stride, float* ranges, int64_t range_stride, dfq_batch_mixed_plan** out_plan) {
    return bm_create("dfq_batch_mixed_plan_create", tensors, n_tensors, config, bases, n_nets, bits, errors, used, cost, codes, code_stride,
                     ranges, range_stride, nullptr, false, out_plan);
}

int dfq_batch_mixed_plan_create_clipped(const dfq_batch_mixed_tensor* tensors, int32_t n_tensors, const dfq_batch_mixed_config* config,
                                        const void* const* bases, int32_t n_nets, int32_t* bits, double* errors, int64_t* used, double* cost,
                                        void* codes, int64_t code_stride, float* ranges, int64_t range_stride,
                                        const dfq_batch_mixed_clip* clip, dfq_batch_mixed_plan** out_plan) {
    return bm_create("dfq_batch_mixed_plan_create_clipped", tensors, n_tensors, config, bases, n_nets, bits, errors, used, cost, codes,
                     code_stride, ranges, range_stride, clip, true, out_plan);
}

int dfq_batch_mixed_plan_set_costs(dfq_batch_mixed_plan* p, const double* costs) {
    if (!p) return fail_arg("dfq_batch_mixed_plan_set_costs: null plan");
    p->args.costs = costs;
    return DFQ_OK;
}

int dfq_batch_mixed_plan_run(dfq_batch_mixed_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_mixed_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    if (const int rc = bm_allocate(p, st, false)) return rc;       // (a plan without clipping: its launches as they always were)
    return p->apply ? bm_apply(p, st, true, false) : DFQ_OK;
}

int dfq_batch_mixed_plan_run_stages(dfq_batch_mixed_plan* p, int32_t stages, void* stream) {
    const char* me = "dfq_batch_mixed_plan_run_stages";
    if (!p) return fail_arg("%s: null plan", me);
    const int all = DFQ_MIXED_ALLOCATE | DFQ_MIXED_CLAMP | DFQ_MIXED_QUANTISE;
    if (stages == 0 || (stages & ~all) != 0) return fail_arg("%s: stages %d (a sum of 1, 2 and 4)", me, (int)stages);
    if ((stages & DFQ_MIXED_CLAMP) && !p->clipped) return fail_arg("%s: the clamp stage needs a clipped plan", me);
    if ((stages & (DFQ_MIXED_CLAMP | DFQ_MIXED_QUANTISE)) && !(stages & DFQ_MIXED_ALLOCATE) && !p->allocated) {
        set_error(std::string(me) + ": no allocation stage has run on this plan");
        return DFQ_ERR_STATE;
    }
    hipStream_t st = as_stream(stream);
    if (stages & DFQ_MIXED_ALLOCATE)
        if (const int rc = bm_allocate(p, st, true)) return rc;
    if (stages & DFQ_MIXED_CLAMP)
        if (const int rc = bm_apply(p, st, false, false)) return rc;
    if (stages & DFQ_MIXED_QUANTISE)
        if (const int rc = bm_apply(p, st, true, true)) return rc;
    return DFQ_OK;
}

}  // extern "C"
