// Weight quantisation of a whole batch of networks of one architecture (extension: quantize_targ_layer,
// layer_transform.py:279-296, for every network of an arena.NetworkBatch at once).  The plan holds network 0's tensor table
// and one byte offset per network, like the replicated LE / BC plans; the arithmetic is the per-network plans' --
// qparams_double + fake_quant_one on the same (min, max) -- so every weight, code and range is bit-identical to
// dfq_row_quant_plan_run (per row) and dfq_quant_plan_run (per tensor).
//
// Per row: a row gets L lanes, L in {4, 8, 16, 32, 64} chosen per tensor from its row length, so one wave covers 64 / L rows
// at a time (16 depthwise rows of 9, where row_seg_quant_kernel spends a wave on each), and kGroupRows such sets of rows
// below L = 64.  A lane keeps its share of the row in registers
// between the min/max and the quantisation: every element is read once and written once, plus its code.  The group's
// reduction is xor_lane_minmax<M> for M < L (DPP / v_permlane*_swap, no LDS).  Rows longer than kRegElems loop, one wave per
// row, and read the row twice.  A per-tensor tensor of at most kRegElems elements is a single such row.
// Per tensor, longer: a min/max launch folds every chunk of kChunkQ elements into its tensor's pair of order-preserving slots
// (atomicMax of enc_ord, as dfq_quant_plan does; the slots are cleared in front of it), the quantising launch reads the pair.
// No workgroup ever waits for another one of its launch.  NaN of either kind is skipped by every range (the rule of "Special
// values", include/dfq_hip.h; range_fold, dfq_range.hpp).
// Work is found from tables of ONE network: wave -> (network, wave of network 0) by a division, then the wave's tensor from a
// table of network 0's waves (one load; a binary search over the tensors cost a chain of dependent loads per wave).
#include <vector>

#include "dfq_batch_shared.hpp"
#include "dfq_range.hpp"

namespace dfq {

constexpr int kRegPerLane = 24;                        // register slots per lane of the 64-lane class (32: scalar spills)
constexpr int64_t kRegElems = (int64_t)kWave * kRegPerLane;   // longest row kept in registers
constexpr int kSmallPerLane = 4;                       // the classes L < 64 hold rows of at most 4 L elements,
constexpr int kGroupRows = 4;                          // kGroupRows of them per lane group
constexpr int kChunkPerThread = 16;
constexpr int kChunkQ = kBlock * kChunkPerThread;      // elements of a per-tensor tensor one workgroup owns

typedef DFQ_GLOBAL_AS int32_t gint32;
typedef DFQ_GLOBAL_AS uint8_t guint8;

struct BqRowDev {                 // a tensor quantised row by row (a per-tensor one of <= kRegElems elements: one row)
    float* data;                  // network 0
    int64_t code_off, range_off;  // into one network's block, -1 = none
    int32_t rows, len;
    int32_t num_bits, symmetric;
    int32_t cls;                  // 0: one wave per row, looping; c > 0: L = 2 << c lanes per row
    int32_t wave_begin;           // first wave (within one network)
};

struct BqChunkDev {               // a per-tensor tensor of more than kRegElems elements
    float* data;
    int64_t code_off, range_off;
    int64_t n;
    int32_t num_bits, symmetric;
    int32_t chunk_begin, n_chunks;   // its chunks within one network
};

struct BqArgs {
    const BqRowDev* rows;
    const int32_t* wave_tensor;   // row tensor of every wave of network 0
    const BqChunkDev* chunks;
    const int32_t* chunk_tensor;  // chunk tensor of every chunk of network 0
    const int64_t* delta;         // bases[n] - bases[0], bytes
    uint32_t* slots;              // [n_nets, chunk_tensors, 2]: ~enc_ord(min), enc_ord(max) (dfq_common.hpp)
    unsigned char* codes;
    float* ranges;
    int64_t code_stride, range_stride;
    int32_t code_bytes;
    int32_t row_wpn, row_waves;
    int32_t chunks_pn, chunk_blocks, chunk_tensors;
};

__device__ __forceinline__ void bq_store_code(unsigned char* codes, int code_bytes, int64_t i, float code) {
    if (code_bytes == 4) ((gint32*)codes)[i] = (int32_t)code;
    else ((guint8*)codes)[i] = (uint8_t)(int32_t)code;   // the int32 code's low byte: uint8 (asymmetric) / int8 (symmetric)
}

// R sets of 64 / L rows of one tensor from first_row on (row first_row + j * 64 / L + lane / L), L lanes each, K register slots
// per lane and row (len <= K * L)
template <int L, int K, int R>
__device__ __forceinline__ void bq_rows(const BqRowDev& T, float* x, unsigned char* codes, int code_bytes, float* ranges, int first_row) {
    constexpr int G = kWave / L;
    const int lane = threadIdx.x % kWave;
    const int g = lane % L;
    const int r0 = first_row + lane / L;
    const int len = T.len;
    gfloat* xr0 = (gfloat*)x;
    // every load of the rows first, the min/max after them: a fold next to each load made every load wait for the one
    // before it (the wave-uniform exits split the loop into blocks the scheduler does not move loads across)
    float v[R][K];
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
        if (ranges && g == 0) { ((gfloat*)ranges)[2 * r + 0] = mn; ((gfloat*)ranges)[2 * r + 1] = mx; }
        const QParams p = qparams_double((double)mn, (double)mx, T.num_bits, T.symmetric);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k * L >= len) break;
            const int i = g + k * L;
            if (i < len) {
                float code;
                xr0[(int64_t)r * len + i] = fake_quant_one(v[j][k], p, &code);
                if (codes) bq_store_code(codes, code_bytes, (int64_t)r * len + i, code);
            }
        }
    }
}

// one row longer than kRegElems: one wave, the row read twice (the second time from the cache)
__device__ __forceinline__ void bq_long_row(const BqRowDev& T, float* x, unsigned char* codes, int code_bytes, float* ranges, int r) {
    const int lane = threadIdx.x % kWave;
    const int len = T.len;
    gfloat* xr = (gfloat*)x + (int64_t)r * len;
    float mn, mx;
    wave_row_range(xr, len, mn, mx);
    if (ranges && lane == 0) { ((gfloat*)ranges)[2 * r + 0] = mn; ((gfloat*)ranges)[2 * r + 1] = mx; }
    const QParams p = qparams_double((double)mn, (double)mx, T.num_bits, T.symmetric);
    for (int i = lane; i < len; i += kWave) {
        float code;
        xr[i] = fake_quant_one(xr[i], p, &code);
        if (codes) bq_store_code(codes, code_bytes, (int64_t)r * len + i, code);
    }
}

// launch 1 (only with per-tensor tensors longer than kRegElems): every chunk of every network folded into its tensor's slots
__global__ __launch_bounds__(kBlock) void bq_chunk_minmax_kernel(BqArgs a) {
    const int net = (int)blockIdx.x / a.chunks_pn;
    const int c = (int)blockIdx.x - net * a.chunks_pn;
    const int t = a.chunk_tensor[c];
    const BqChunkDev T = a.chunks[t];
    const gfloat* x = (const gfloat*)(const float*)((const char*)T.data + a.delta[net]);
    const int64_t b = (int64_t)(c - T.chunk_begin) * kChunkQ;
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kChunkPerThread; ++j) {
        const int64_t i = b + j * kBlock + threadIdx.x;
        if (i < T.n) range_fold(x[i], mn, mx);
    }
    block_range(mn, mx);
    if (threadIdx.x == 0) {                            // (nothing for a chunk of NaNs)
        uint32_t* slot = a.slots + 2 * ((int64_t)net * a.chunk_tensors + t);
        range_publish(mn, mx, slot + 0, slot + 1);
    }
}

// launch 2: the chunks of the long per-tensor tensors (their tensor's range from its slots), then the row groups
__global__ __launch_bounds__(kBlock) void bq_quant_kernel(BqArgs a) {
    if ((int)blockIdx.x < a.chunk_blocks) {            // (block-uniform)
        const int net = (int)blockIdx.x / a.chunks_pn;
        const int c = (int)blockIdx.x - net * a.chunks_pn;
        const int t = a.chunk_tensor[c];
        const BqChunkDev T = a.chunks[t];
        const uint32_t* slot = a.slots + 2 * ((int64_t)net * a.chunk_tensors + t);
        const float mn = slot_min(slot[0]);
        const float mx = slot_max(slot[1]);
        const int ci = c - T.chunk_begin;
        if (ci == 0 && threadIdx.x == 0 && T.range_off >= 0) {
            gfloat* rg = (gfloat*)a.ranges + (int64_t)net * a.range_stride + T.range_off;
            rg[0] = mn;
            rg[1] = mx;
        }
        const QParams p = qparams_double((double)mn, (double)mx, T.num_bits, T.symmetric);
        gfloat* x = (gfloat*)(float*)((char*)T.data + a.delta[net]);
        unsigned char* codes = T.code_off >= 0 ? a.codes + ((int64_t)net * a.code_stride + T.code_off) * a.code_bytes : nullptr;
        const int64_t b = (int64_t)ci * kChunkQ;
        float v[kChunkPerThread];
#pragma unroll
        for (int j = 0; j < kChunkPerThread; ++j) {
            const int64_t i = b + j * kBlock + threadIdx.x;
            v[j] = i < T.n ? x[i] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < kChunkPerThread; ++j) {
            const int64_t i = b + j * kBlock + threadIdx.x;
            if (i < T.n) {
                float code;
                x[i] = fake_quant_one(v[j], p, &code);
                if (codes) bq_store_code(codes, a.code_bytes, i, code);
            }
        }
        return;
    }
    const int w = ((int)blockIdx.x - a.chunk_blocks) * (kBlock / kWave) + (int)threadIdx.x / kWave;
    if (w >= a.row_waves) return;                      // (wave-uniform)
    const int net = w / a.row_wpn;
    const int lw = w - net * a.row_wpn;
    const BqRowDev T = a.rows[a.wave_tensor[lw]];
    float* x = (float*)((char*)T.data + a.delta[net]);
    unsigned char* codes = T.code_off >= 0 ? a.codes + ((int64_t)net * a.code_stride + T.code_off) * a.code_bytes : nullptr;
    float* ranges = T.range_off >= 0 ? a.ranges + (int64_t)net * a.range_stride + T.range_off : nullptr;
    const int wi = lw - T.wave_begin;
    switch (T.cls) {
        case 1: bq_rows<4, kSmallPerLane, kGroupRows>(T, x, codes, a.code_bytes, ranges, wi * 16 * kGroupRows); break;
        case 2: bq_rows<8, kSmallPerLane, kGroupRows>(T, x, codes, a.code_bytes, ranges, wi * 8 * kGroupRows); break;
        case 3: bq_rows<16, kSmallPerLane, kGroupRows>(T, x, codes, a.code_bytes, ranges, wi * 4 * kGroupRows); break;
        case 4: bq_rows<32, kSmallPerLane, kGroupRows>(T, x, codes, a.code_bytes, ranges, wi * 2 * kGroupRows); break;
        case 5: bq_rows<64, kRegPerLane, 1>(T, x, codes, a.code_bytes, ranges, wi); break;
        default: bq_long_row(T, x, codes, a.code_bytes, ranges, wi); break;
    }
}

// lane class of a row of `len` elements: the fewest lanes that hold it in kSmallPerLane slots, 64 up to kRegElems, else 0
inline int bq_class(int len) {
    for (int c = 1; c <= 4; ++c)
        if (len <= (int64_t)(2 << c) * kSmallPerLane) return c;
    return len <= kRegElems ? 5 : 0;
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_quant_plan {
    DevSlab mem;
    BqArgs args{};
    int launches = 1;
};

extern "C" {

int64_t dfq_batch_quant_register_elements(void) { return kRegElems; }

int32_t dfq_batch_quant_plan_launches(const dfq_batch_quant_plan* p) { return p ? p->launches : 0; }

void dfq_batch_quant_plan_destroy(dfq_batch_quant_plan* p) { batch_plan_destroy(p); }

int dfq_batch_quant_plan_create(const dfq_batch_quant_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                                void* codes, int32_t code_bytes, int64_t code_stride, float* ranges, int64_t range_stride,
                                dfq_batch_quant_plan** out_plan) {
    const char* me = "dfq_batch_quant_plan_create";
    if (!tensors || n_tensors <= 0 || !out_plan) return fail_arg("%s: no tensors", me);
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    if (code_stride < 0 || range_stride < 0) return fail_arg("%s: negative stride", me);
    std::vector<BqRowDev> rows;
    std::vector<BqChunkDev> chunks;
    std::vector<int32_t> wave_tensor, chunk_tensor;
    int64_t waves = 0, nchunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_quant_tensor& t = tensors[i];
        if (!t.data || t.rows <= 0 || t.row_len <= 0 || t.row_len > INT64_MAX / 2 / t.rows)
            return fail_arg("%s: tensor %d is empty", me, i);
        const int64_t numel = t.rows * t.row_len;
        const int lo = t.per_row ? 2 : 1, hi = t.per_row ? 16 : 30;
        if (t.num_bits < lo || t.num_bits > hi)
            return fail_arg("%s: tensor %d: num_bits %d outside [%d, %d] (%s)", me, i, (int)t.num_bits, lo, hi, t.per_row ? "per row" : "per tensor");
        if (t.symmetric && t.num_bits == 1) return fail_arg("%s: tensor %d: symmetric with num_bits=1 has qmax = 0 (the scale would be max / 0)", me, i);
        if (t.code_offset < -1 || t.range_offset < -1) return fail_arg("%s: tensor %d: negative offset", me, i);
        if (t.code_offset >= 0) {
            if (!codes) return fail_arg("%s: tensor %d writes codes, but the code block is null", me, i);
            if (code_bytes != 1 && code_bytes != 4) return fail_arg("%s: code width %d bytes (1 or 4)", me, (int)code_bytes);
            if (code_bytes == 1 && t.num_bits > 8) return fail_arg("%s: tensor %d: 1-byte codes of %d bits", me, i, (int)t.num_bits);
            if (t.code_offset > code_stride - numel) return fail_arg("%s: tensor %d: codes overflow the code stride", me, i);
        }
        const int64_t n_ranges = 2 * (t.per_row ? t.rows : 1);
        if (t.range_offset >= 0) {
            if (!ranges) return fail_arg("%s: tensor %d writes ranges, but the range block is null", me, i);
            if (t.range_offset > range_stride - n_ranges) return fail_arg("%s: tensor %d: ranges overflow the range stride", me, i);
        }
        if (!t.per_row && numel > kRegElems) {
            BqChunkDev c;
            c.data = t.data; c.code_off = t.code_offset; c.range_off = t.range_offset; c.n = numel;
            c.num_bits = t.num_bits; c.symmetric = t.symmetric ? 1 : 0;
            c.chunk_begin = (int32_t)nchunks;
            const int64_t k = (numel + kChunkQ - 1) / kChunkQ;
            c.n_chunks = (int32_t)k;
            if (k * n_nets > 0x7fffffff / 2) return fail_arg("%s: too much work for one launch", me);
            chunk_tensor.insert(chunk_tensor.end(), (size_t)k, (int32_t)chunks.size());
            chunks.push_back(c);
            nchunks += k;
        } else {
            BqRowDev r;
            r.data = t.data; r.code_off = t.code_offset; r.range_off = t.range_offset;
            const int64_t rr = t.per_row ? t.rows : 1, len = t.per_row ? t.row_len : numel;
            if (rr > 0x7fffffff - kWave || len > 0x7fffffff - kWave) return fail_arg("%s: tensor %d: too many rows or a row too long", me, i);
            r.rows = (int32_t)rr;
            r.len = (int32_t)len;
            r.num_bits = t.num_bits; r.symmetric = t.symmetric ? 1 : 0;
            r.cls = bq_class(r.len);
            r.wave_begin = (int32_t)waves;
            const int64_t per_wave = r.cls == 5 ? 1 : r.cls ? kWave / (2 << r.cls) * kGroupRows : 1;
            const int64_t w = (r.rows + per_wave - 1) / per_wave;
            if (w * n_nets > 0x7fffffff) return fail_arg("%s: too much work for one launch", me);
            wave_tensor.insert(wave_tensor.end(), (size_t)w, (int32_t)rows.size());
            rows.push_back(r);
            waves += w;
        }
        if (waves * n_nets > 0x7fffffff - kBlock || nchunks * n_nets > 0x7fffffff / 2)
            return fail_arg("%s: too much work for one launch", me);
    }
    const int64_t row_blocks = (waves * n_nets + kBlock / kWave - 1) / (kBlock / kWave);
    if (row_blocks + nchunks * n_nets > 0x7fffffff) return fail_arg("%s: too much work for one launch", me);

    dfq_batch_quant_plan* p = new dfq_batch_quant_plan();
    BqArgs& a = p->args;
    a.codes = (unsigned char*)codes;
    a.ranges = ranges;
    a.code_stride = code_stride;
    a.range_stride = range_stride;
    a.code_bytes = code_bytes;
    a.row_wpn = (int32_t)waves;
    a.row_waves = (int32_t)(waves * n_nets);
    a.chunks_pn = (int32_t)nchunks;
    a.chunk_blocks = (int32_t)(nchunks * n_nets);
    a.chunk_tensors = (int32_t)chunks.size();
    p->launches = chunks.empty() ? 1 : 2;
    BatchUpload up{p->mem};
    a.rows = up.put(rows);
    a.wave_tensor = up.put(wave_tensor);
    a.chunks = up.put(chunks);
    a.chunk_tensor = up.put(chunk_tensor);
    a.delta = up.put(batch_delta(bases, n_nets));
    a.slots = (uint32_t*)up.raw(nullptr, sizeof(uint32_t) * 2 * (size_t)a.chunk_tensors * n_nets);
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch quant plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_quant_plan_run(dfq_batch_quant_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_quant_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    const BqArgs& a = p->args;
    if (a.chunk_blocks > 0) {
        DFQ_HIP_TRY(hipMemsetAsync(a.slots, 0, sizeof(uint32_t) * 2 * (size_t)a.chunk_tensors * (size_t)(a.chunk_blocks / a.chunks_pn), st));
        hipLaunchKernelGGL(bq_chunk_minmax_kernel, dim3(a.chunk_blocks), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
    }
    const int blocks = a.chunk_blocks + (a.row_waves + kBlock / kWave - 1) / (kBlock / kWave);
    hipLaunchKernelGGL(bq_quant_kernel, dim3(blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
