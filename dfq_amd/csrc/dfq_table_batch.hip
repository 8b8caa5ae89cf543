// Weight statistics of the ncnn int8 calibration table for a whole batch of networks of one architecture (extension: the
// weight block of model_int8_tensor.table, convert_ncnn.py:178-201, for every network of an arena.NetworkBatch at once).
// The plan holds network 0's tensor table and one byte offset per network, like the other batch plans.  One run reads every
// weight of every network ONCE and writes no weight: per tensor its (min, max) -- what dfq_quant_plan_measure gives -- and
// per output row max|w| -- what dfq_row_range(signed) gives.  Both are selections, no arithmetic: the values are exact.
//
// The caller's float32 block [n_nets, stride] is cleared, then two launches, neither with a wait inside:
//   1. bt_stream_kernel.  A tensor is cut into flat pieces of kTablePiece floats, one workgroup each (batch_piece,
//      dfq_batch_shared.hpp): every lane moves 16 bytes per access whatever the row length, and depthwise rows of 9
//      or the stem's rows of 27 are just elements e with row e / row_len -- 455 rows of 9 to a workgroup, not a wave each.
//      A lane folds the four elements of a vector into runs of one row.  The run its vector STARTS in goes through a
//      segmented max-scan over the wave (wave_head_scan); the last lane of every segment merges it into
//      the piece's row table in LDS.  Runs that start inside a vector (one at most for rows of four elements or more) go to
//      the LDS table directly.  The rows of the piece are then stored; only the first and the last row of a piece can
//      continue in a neighbouring piece, and those two are merged into the block with atomicMax: |w| >= 0, so the bit
//      patterns of the floats order like the floats and the cleared word (+0) is the identity.  The piece's (min, max) is
//      merged into the tensor's two words as ~enc_ord(min), enc_ord(max), the order-preserving words of dfq_quant_batch.hip.
//      Min and max do not depend on the order of the merges: the result is deterministic.
//   2. bt_decode_kernel, a thread per tensor and network: the two merged words become the floats (min, max) in place.
// NaN of either kind is skipped by every min / max (the rule of "Special values", include/dfq_hip.h; range_fold and
// range_fold_abs, dfq_range.hpp); a tensor of nothing but NaN ends as (NaN, NaN), a row of nothing but NaN as 0.
#include <math.h>

#include <vector>

#include "dfq_batch_shared.hpp"
#include "dfq_range.hpp"

namespace dfq {

constexpr int kTableInFlight = kPieceInFlight;                  // 16-byte loads a lane issues before it uses the first
constexpr int kTablePiece = kBatchPiece;                        // floats of one tensor a workgroup reads

struct BtTensorDev {              // a weight of network 0
    const float* w;
    int64_t n;                    // rows * row_len
    int64_t range_off, row_off;   // floats into one network's part of the block
    int32_t row_len, rows;
    int32_t piece_begin;          // first piece (within one network)
    int32_t pad;
};

struct BtArgs {
    const BtTensorDev* tensors;
    const int32_t* piece_tensor;  // tensor of every piece of network 0
    const int64_t* delta;         // bases[n] - bases[0], bytes
    float* out;                   // [n_nets, stride]
    int64_t stride;
    int32_t pieces_pn, n_tensors, n_nets;
};

// launch 1: (min, max) of the piece into its tensor's words, max|w| of every row the piece touches
__global__ __launch_bounds__(kBlock) void bt_stream_kernel(BtArgs a) {
    __shared__ uint32_t row_max[kTablePiece];          // bits of max|w| of row first_row + i (a piece of rows of 1 has kTablePiece)
    BtTensorDev T;
    const BatchPiece p = batch_piece(a.pieces_pn, a.piece_tensor, a.tensors, T);
    const gfloat* w = (const gfloat*)(const float*)((const char*)T.w + a.delta[p.net]) + p.start;
    const int t = threadIdx.x;
    const int lane = t % kWave;
    const int nv = p.nv, n_rows = p.n_rows;
    const uint32_t row_len = p.row_len;
    fvec4 x[kTableInFlight];
    float xt;
    batch_piece_load<false>(p, w, x, xt);
    for (int i = t; i < n_rows; i += kBlock) row_max[i] = 0u;
    __syncthreads();
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kTableInFlight; ++j) {
        if (j * kBlock >= nv) break;                   // (workgroup-uniform)
        const int v = j * kBlock + t;
        const bool live = v < nv;
        const uint32_t e = p.rem0 + 4u * (uint32_t)v;
        const uint32_t key = e / row_len;              // the row this vector starts in
        uint32_t rem = e - key * row_len;
        uint32_t r = key;
        float head[1] = {0.0f}, run = 0.0f;
        bool first = true;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (live) range_fold(x[j][c], mn, mx);
            range_fold_abs(x[j][c], run);
            if (++rem == row_len) {                    // the row ends behind this element
                rem = 0;
                if (first) { head[0] = run; first = false; }
                else if (live) atomicMax(&row_max[r], __float_as_uint(run));
                ++r;
                run = 0.0f;
            }
        }
        if (first) head[0] = run;
        else if (live && rem != 0) atomicMax(&row_max[r], __float_as_uint(run));
        wave_head_scan(p, v, key, head, [](float (&h)[1], const float (&o)[1]) { h[0] = vmax_raw(h[0], o[0]); });
        // the last lane of the segment holds its maximum: r is the row the NEXT lane's vector starts in
        if (live && (lane == kWave - 1 || v + 1 >= nv || r != key)) atomicMax(&row_max[key], __float_as_uint(head[0]));
    }
    const int tail = (nv << 2) + t;
    if (tail < p.count) {
        range_fold(xt, mn, mx);
        float run = 0.0f;
        range_fold_abs(xt, run);
        atomicMax(&row_max[(p.rem0 + (uint32_t)tail) / row_len], __float_as_uint(run));
    }
    block_range(mn, mx);                               // (the row table is complete behind its barrier, too)
    uint32_t* out = (uint32_t*)(a.out + (int64_t)p.net * a.stride);
    if (t == 0) range_publish(mn, mx, out + T.range_off + 0, out + T.range_off + 1);      // (nothing for a piece of NaNs)
    uint32_t* rows = out + T.row_off + p.first_row;
    for (int i = t; i < n_rows; i += kBlock) {
        const uint32_t bits = row_max[i];
        if (i == 0 || i == n_rows - 1) atomicMax(rows + i, bits);      // the two rows a neighbouring piece may hold a part of
        else ((guint*)rows)[i] = bits;
    }
}

// launch 2: the merged words of every tensor and network become (min, max)
__global__ __launch_bounds__(kBlock) void bt_decode_kernel(BtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)a.n_tensors * a.n_nets) return;
    const int net = (int)(i / a.n_tensors);
    const int ti = (int)(i - (int64_t)net * a.n_tensors);
    float* pair = a.out + (int64_t)net * a.stride + a.tensors[ti].range_off;
    const uint32_t lo = ((const guint*)pair)[0], hi = ((const guint*)pair)[1];
    ((gfloat*)pair)[0] = slot_min(lo);
    ((gfloat*)pair)[1] = slot_max(hi);
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_table_plan {
    DevSlab mem;
    BtArgs args{};
    int stream_blocks = 0, decode_blocks = 0;
};

extern "C" {

int32_t dfq_batch_table_plan_launches(const dfq_batch_table_plan* p) { return p ? 2 : 0; }

void dfq_batch_table_plan_destroy(dfq_batch_table_plan* p) { batch_plan_destroy(p); }

int dfq_batch_table_plan_create(const dfq_batch_table_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                                float* out, int64_t stride, dfq_batch_table_plan** out_plan) {
    const char* me = "dfq_batch_table_plan_create";
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (!tensors || n_tensors <= 0) return fail_arg("%s: the tensor table is null or empty (n_tensors %d)", me, (int)n_tensors);
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    for (int n = 1; n < n_nets; ++n)                   // the 16-byte loads of network 0 must be 16-byte loads everywhere
        if (((uintptr_t)bases[n] - (uintptr_t)bases[0]) % 16 != 0) return fail_arg("%s: network %d is not 16-byte aligned to network 0", me, n);
    if (!out || stride <= 0) return fail_arg("%s: the output block is null or empty (stride %lld)", me, (long long)stride);

    std::vector<BtTensorDev> dev;
    std::vector<int32_t> piece_tensor;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_table_tensor& q = tensors[i];
        if (!q.data) return fail_arg("%s: tensor %d: null weight", me, i);
        if (q.rows <= 0 || q.row_len <= 0) return fail_arg("%s: tensor %d: empty shape [%lld, %lld]", me, i, (long long)q.rows, (long long)q.row_len);
        if (q.rows > 0x7fffffff || q.row_len > 0x7fffffff - 2 * kTablePiece || q.rows > INT64_MAX / 2 / q.row_len)
            return fail_arg("%s: tensor %d: a shape of [%lld, %lld]", me, i, (long long)q.rows, (long long)q.row_len);
        if ((uintptr_t)q.data % 16 != 0) return fail_arg("%s: tensor %d: the weight is not 16-byte aligned", me, i);
        if (q.range_offset < 0 || q.range_offset > stride - 2)
            return fail_arg("%s: tensor %d: the (min, max) pair at %lld lies outside the stride %lld", me, i, (long long)q.range_offset, (long long)stride);
        if (q.row_offset < 0 || q.row_offset > stride - q.rows)
            return fail_arg("%s: tensor %d: %lld rows at %lld lie outside the stride %lld", me, i, (long long)q.rows, (long long)q.row_offset,
                            (long long)stride);
        BtTensorDev T{q.data, q.rows * q.row_len, q.range_offset, q.row_offset, (int32_t)q.row_len, (int32_t)q.rows, 0, 0};
        const int64_t begin = batch_add_pieces(piece_tensor, i, T.n, 0x7fffffff / n_nets);
        if (begin < 0) return fail_arg("%s: too much work for one launch", me);
        T.piece_begin = (int32_t)begin;
        dev.push_back(T);
    }
    const int64_t pieces = (int64_t)piece_tensor.size();
    if (stride > INT64_MAX / 4 / n_nets) return fail_arg("%s: a block of %d x %lld floats", me, (int)n_nets, (long long)stride);

    dfq_batch_table_plan* p = new dfq_batch_table_plan();
    BtArgs& a = p->args;
    a.out = out;
    a.stride = stride;
    a.pieces_pn = (int32_t)pieces;
    a.n_tensors = n_tensors;
    a.n_nets = n_nets;
    p->stream_blocks = (int)(pieces * n_nets);
    p->decode_blocks = (int)(((int64_t)n_tensors * n_nets + kBlock - 1) / kBlock);
    BatchUpload up{p->mem};
    a.tensors = up.put(dev);
    a.piece_tensor = up.put(piece_tensor);
    a.delta = up.put(batch_delta(bases, n_nets));
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch table plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_table_plan_run(dfq_batch_table_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_table_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    const BtArgs& a = p->args;
    DFQ_HIP_TRY(hipMemsetAsync(a.out, 0, sizeof(float) * (size_t)a.stride * (size_t)a.n_nets, st));
    hipLaunchKernelGGL(bt_stream_kernel, dim3(p->stream_blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(bt_decode_kernel, dim3(p->decode_blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
