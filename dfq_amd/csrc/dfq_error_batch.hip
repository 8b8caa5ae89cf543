// Weight quantisation error of a whole batch of networks of one architecture (extension: the batch form of
// _quantize_error(param, num_bits, reduction, signed), dfq.py:8-25, for every weight of every network of an
// arena.NetworkBatch and several quantiser configurations at once).  The plan holds network 0's tensor table and one byte
// offset per network, like the other batch plans.  One run reads every weight twice, writes no weight, and leaves per
// network and tensor 1 + 3 * n_configs float64 sums in the caller's block: sum w^2, then per configuration sum e, sum |e|,
// sum e^2 of e = fake_quant_one(w, qparams_double(min, max, bits, symmetric)) - w, the float32 value dfq.py:15 forms and,
// bit for bit, what dfq_batch_quant_plan_run would store minus w ((min, max) of the tensor, or of the row for a per-row
// configuration).
//
// A tensor is cut into flat pieces of kErrPiece floats, one workgroup each (batch_piece, dfq_batch_shared.hpp): a lane issues
// four 16-byte loads back to back whatever the row length, and the row of element e is e / row_len.  The words of the ranges
// are cleared, then three launches, none with a wait inside:
//   1. be_range_kernel: the piece's (min, max) into its tensor's two words, and -- only if a configuration is per row --
//      the (min, max) of every row the piece touches.  The four elements of a vector are folded into runs of one row; the
//      run a vector STARTS in goes through the segmented scan over the wave (wave_head_scan), here of a (min, max) pair, the
//      others into the piece's row table in LDS.  Rows inside the piece are stored, the first and the last row of a piece,
//      which a neighbouring piece may hold a part of, are merged with atomicMax of the order-preserving words ~enc_ord(min),
//      enc_ord(max) (dfq_common.hpp).  min and max do not depend on the order of the merges.
//   2. be_error_kernel reads the piece again and keeps a lane's 16 elements in registers across all configurations.  A
//      per-tensor configuration takes one QParams from the tensor's words.  A per-row one stages {scale, min_value} of the
//      piece's rows in LDS (neg_min is -min_value in both recipes of qparams_double), kErrRowsLds rows at a time: a piece
//      holds more rows than that only for rows of one or two elements, and then a lane's elements of the second half of the
//      rows simply follow those of the first, so the order of the sums is the same.  16 KB of LDS, what the fold kernel has.
//      A lane adds its elements in element order in float64 (e^2 and w^2 formed in float64, where the product of two
//      float32 is exact); block_sum -- wave_sum, then the four waves in fixed order -- gives the piece's sums, which go to
//      the plan's scratch [n_nets, pieces, 1 + 3 * n_configs].
//   3. be_fold_kernel: a thread per network, tensor and value adds the tensor's pieces in rising piece order into the
//      caller's block.
// No floating-point atomic anywhere: two runs are bit-identical, and network n's sums depend on nothing but its weights.
// NaN of either kind is skipped by every range (the rule of "Special values", include/dfq_hip.h; range_fold, dfq_range.hpp); an
// element that is NaN has e = NaN, so a tensor holding one gets NaN sums, in its own slot only.
#include <math.h>

#include <vector>

#include "dfq_batch_shared.hpp"
#include "dfq_range.hpp"

namespace dfq {

constexpr int kErrInFlight = kPieceInFlight;                 // 16-byte loads a lane issues before it uses the first
constexpr int kErrPiece = kBatchPiece;                       // floats of one tensor a workgroup reads
constexpr int kErrRowsLds = 2048;                            // rows whose quantiser parameters are staged at a time
constexpr int kErrMaxConfigs = 4;

struct BeTensorDev {              // a weight of network 0
    const float* w;
    int64_t n;                    // rows * row_len
    int64_t out_off;              // doubles into one network's part of the block
    int64_t row_begin;            // its first row among the rows of one network
    int32_t row_len, rows;
    int32_t piece_begin, n_pieces;   // its pieces (within one network)
};

struct BeArgs {
    const BeTensorDev* tensors;
    const int32_t* piece_tensor;  // tensor of every piece of network 0
    const int64_t* delta;         // bases[n] - bases[0], bytes
    const dfq_batch_error_config* configs;
    uint32_t* tensor_words;       // [n_nets, n_tensors, 2]: ~enc_ord(min), enc_ord(max)
    uint32_t* row_words;          // [n_nets, rows_pn, 2], null without a per-row configuration
    double* partial;              // [n_nets, pieces_pn, n_vals]
    double* out;                  // [n_nets, stride]
    int64_t stride, rows_pn;
    int32_t pieces_pn, n_tensors, n_nets, n_configs, n_vals;
};

// what the kernels share: the piece of this workgroup, its tensor, its first element
struct BePiece : BatchPiece {
    BeTensorDev T;
    const gfloat* w;
};

__device__ __forceinline__ BePiece be_piece(const BeArgs& a) {
    BePiece p;
    (BatchPiece&)p = batch_piece(a.pieces_pn, a.piece_tensor, a.tensors, p.T);
    p.w = (const gfloat*)(const float*)((const char*)p.T.w + a.delta[p.net]) + p.start;
    return p;
}

// launch 1: (min, max) of the piece into its tensor's words and, with a per-row configuration, of every row it touches
__global__ __launch_bounds__(kBlock) void be_range_kernel(BeArgs a) {
    __shared__ uint32_t row_mn[kErrPiece];             // ~enc_ord(min) of row first_row + i (a piece of rows of 1 has kErrPiece)
    __shared__ uint32_t row_mx[kErrPiece];             // enc_ord(max)
    const BePiece p = be_piece(a);
    const int t = threadIdx.x;
    const int lane = t % kWave;
    const int nv = p.nv;
    const uint32_t row_len = p.row_len;
    const bool by_row = a.row_words != nullptr;        // (uniform over the launch)
    fvec4 x[kErrInFlight];
    float xt;
    batch_piece_load<false>(p, p.w, x, xt);
    if (by_row) {
        for (int i = t; i < p.n_rows; i += kBlock) { row_mn[i] = 0u; row_mx[i] = 0u; }
        __syncthreads();
    }
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kErrInFlight; ++j) {
        if (j * kBlock >= nv) break;                   // (workgroup-uniform)
        const int v = j * kBlock + t;
        const bool live = v < nv;
        if (!by_row) {
            if (live) range_fold4(x[j], mn, mx);
            continue;
        }
        const uint32_t e = p.rem0 + 4u * (uint32_t)v;
        const uint32_t key = e / row_len;              // the row this vector starts in
        uint32_t rem = e - key * row_len;
        uint32_t r = key;
        float head[2] = {INFINITY, -INFINITY}, rmn = INFINITY, rmx = -INFINITY;
        bool first = true;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (live) range_fold(x[j][c], mn, mx);
            range_fold(x[j][c], rmn, rmx);
            if (++rem == row_len) {                    // the row ends behind this element
                rem = 0;
                if (first) { head[0] = rmn; head[1] = rmx; first = false; }
                else if (live) range_publish(rmn, rmx, &row_mn[r], &row_mx[r]);
                ++r;
                rmn = INFINITY;
                rmx = -INFINITY;
            }
        }
        if (first) { head[0] = rmn; head[1] = rmx; }
        else if (live && rem != 0) range_publish(rmn, rmx, &row_mn[r], &row_mx[r]);
        wave_head_scan(p, v, key, head, [](float (&h)[2], const float (&o)[2]) { range_merge(h[0], h[1], o[0], o[1]); });
        // the last lane of the segment holds its range: r is the row the NEXT lane's vector starts in
        if (live && (lane == kWave - 1 || v + 1 >= nv || r != key)) range_publish(head[0], head[1], &row_mn[key], &row_mx[key]);
    }
    const int tail = (nv << 2) + t;
    if (tail < p.count) {
        range_fold(xt, mn, mx);
        if (by_row) {
            const uint32_t r = (p.rem0 + (uint32_t)tail) / row_len;
            float tmn = INFINITY, tmx = -INFINITY;
            range_fold(xt, tmn, tmx);
            range_publish(tmn, tmx, &row_mn[r], &row_mx[r]);
        }
    }
    block_range(mn, mx);                               // (the row table is complete behind its barrier, too)
    if (t == 0) {                                      // (nothing for a piece of NaNs)
        uint32_t* words = a.tensor_words + 2 * ((int64_t)p.net * a.n_tensors + p.ti);
        range_publish(mn, mx, words + 0, words + 1);
    }
    if (!by_row) return;
    uint32_t* rows = a.row_words + 2 * ((int64_t)p.net * a.rows_pn + p.T.row_begin + p.first_row);
    for (int i = t; i < p.n_rows; i += kBlock) {
        const uint32_t lo = row_mn[i], hi = row_mx[i];
        if (i == 0 || i == p.n_rows - 1) {             // the two rows a neighbouring piece may hold a part of
            atomicMax(rows + 2 * i + 0, lo);
            atomicMax(rows + 2 * i + 1, hi);
        } else {
            ((guint*)rows)[2 * i + 0] = lo;
            ((guint*)rows)[2 * i + 1] = hi;
        }
    }
}

// one element's error into a lane's three sums
__device__ __forceinline__ void be_add(float w, const QParams& q, double& s, double& sa, double& ss) {
    float code;
    const float e = fake_quant_one(w, q, &code) - w;
    const double d = (double)e;
    s += d;
    sa += (double)fabsf(e);
    ss += d * d;
}

// A lane's elements in element order under one configuration.  PER_ROW: the parameters of row `base + i` are q_scale[i],
// q_minv[i] for i < kErrRowsLds; elements of other rows are left to another call.
template <bool PER_ROW>
__device__ __forceinline__ void be_accumulate(const BePiece& p, const fvec4 (&x)[kErrInFlight], float xt, QParams q, const float* q_scale,
                                              const float* q_minv, uint32_t base, double& s, double& sa, double& ss) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < kErrInFlight; ++j) {
        if (j * kBlock >= p.nv) break;                 // (workgroup-uniform)
        const int v = j * kBlock + t;
        if (v >= p.nv) continue;
        uint32_t r = 0, rem = 0;
        if (PER_ROW) {
            const uint32_t e = p.rem0 + 4u * (uint32_t)v;
            r = e / p.row_len;
            rem = e - r * p.row_len;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (PER_ROW) {
                const uint32_t i = r - base;
                if (++rem == p.row_len) { rem = 0; ++r; }
                if (i >= (uint32_t)kErrRowsLds) continue;
                q.scale = q_scale[i];
                q.min_value = q_minv[i];
                q.neg_min = -q.min_value;
            }
            be_add(x[j][c], q, s, sa, ss);
        }
    }
    const int tail = (p.nv << 2) + t;
    if (tail < p.count) {
        if (PER_ROW) {
            const uint32_t i = (p.rem0 + (uint32_t)tail) / p.row_len - base;
            if (i >= (uint32_t)kErrRowsLds) return;
            q.scale = q_scale[i];
            q.min_value = q_minv[i];
            q.neg_min = -q.min_value;
        }
        be_add(xt, q, s, sa, ss);
    }
}

// launch 2: the piece's sums under every configuration
__global__ __launch_bounds__(kBlock) void be_error_kernel(BeArgs a) {
    __shared__ float q_scale[kErrRowsLds];             // of row first_row + base + i under the configuration at hand
    __shared__ float q_minv[kErrRowsLds];
    __shared__ double sh[kBlock / kWave];
    const BePiece p = be_piece(a);
    const int t = threadIdx.x;
    fvec4 x[kErrInFlight];
    float xt;
    batch_piece_load<false>(p, p.w, x, xt);
    double* part = a.partial + ((int64_t)p.net * a.pieces_pn + p.lp) * a.n_vals;
    {
        double sw = 0.0;
#pragma unroll
        for (int j = 0; j < kErrInFlight; ++j) {
            if (j * kBlock + t < p.nv) {
#pragma unroll
                for (int c = 0; c < 4; ++c) sw += (double)x[j][c] * (double)x[j][c];
            }
        }
        if ((p.nv << 2) + t < p.count) sw += (double)xt * (double)xt;
        sw = block_sum(sw, sh);
        if (t == 0) part[0] = sw;
    }
    const uint32_t* words = a.tensor_words + 2 * ((int64_t)p.net * a.n_tensors + p.ti);
    const float tmn = slot_min(words[0]), tmx = slot_max(words[1]);
    const uint32_t* rows = a.row_words ? a.row_words + 2 * ((int64_t)p.net * a.rows_pn + p.T.row_begin + p.first_row) : nullptr;
    for (int c = 0; c < a.n_configs; ++c) {
        const dfq_batch_error_config cfg = a.configs[c];
        double s = 0.0, sa = 0.0, ss = 0.0;
        if (!cfg.per_row) {                            // (uniform over the launch)
            const QParams q = qparams_double((double)tmn, (double)tmx, cfg.num_bits, cfg.symmetric);
            be_accumulate<false>(p, x, xt, q, nullptr, nullptr, 0u, s, sa, ss);
        } else {
            QParams q = qparams_double(0.0, 1.0, cfg.num_bits, cfg.symmetric);      // qmin and qmax; the rest comes per row
            for (int base = 0; base < p.n_rows; base += kErrRowsLds) {
                __syncthreads();                       // the table may still be read for the rows before
                for (int i = t; i < kErrRowsLds && base + i < p.n_rows; i += kBlock) {
                    const QParams rq = qparams_double((double)slot_min(rows[2 * (base + i) + 0]), (double)slot_max(rows[2 * (base + i) + 1]),
                                                      cfg.num_bits, cfg.symmetric);
                    q_scale[i] = rq.scale;
                    q_minv[i] = rq.min_value;
                }
                __syncthreads();
                be_accumulate<true>(p, x, xt, q, q_scale, q_minv, (uint32_t)base, s, sa, ss);
            }
        }
        s = block_sum(s, sh);
        sa = block_sum(sa, sh);
        ss = block_sum(ss, sh);
        if (t == 0) {
            part[1 + 3 * c + 0] = s;
            part[1 + 3 * c + 1] = sa;
            part[1 + 3 * c + 2] = ss;
        }
    }
}

// launch 3: a tensor's pieces, in rising order, into the caller's block
__global__ __launch_bounds__(kBlock) void be_fold_kernel(BeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t per_net = (int64_t)a.n_tensors * a.n_vals;
    if (i >= per_net * a.n_nets) return;
    const int net = (int)(i / per_net);
    const int rest = (int)(i - net * per_net);
    const int ti = rest / a.n_vals;
    const int k = rest - ti * a.n_vals;
    const BeTensorDev T = a.tensors[ti];
    const double* part = a.partial + ((int64_t)net * a.pieces_pn + T.piece_begin) * a.n_vals + k;
    double s = 0.0;
    for (int q = 0; q < T.n_pieces; ++q) s += part[(int64_t)q * a.n_vals];
    a.out[(int64_t)net * a.stride + T.out_off + k] = s;
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_error_plan {
    DevSlab mem;
    BeArgs args{};
    size_t word_bytes = 0;
    int piece_blocks = 0, fold_blocks = 0;
};

extern "C" {

int32_t dfq_batch_error_plan_launches(const dfq_batch_error_plan* p) { return p ? 3 : 0; }

void dfq_batch_error_plan_destroy(dfq_batch_error_plan* p) { batch_plan_destroy(p); }

int dfq_batch_error_plan_create(const dfq_batch_error_tensor* tensors, int32_t n_tensors, const dfq_batch_error_config* configs,
                                int32_t n_configs, const void* const* bases, int32_t n_nets, double* out, int64_t stride,
                                dfq_batch_error_plan** out_plan) {
    const char* me = "dfq_batch_error_plan_create";
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (!tensors || n_tensors <= 0) return fail_arg("%s: the tensor table is null or empty (n_tensors %d)", me, (int)n_tensors);
    if (!configs || n_configs < 1 || n_configs > kErrMaxConfigs)
        return fail_arg("%s: the configuration table is null or holds %d entries (1..%d)", me, (int)n_configs, kErrMaxConfigs);
    bool by_row = false;
    std::vector<dfq_batch_error_config> cfg(configs, configs + n_configs);
    for (int c = 0; c < n_configs; ++c) {
        dfq_batch_error_config& q = cfg[c];
        const int lo = q.per_row ? 2 : 1, hi = q.per_row ? 16 : 30;
        if (q.num_bits < lo || q.num_bits > hi)
            return fail_arg("%s: configuration %d: num_bits %d outside [%d, %d] (%s)", me, c, (int)q.num_bits, lo, hi, q.per_row ? "per row" : "per tensor");
        if (q.symmetric && q.num_bits == 1)
            return fail_arg("%s: configuration %d: symmetric with num_bits=1 has qmax = 0 (the scale would be max / 0)", me, c);
        q.symmetric = q.symmetric ? 1 : 0;
        q.per_row = q.per_row ? 1 : 0;
        q.pad = 0;
        by_row = by_row || q.per_row;
    }
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    for (int n = 1; n < n_nets; ++n)                   // the 16-byte loads of network 0 must be 16-byte loads everywhere
        if (((uintptr_t)bases[n] - (uintptr_t)bases[0]) % 16 != 0) return fail_arg("%s: network %d is not 16-byte aligned to network 0", me, n);
    if (!out || stride <= 0) return fail_arg("%s: the output block is null or empty (stride %lld)", me, (long long)stride);
    const int n_vals = 1 + 3 * n_configs;

    std::vector<BeTensorDev> dev;
    std::vector<int32_t> piece_tensor;
    int64_t rows_pn = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_error_tensor& q = tensors[i];
        if (!q.data) return fail_arg("%s: tensor %d: null weight", me, i);
        if (q.rows <= 0 || q.row_len <= 0) return fail_arg("%s: tensor %d: empty shape [%lld, %lld]", me, i, (long long)q.rows, (long long)q.row_len);
        if (q.rows > 0x7fffffff || q.row_len > 0x7fffffff - 2 * kErrPiece || q.rows > INT64_MAX / 2 / q.row_len)
            return fail_arg("%s: tensor %d: a shape of [%lld, %lld]", me, i, (long long)q.rows, (long long)q.row_len);
        if ((uintptr_t)q.data % 16 != 0) return fail_arg("%s: tensor %d: the weight is not 16-byte aligned", me, i);
        if (q.out_offset < 0 || q.out_offset > stride - n_vals)
            return fail_arg("%s: tensor %d: %d sums at %lld lie outside the stride %lld", me, i, n_vals, (long long)q.out_offset, (long long)stride);
        BeTensorDev T{q.data, q.rows * q.row_len, q.out_offset, rows_pn, (int32_t)q.row_len, (int32_t)q.rows, 0, 0};
        const int64_t begin = batch_add_pieces(piece_tensor, i, T.n, 0x7fffffff / n_nets / n_vals);
        rows_pn += q.rows;
        if (begin < 0 || rows_pn > INT64_MAX / 16 / n_nets) return fail_arg("%s: too much work for one launch", me);
        T.piece_begin = (int32_t)begin;
        T.n_pieces = (int32_t)((int64_t)piece_tensor.size() - begin);
        dev.push_back(T);
    }
    const int64_t pieces = (int64_t)piece_tensor.size();
    if (stride > INT64_MAX / 8 / n_nets) return fail_arg("%s: a block of %d x %lld doubles", me, (int)n_nets, (long long)stride);

    dfq_batch_error_plan* p = new dfq_batch_error_plan();
    BeArgs& a = p->args;
    a.out = out;
    a.stride = stride;
    a.rows_pn = rows_pn;
    a.pieces_pn = (int32_t)pieces;
    a.n_tensors = n_tensors;
    a.n_nets = n_nets;
    a.n_configs = n_configs;
    a.n_vals = n_vals;
    p->piece_blocks = (int)(pieces * n_nets);
    p->fold_blocks = (int)(((int64_t)n_tensors * n_vals * n_nets + kBlock - 1) / kBlock);
    BatchUpload up{p->mem};
    a.tensors = up.put(dev);
    a.piece_tensor = up.put(piece_tensor);
    a.delta = up.put(batch_delta(bases, n_nets));
    a.configs = up.put(cfg);
    // the words of the tensors and, behind them, of the rows: one clear per run
    const size_t tensor_words = 2 * (size_t)n_tensors * (size_t)n_nets;
    const size_t row_words = by_row ? 2 * (size_t)rows_pn * (size_t)n_nets : 0;
    p->word_bytes = sizeof(uint32_t) * (tensor_words + row_words);
    a.tensor_words = (uint32_t*)up.raw(nullptr, p->word_bytes);
    a.row_words = by_row && a.tensor_words ? a.tensor_words + tensor_words : nullptr;
    a.partial = (double*)up.raw(nullptr, sizeof(double) * (size_t)pieces * (size_t)n_nets * (size_t)n_vals);
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch error plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_error_plan_run(dfq_batch_error_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_error_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    const BeArgs& a = p->args;
    DFQ_HIP_TRY(hipMemsetAsync(a.tensor_words, 0, p->word_bytes, st));
    hipLaunchKernelGGL(be_range_kernel, dim3(p->piece_blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(be_error_kernel, dim3(p->piece_blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(be_fold_kernel, dim3(p->fold_blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
