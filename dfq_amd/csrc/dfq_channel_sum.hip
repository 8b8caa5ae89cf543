// Per-channel sums of an NCHW activation, for the empirical bias correction on distilled data (improve_dfq.py:311-371): what
// the reference keeps whole per hooked layer, reduces with `outputs.mean(0)`, copies to the host and sums there in float32
// (:349-355, :365) is reduced here in ONE read of the activation, at the moment a forward hook sees it:
//   acc[c] = acc[c] + weight * sum_n sum_hw x[n, c, hw]                  x [N, C, HW] contiguous float32, row r = (n, c) of HW floats
// in float64 from the first addition on.
//
// x is cut into flat pieces of kSumPiece floats, one workgroup each, as bf_stream_kernel / bt_stream_kernel / be_range_kernel
// cut a weight (dfq_fold_batch.hip, dfq_table_batch.hip, dfq_error_batch.hip): a lane issues four 16-byte loads back to back
// whatever HW is, and the row of element e is e / HW -- a [N, C] matrix, 3 x 3 and 7 x 7 maps and 112 x 112 maps take one
// path, and no wave is left with a row of nine floats.  Two launches, no wait inside, no floating-point atomic:
//   1. cs_piece_kernel: the sum of every row over the elements the piece holds of it.
//        a. A lane folds the four elements of a vector into runs of one row.  A row that begins and ends inside the vector
//           is stored to the piece's row table in LDS; `head` is the run of the row the vector starts in, `open` the run
//           that is still open at its end (both the whole vector when no row ends in it).
//        b. The 64 vectors of a wave are consecutive (a "span" of 256 floats; 16 spans per piece, span = load * 4 + wave).
//           A segmented scan over the lanes (be_range_kernel's, with a sum for the (min, max) pair: lane l takes lane
//           l - d's partial iff that lane still lies in the row open at l's end -- a select, never a multiplication by a
//           0 / 1 mask, so a NaN stays in its row) gives every lane the sum of its open row so far; the lane a row ENDS in
//           adds its head run to what the lane before it holds and has the row's sum over the span.
//        c. A row that lies inside one span has one writer: a plain store to the row table.  The first row of a span and
//           the row open at its end may continue in a neighbouring span: they go to the span's two boundary slots (and the
//           up to three single floats behind the last vector of x to three more), which ARE in element order; one thread
//           per slot adds the slots of its row in rising order and the first of them stores the row.
//        d. Rows inside the piece go to row_sum[row] in the scratch; the first and the last row of the piece, which a
//           neighbouring piece may hold a part of, to the piece's two boundary slots there.
//   2. cs_fold_kernel: w lanes per channel, w = the power of two at or above N, at most 64 (a [2, C] matrix does not pay for
//      a wave per channel).  Lane s takes samples s, s + w, ... in rising order; a row's sum is row_sum[row], or its pieces'
//      boundary slots added in rising piece order when it is the first or last row of a piece; a fixed butterfly over the w
//      lanes gives the channel, and one lane adds weight * sum to acc[c].
// Rows of one channel never share a word: with C * HW < kSumPiece a piece holds a channel several times, and every one of
// its rows has its own entry until the fold adds them.  The scratch is 8 B per row plus 16 B per piece; for HW = 1 that is
// 8 B written per 4 B read -- a [N, C] matrix is kilobytes, and from HW = 9 on it is a fifth of the read and falling.
// The order of all additions depends on (N, C, HW) alone: x is 16-byte aligned (refused otherwise; the Python layer copies),
// so its address does not shift the vectors against the rows.
#include "dfq_common.hpp"

namespace dfq {

constexpr int kSumInFlight = 4;                              // 16-byte loads a lane issues before it uses the first
constexpr int kSumPiece = kBlock * 4 * kSumInFlight;         // floats a workgroup reads
constexpr int kSumSpans = kSumInFlight * (kBlock / kWave);   // runs of 64 consecutive vectors in a piece
constexpr int kSumSlots = 2 * kSumSpans + 3;                 // boundary slots of a piece's spans, and x's last single floats

struct CsArgs {
    const float* x;
    double* row_sum;              // [N * C] scratch: rows inside a piece
    double* piece_first;          // [pieces]: what the piece holds of its first row
    double* piece_last;           // [pieces]: ... of its last row, if that is another one
    double* acc;                  // [C]
    double weight;
    int64_t total, n_samples, channels, hw;
};

// launch 1: the piece's share of every row it touches
__global__ __launch_bounds__(kBlock) void cs_piece_kernel(CsArgs a) {
    __shared__ double row_tab[kSumPiece];                        // row first_row + i over this piece (a piece of rows of 1 has kSumPiece)
    __shared__ double slot_sum[kSumSlots];
    __shared__ int slot_row[kSumSlots];                      // row (from first_row) of a boundary slot, -1: unused
    const int t = threadIdx.x;
    const int lane = t % kWave;
    const int64_t start = (int64_t)blockIdx.x * kSumPiece;
    const int count = (int)(a.total - start < kSumPiece ? a.total - start : kSumPiece);
    const int64_t first_row = start / a.hw;
    const uint32_t row_len = (uint32_t)a.hw;
    const uint32_t rem0 = (uint32_t)(start - first_row * a.hw);          // of the piece's first element in its row
    const int n_rows = (int)((rem0 + (uint32_t)count - 1u) / row_len) + 1;
    const int nv = count >> 2;
    const gfloat* x = (const gfloat*)a.x + start;

    // every load of the piece back to back, a lane past the piece's end reading the last vector again (bf_stream_kernel);
    // x may end in up to three single floats, one each for the first lanes
    fvec4 xv[kSumInFlight];
    if (nv > 0) {
#pragma unroll
        for (int j = 0; j < kSumInFlight; ++j) {
            const int v = j * kBlock + t;
            xv[j] = *(const gfvec4*)(x + 4 * (v < nv ? v : nv - 1));
        }
    } else {
#pragma unroll
        for (int j = 0; j < kSumInFlight; ++j) xv[j] = fvec4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    const int tail = (nv << 2) + t;
    const float xt = tail < count ? x[tail] : 0.0f;

    if (t < kSumSlots) slot_row[t] = -1;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSumInFlight; ++j) {
        if (j * kBlock >= nv) break;                         // (workgroup-uniform)
        const int v = j * kBlock + t;
        const bool live = v < nv;
        const int span = j * (kBlock / kWave) + t / kWave;
        const uint32_t e = rem0 + 4u * (uint32_t)v;
        const uint32_t key = e / row_len;                    // the row this vector starts in
        uint32_t rem = e - key * row_len;
        uint32_t r = key;
        double head = 0.0, run = 0.0;
        bool ended = false;                                  // the row the vector starts in ends in it
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            run += (double)xv[j][c];
            if (++rem == row_len) {                          // the row ends behind this element
                rem = 0;
                if (!ended) { head = run; ended = true; }
                else if (live) row_tab[r] = run;             // began and ended in this vector
                ++r;
                run = 0.0;
            }
        }
        if (!ended) head = run;
        // `run` is what the vector holds of row r, the row of the NEXT vector's first element (nothing, 0.0, if a row ends with
        // the vector).  Segmented scan over the lanes that hold a part of that row: they are consecutive, and the first of them
        // is the lane whose vector holds the row's first element (or lane 0)
        const uint32_t wave_e0 = rem0 + 4u * (uint32_t)(v - lane);
        const uint32_t span_row = wave_e0 / row_len;         // the span's first row
        const int64_t ahead = (int64_t)r * row_len - (int64_t)wave_e0;
        const int lane_first = ahead <= 0 ? 0 : (int)(ahead >> 2);
        double open = run;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int src = lane >= d ? lane - d : lane;
            const double o = __shfl(open, src);
            if (lane - d >= lane_first) open += o;
        }
        const double before = __shfl(open, lane > 0 ? lane - 1 : 0);      // of row `key`, in the lanes in front
        if (live) {
            if (ended) {                                     // row `key` ends here: its sum over the span
                const double s = (lane > 0 ? before : 0.0) + head;
                if (key == span_row) { slot_sum[2 * span] = s; slot_row[2 * span] = (int)key; }
                else row_tab[key] = s;
            }
            if ((lane == kWave - 1 || v + 1 >= nv) && rem != 0) {         // the span's last vector leaves row r open
                const int k = 2 * span + (r == span_row ? 0 : 1);
                slot_sum[k] = open;
                slot_row[k] = (int)r;
            }
        }
    }
    if (tail < count) {                                      // (t < 3)
        slot_sum[2 * kSumSpans + t] = (double)xt;
        slot_row[2 * kSumSpans + t] = (int)((rem0 + (uint32_t)tail) / row_len);
    }
    __syncthreads();
    // the slots of one row, in rising order (which is element order), by the thread of the first of them
    double merged = 0.0;
    bool mine = false;
    if (t < kSumSlots) {
        const int row = slot_row[t];
        int first = -1;
#pragma unroll
        for (int q = 0; q < kSumSlots; ++q) {
            if (row >= 0 && slot_row[q] == row) {
                if (first < 0) first = q;
                merged += slot_sum[q];
            }
        }
        mine = first == t;
        if (mine) row_tab[row] = merged;
    }
    __syncthreads();
    for (int i = t; i < n_rows; i += kBlock) {
        const double s = row_tab[i];
        if (i == 0) a.piece_first[blockIdx.x] = s;
        else if (i == n_rows - 1) a.piece_last[blockIdx.x] = s;
        else a.row_sum[first_row + i] = s;
    }
}

// the sum of row r: its entry, or -- for the first or last row of a piece -- the pieces' boundary slots in rising piece order
__device__ __forceinline__ double cs_row_total(const CsArgs& a, int64_t r) {
    const int64_t e0 = r * a.hw, e1 = e0 + a.hw - 1;
    const int64_t p_hi = e1 / kSumPiece;
    double s = 0.0;
    for (int64_t p = e0 / kSumPiece; p <= p_hi; ++p) {
        const int64_t begin = p * kSumPiece;
        const int64_t end = begin + kSumPiece < a.total ? begin + kSumPiece : a.total;
        if (r == begin / a.hw) s += a.piece_first[p];
        else if (r == (end - 1) / a.hw) s += a.piece_last[p];
        else s += a.row_sum[r];                              // (inside its one piece)
    }
    return s;
}

// launch 2: `width` lanes per channel (a power of two, at most a wave), kBlock / width channels per workgroup
__global__ __launch_bounds__(kBlock) void cs_fold_kernel(CsArgs a, int width) {
    const int64_t c = (int64_t)blockIdx.x * (kBlock / width) + threadIdx.x / width;
    const int sub = threadIdx.x % width;
    double s = 0.0;
    if (c < a.channels)
        for (int64_t n = sub; n < a.n_samples; n += width) s += cs_row_total(a, n * a.channels + c);
    for (int d = width >> 1; d > 0; d >>= 1) s += __shfl_xor(s, d);      // (uniform: every lane of the launch takes part)
    if (c < a.channels && sub == 0) a.acc[c] = a.acc[c] + a.weight * s;
}

// improve_dfq.py:361-368: the shift rounded to float32 once, then one float32 subtraction
__global__ __launch_bounds__(kBlock) void bias_sub_delta_kernel(float* bias, const double* acc_q, const double* acc_ref, int64_t channels,
                                                                double scale) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= channels) return;
    const float shift = (float)((acc_q[c] - acc_ref[c]) * scale);
    bias[c] = bias[c] - shift;
}

namespace {

// pieces of a shape, or -1 with the argument error set
int64_t cs_pieces(const char* me, int64_t n_samples, int64_t channels, int64_t hw) {
    if (n_samples <= 0 || channels <= 0 || hw <= 0) {
        fail_arg("%s: a shape of [%lld, %lld, %lld]", me, (long long)n_samples, (long long)channels, (long long)hw);
        return -1;
    }
    if (hw > 0x7fffffff - 4 * kSumPiece || channels > 0x7fffffff || n_samples > INT64_MAX / 16 / channels ||
        n_samples * channels > INT64_MAX / 16 / hw) {
        fail_arg("%s: a shape of [%lld, %lld, %lld] is too large", me, (long long)n_samples, (long long)channels, (long long)hw);
        return -1;
    }
    const int64_t pieces = (n_samples * channels * hw + kSumPiece - 1) / kSumPiece;
    if (pieces > 0x7fffffff) {
        fail_arg("%s: [%lld, %lld, %lld] is more than 2^31 - 1 pieces of %d floats", me, (long long)n_samples, (long long)channels,
                 (long long)hw, kSumPiece);
        return -1;
    }
    return pieces;
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" {

size_t dfq_channel_sum_scratch_bytes(int64_t n_samples, int64_t channels, int64_t hw) {
    const int64_t pieces = cs_pieces("dfq_channel_sum_scratch_bytes", n_samples, channels, hw);
    if (pieces < 0) return 0;
    return sizeof(double) * ((size_t)n_samples * (size_t)channels + 2 * (size_t)pieces);
}

int dfq_channel_sum_accumulate(const float* x, int64_t n_samples, int64_t channels, int64_t hw, double weight, double* acc, void* scratch,
                               void* stream) {
    const char* me = "dfq_channel_sum_accumulate";
    if (!x || !acc || !scratch) return fail_arg("%s: null %s", me, !x ? "x" : !acc ? "acc" : "scratch");
    const int64_t pieces = cs_pieces(me, n_samples, channels, hw);
    if (pieces < 0) return DFQ_ERR_ARG;
    if ((uintptr_t)x % 16 != 0) return fail_arg("%s: x is not 16-byte aligned (the caller copies such a view)", me);
    if ((uintptr_t)acc % 8 != 0 || (uintptr_t)scratch % 8 != 0) return fail_arg("%s: %s is not 8-byte aligned", me, (uintptr_t)acc % 8 ? "acc" : "scratch");
    CsArgs a;
    a.x = x;
    a.row_sum = (double*)scratch;
    a.piece_first = a.row_sum + n_samples * channels;
    a.piece_last = a.piece_first + pieces;
    a.acc = acc;
    a.weight = weight;
    a.total = n_samples * channels * hw;
    a.n_samples = n_samples;
    a.channels = channels;
    a.hw = hw;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(cs_piece_kernel, dim3((unsigned)pieces), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    int width = 1;                                           // lanes per channel: the samples, up to a wave
    while (width < kWave && width < n_samples) width <<= 1;
    const int64_t per_block = kBlock / width;
    hipLaunchKernelGGL(cs_fold_kernel, dim3((unsigned)((channels + per_block - 1) / per_block)), dim3(kBlock), 0, st, a, width);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

int dfq_bias_sub_channel_delta(float* bias, const double* acc_q, const double* acc_ref, int64_t channels, double scale, void* stream) {
    const char* me = "dfq_bias_sub_channel_delta";
    if (!bias || !acc_q || !acc_ref) return fail_arg("%s: null %s", me, !bias ? "bias" : !acc_q ? "acc_q" : "acc_ref");
    if (channels <= 0 || channels > (int64_t)0x7fffffff * kBlock) return fail_arg("%s: %lld channels", me, (long long)channels);
    if ((uintptr_t)bias % 4 != 0) return fail_arg("%s: bias is not 4-byte aligned", me);
    if ((uintptr_t)acc_q % 8 != 0 || (uintptr_t)acc_ref % 8 != 0) return fail_arg("%s: %s is not 8-byte aligned", me, (uintptr_t)acc_q % 8 ? "acc_q" : "acc_ref");
    hipLaunchKernelGGL(bias_sub_delta_kernel, dim3((unsigned)((channels + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), bias,
                       acc_q, acc_ref, channels, scale);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
