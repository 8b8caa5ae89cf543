// BatchNorm folding of a whole batch of networks of one architecture (extension: merge_batchnorm,
// utils/layer_transform.py:246-272, for every network of an arena.NetworkBatch at once).  The plan holds network 0's pair
// table and one byte offset per network, like the other batch plans; the arithmetic is dfq_fold_batchnorm's
// (bn_fold_vec_kernel + scale_rows_kernel op 0, dfq_misc.hip), operation for operation, so every weight, bias, proxy and
// BatchNorm vector is bit-identical to that call on each network alone.
//
// Two launches, neither with a wait inside, no atomics:
//   1. bf_stream_kernel reads and writes every folded weight once.  A tensor is cut into flat pieces of kFoldPiece floats,
//      one workgroup each (batch_piece, dfq_batch_shared.hpp): the row of element e is e / row_len, so depthwise rows of 9,
//      the stem's rows of 27 and rows longer than a piece all take the same path and every lane moves 16 bytes at a time
//      whatever the row length.  The
//      piece's k = gamma / sqrtf(var + eps) -- one per row it touches, at most kFoldPiece of them -- are recomputed into LDS
//      while the piece's loads are in flight.  gamma and var are only READ in this launch.
//   2. bf_vec_kernel, a thread per channel of every pair and network: the bias update, the proxies, the identity BatchNorm.
//      It is the only writer of gamma / var, and stream order puts it behind every reader.
#include <math.h>

#include <vector>

#include "dfq_batch_shared.hpp"

namespace dfq {

constexpr int kFoldInFlight = kPieceInFlight;                   // 16-byte loads a lane issues before it uses the first
constexpr int kFoldPiece = kBatchPiece;                         // floats of one tensor a workgroup scales

struct BfPairDev {                // a (layer, BatchNorm) pair of network 0
    float *w, *b, *gamma, *beta, *mean, *var, *fake_weight, *fake_bias;
    int64_t n;                    // out_ch * row_len
    int32_t row_len, out_ch;
    float eps;
    int32_t piece_begin;          // first piece (within one network)
    int32_t chan_begin;           // first channel (within one network)
};

struct BfArgs {
    const BfPairDev* pairs;
    const int32_t* piece_pair;    // pair of every piece of network 0
    const int32_t* chan_pair;     // pair of every channel of network 0
    const int64_t* delta;         // bases[n] - bases[0], bytes
    int32_t pieces_pn, chans_pn, n_nets;
};

template <typename T>
__device__ __forceinline__ T* bf_at(T* p, int64_t d) { return (T*)((char*)p + d); }

// launch 1: w[r, :] *= gamma[r] / sqrtf(var[r] + eps)
__global__ __launch_bounds__(kBlock) void bf_stream_kernel(BfArgs a) {
    __shared__ float k_of[kFoldPiece];                 // k of row first_row + i
    BfPairDev P;
    const BatchPiece p = batch_piece(a.pieces_pn, a.piece_pair, a.pairs, P);
    const int64_t d = a.delta[p.net];
    gfloat* w = (gfloat*)bf_at(P.w, d) + p.start;
    const int t = threadIdx.x;
    const int nv = p.nv, n_rows = p.n_rows;
    const uint32_t row_len = p.row_len, rem0 = p.rem0;
    fvec4 x[kFoldInFlight];
    float xt;
    batch_piece_load<true>(p, w, x, xt);
    const int tail = (nv << 2) + t;
    const gfloat* gamma = (const gfloat*)bf_at(P.gamma, d) + p.first_row;
    const gfloat* var = (const gfloat*)bf_at(P.var, d) + p.first_row;
    for (int i = t; i < n_rows; i += kBlock) {
        const float sd = sqrtf(var[i] + P.eps);        // bn_fold_vec_kernel, dfq_misc.hip
        k_of[i] = gamma[i] / sd;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kFoldInFlight; ++j) {
        const int v = j * kBlock + t;
        if (v >= nv) continue;
        const uint32_t e = rem0 + 4u * (uint32_t)v;
        uint32_t row = e / row_len;
        uint32_t rem = e - row * row_len;
        fvec4 y;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            y[c] = x[j][c] * k_of[row];                // scale_rows_kernel, op 0
            if (++rem == row_len) { rem = 0; ++row; }
        }
        DFQ_NT_STORE(y, (gfvec4*)(w + 4 * v));
    }
    if (tail < p.count) w[tail] = xt * k_of[(rem0 + (uint32_t)tail) / row_len];
}

// launch 2: the per-channel part of bn_fold_vec_kernel; var becomes 1 here, what fill_kernel does behind the row scale
__global__ __launch_bounds__(kBlock) void bf_vec_kernel(BfArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)a.chans_pn * a.n_nets) return;
    const int net = (int)(t / a.chans_pn);
    const int j = (int)(t - (int64_t)net * a.chans_pn);
    const BfPairDev P = a.pairs[a.chan_pair[j]];
    const int o = j - P.chan_begin;
    const int64_t d = a.delta[net];
    gfloat* b = (gfloat*)bf_at(P.b, d);
    gfloat* gamma = (gfloat*)bf_at(P.gamma, d);
    gfloat* beta = (gfloat*)bf_at(P.beta, d);
    gfloat* mean = (gfloat*)bf_at(P.mean, d);
    gfloat* var = (gfloat*)bf_at(P.var, d);
    const float g = gamma[o], bt = beta[o], mu = mean[o], vr = var[o];
    const float sd = sqrtf(vr + P.eps);
    const float k = g / sd;
    const float gm = g * mu;
    const float shift = bt - gm / sd;
    const float bk = b[o] * k;
    b[o] = bk + shift;
    ((gfloat*)bf_at(P.fake_weight, d))[o] = fabsf(g);
    ((gfloat*)bf_at(P.fake_bias, d))[o] = bt;
    var[o] = 1.0f;
    gamma[o] = 1.0f;
    beta[o] = 0.0f;
    mean[o] = 0.0f;
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_fold_plan {
    DevSlab mem;
    BfArgs args{};
    int stream_blocks = 0, vec_blocks = 0;
    int64_t elements = 0;
};

extern "C" {

int32_t dfq_batch_fold_plan_launches(const dfq_batch_fold_plan* p) { return p ? (p->stream_blocks > 0) + (p->vec_blocks > 0) : 0; }

int64_t dfq_batch_fold_plan_elements(const dfq_batch_fold_plan* p) { return p ? p->elements : 0; }

void dfq_batch_fold_plan_destroy(dfq_batch_fold_plan* p) { batch_plan_destroy(p); }

int dfq_batch_fold_plan_create(const dfq_batch_fold_pair* pairs, int32_t n_pairs, const void* const* bases, int32_t n_nets,
                               dfq_batch_fold_plan** out_plan) {
    const char* me = "dfq_batch_fold_plan_create";
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (!pairs || n_pairs <= 0) return fail_arg("%s: the pair table is null or empty (n_pairs %d)", me, (int)n_pairs);
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    for (int n = 1; n < n_nets; ++n)                   // the 16-byte accesses of network 0 must be 16-byte accesses everywhere
        if (((uintptr_t)bases[n] - (uintptr_t)bases[0]) % 16 != 0) return fail_arg("%s: network %d is not 16-byte aligned to network 0", me, n);

    std::vector<BfPairDev> dev;
    std::vector<int32_t> piece_pair, chan_pair;
    std::vector<const void*> vectors;                  // every per-channel vector seen so far: none may appear twice
    int64_t chans = 0, elements = 0;
    for (int i = 0; i < n_pairs; ++i) {
        const dfq_batch_fold_pair& q = pairs[i];
        if (!q.w || !q.b || !q.gamma || !q.beta || !q.mean || !q.var || !q.fake_weight || !q.fake_bias)
            return fail_arg("%s: pair %d: null tensor", me, i);
        if (q.out_ch <= 0 || q.row_len <= 0) return fail_arg("%s: pair %d: empty shape [%d, %lld]", me, i, (int)q.out_ch, (long long)q.row_len);
        if (q.row_len > 0x7fffffff - kFoldPiece) return fail_arg("%s: pair %d: a row of %lld elements", me, i, (long long)q.row_len);
        if ((uintptr_t)q.w % 16 != 0) return fail_arg("%s: pair %d: the weight is not 16-byte aligned", me, i);
        for (int j = 0; j < i; ++j)
            if (pairs[j].w == q.w) return fail_arg("%s: pairs %d and %d share a weight", me, j, i);
        const void* mine[7] = {q.b, q.gamma, q.beta, q.mean, q.var, q.fake_weight, q.fake_bias};
        for (int u = 0; u < 7; ++u) {
            for (int v = 0; v < u; ++v)
                if (mine[v] == mine[u]) return fail_arg("%s: pair %d: two of its vectors are the same", me, i);
            if (std::find(vectors.begin(), vectors.end(), mine[u]) != vectors.end())
                return fail_arg("%s: pair %d shares a bias or a BatchNorm vector with an earlier pair", me, i);
        }
        vectors.insert(vectors.end(), mine, mine + 7);
        BfPairDev P{q.w, q.b, q.gamma, q.beta, q.mean, q.var, q.fake_weight, q.fake_bias,
                    (int64_t)q.out_ch * q.row_len, (int32_t)q.row_len, q.out_ch, q.eps, 0, (int32_t)chans};
        const int64_t begin = batch_add_pieces(piece_pair, i, P.n, 0x7fffffff / n_nets);
        chans += q.out_ch;
        elements += P.n;
        if (begin < 0 || chans > 0x7fffffff / n_nets) return fail_arg("%s: too much work for one launch", me);
        P.piece_begin = (int32_t)begin;
        chan_pair.insert(chan_pair.end(), (size_t)q.out_ch, (int32_t)i);
        dev.push_back(P);
    }

    const int64_t pieces = (int64_t)piece_pair.size();
    dfq_batch_fold_plan* p = new dfq_batch_fold_plan();
    BfArgs& a = p->args;
    a.pieces_pn = (int32_t)pieces;
    a.chans_pn = (int32_t)chans;
    a.n_nets = n_nets;
    p->stream_blocks = (int)(pieces * n_nets);
    p->vec_blocks = (int)((chans * n_nets + kBlock - 1) / kBlock);
    p->elements = elements;
    BatchUpload up{p->mem};
    a.pairs = up.put(dev);
    a.piece_pair = up.put(piece_pair);
    a.chan_pair = up.put(chan_pair);
    a.delta = up.put(batch_delta(bases, n_nets));
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch fold plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_fold_plan_run(dfq_batch_fold_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_fold_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    const BfArgs& a = p->args;
    hipLaunchKernelGGL(bf_stream_kernel, dim3(p->stream_blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(bf_vec_kernel, dim3(p->vec_blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
