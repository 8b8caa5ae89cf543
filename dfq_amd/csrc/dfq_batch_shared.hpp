// What the batch plans share (dfq_quant_batch.hip, dfq_absorb_batch.hip, dfq_act_batch.hip, dfq_fold_batch.hip,
// dfq_table_batch.hip, dfq_error_batch.hip).  Host side: a plan holds the tables of network 0 in a DevSlab
// `mem` and finds network n's tensors bases[n] - bases[0] bytes further on.  Device side: the flat pieces the streaming plans
// (fold, table, error) cut their tensors into.  Everything here has internal linkage (the library exports nothing for it).
#pragma once

#include "dfq_common.hpp"

namespace dfq {
namespace {

// the base addresses of a batch: DFQ_OK, or the argument error under the caller's name
inline int batch_check_bases(const char* me, const void* const* bases, int32_t n_nets) {
    if (!bases || n_nets <= 0) return fail_arg("%s: no networks (n_nets %d)", me, (int)n_nets);
    for (int n = 0; n < n_nets; ++n)
        if (!bases[n]) return fail_arg("%s: base address of network %d is null", me, n);
    return DFQ_OK;
}

// bases[n] - bases[0], bytes
inline std::vector<int64_t> batch_delta(const void* const* bases, int32_t n_nets) {
    std::vector<int64_t> delta(n_nets);
    for (int n = 0; n < n_nets; ++n) delta[n] = (int64_t)((uintptr_t)bases[n] - (uintptr_t)bases[0]);
    return delta;
}

// Host tables into a plan's DevSlab.  The first error is kept in `err` and nothing is tried after it; an empty table stays null.
struct BatchUpload {
    DevSlab& mem;
    hipError_t err = hipSuccess;
    void* raw(const void* h, size_t bytes) {               // h null: the allocation alone
        void* d = nullptr;
        if (err != hipSuccess || bytes == 0) return nullptr;
        if ((err = mem.alloc(&d, bytes)) == hipSuccess && h) err = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
        return d;
    }
    template <typename T>
    const T* put(const std::vector<T>& table) { return (const T*)raw(table.data(), sizeof(T) * table.size()); }
};

template <typename Plan>
void batch_plan_destroy(Plan* p) {
    if (!p) return;
    dev_quiesce();                                         // nothing in flight may still use the blocks released below
    p->mem.release();
    delete p;
}

// ---- flat pieces -------------------------------------------------------------------------------------------------------------
// A [rows, row_len] tensor is cut into pieces of kBatchPiece consecutive floats, one workgroup each: element e lies in row
// e / row_len, so rows of 9, of 27 and rows longer than a piece take the same path, and every lane moves 16 bytes per access
// whatever the row length.  Work is found from tables of ONE network: workgroup -> (network, piece of network 0) by a
// division, then the piece's tensor from a table of network 0's pieces (one load).
constexpr int kPieceInFlight = 4;                               // 16-byte loads a lane issues before it uses the first
constexpr int kBatchPiece = kBlock * 4 * kPieceInFlight;        // floats of one tensor a workgroup reads

// host: the pieces of tensor `tensor` (n elements) behind those already in the table; its first piece, or -1 -- nothing
// appended -- if one network would then have more than `most` pieces
inline int64_t batch_add_pieces(std::vector<int32_t>& piece_tensor, int32_t tensor, int64_t n, int64_t most) {
    const int64_t begin = (int64_t)piece_tensor.size(), k = (n + kBatchPiece - 1) / kBatchPiece;
    if (k > most - begin) return -1;
    piece_tensor.insert(piece_tensor.end(), (size_t)k, tensor);
    return begin;
}

struct BatchPiece {               // the piece of this workgroup
    int64_t start;                // its first element in the tensor
    int64_t first_row;
    uint32_t rem0, row_len;       // rem0: the place of the piece's first element in its row
    int net, lp, ti, count, n_rows, nv;      // lp: piece within one network; count floats, nv whole 16-byte vectors
};

// TensorDev: the plan's table entry, with n (elements), row_len and piece_begin
template <typename TensorDev>
__device__ __forceinline__ BatchPiece batch_piece(int pieces_pn, const int32_t* piece_tensor, const TensorDev* tensors, TensorDev& T) {
    BatchPiece p;
    p.net = (int)(blockIdx.x / (unsigned)pieces_pn);
    p.lp = (int)blockIdx.x - p.net * pieces_pn;
    p.ti = piece_tensor[p.lp];
    T = tensors[p.ti];
    p.start = (int64_t)(p.lp - T.piece_begin) * kBatchPiece;
    p.count = (int)(T.n - p.start < kBatchPiece ? T.n - p.start : kBatchPiece);
    p.first_row = p.start / T.row_len;
    p.rem0 = (uint32_t)(p.start - p.first_row * T.row_len);
    p.row_len = (uint32_t)T.row_len;
    p.n_rows = (int)((p.rem0 + (uint32_t)p.count - 1u) / p.row_len) + 1;
    p.nv = p.count >> 2;
    return p;
}

// Every load of the piece (`w`: its first element) back to back: a load under a per-lane condition is a block of its own that
// ends in a wait, so a lane past the piece's end reads the last vector again (the same line) under one workgroup-uniform
// condition instead.  A tensor's last piece may end in up to three single floats, one each for the first lanes (xt).
template <bool NT>
__device__ __forceinline__ void batch_piece_load(const BatchPiece& p, const gfloat* w, fvec4 (&x)[kPieceInFlight], float& xt) {
    const int t = threadIdx.x;
    if (p.nv > 0) {
#pragma unroll
        for (int j = 0; j < kPieceInFlight; ++j) {
            const int v = j * kBlock + t;
            const gfvec4* at = (const gfvec4*)(w + 4 * (v < p.nv ? v : p.nv - 1));
            x[j] = NT ? DFQ_NT_LOAD(at) : *at;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPieceInFlight; ++j) x[j] = fvec4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    const int tail = (p.nv << 2) + t;
    xt = tail < p.count ? w[tail] : 0.0f;
}

// Segmented scan over the wave of the run a lane's vector `v` STARTS in (`key`: that row; `head`: N values).  Rows are
// contiguous, so the lanes whose vectors start in one row are consecutive, and the first of them is the first lane whose
// vector starts at or behind the row's first element: six shuffles, no keys exchanged.  merge(head, other) folds the values
// of a lane further down into a lane's own; the LAST lane of a segment ends with the segment's result.
template <int N, typename Merge>
__device__ __forceinline__ void wave_head_scan(const BatchPiece& p, int v, uint32_t key, float (&head)[N], Merge merge) {
    const int lane = threadIdx.x % kWave;
    const int wave_e0 = (int)(p.rem0 + 4u * (uint32_t)(v - lane));
    const int ahead = (int)(key * p.row_len) - wave_e0;
    const int lane_start = ahead <= 0 ? 0 : (ahead + 3) >> 2;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        float other[N];
#pragma unroll
        for (int k = 0; k < N; ++k) other[k] = __shfl(head[k], lane >= d ? lane - d : lane);
        if (lane - d >= lane_start) merge(head, other);
    }
}

}  // namespace
}  // namespace dfq
