// MSE-optimal weight clipping of a whole batch of networks of one architecture (extension: the reference's clip_weight,
// dfq.py:167-170, with a searched bound per tensor or per output row in place of one constant for the network).  The
// definition -- shrink factors, candidate ends, the error of a candidate (of the CLAMPED weight), the choice, the clamp -- is the comment of
// dfq_batch_clip_plan_create in include/dfq_hip.h; nothing here restates the numerics differently.  The plan holds network 0's
// tensor table and one byte offset per network, like the other batch plans.
//
// A UNIT is an output row (per_row) or a whole tensor.  Units of at most kClipRegElems elements -- every row of a per-row
// plan up to that length, and per-tensor tensors that small -- take the lane classes of bq_rows (dfq_quant_batch.hip): L in
// {4, 8, 16, 32, 64} lanes per unit, 64 / L units per wave and kClipGroupRows such sets below L = 64.  A lane loads its share
// once (all loads in front of the first fold), and the share stays in registers for the min/max, for all K candidates and
// for the clamp: one launch, one read, at most one write (bc_row_kernel).
//   * qparams_double is a float64 division.  Lane g of a unit's L lanes forms the parameters of candidate base + g, so one
//     pass through the division's instructions serves L candidates (K <= 64: ONE pass for the 64-lane class); the candidate
//     at hand is then broadcast inside the unit's lanes: v_readlane for L = 64, a permute below.
//   * a candidate's sum: a lane adds its elements in slot order in float64 (e^2 formed in float64, exactly), then the xor
//     butterfly of wave_sum restricted to the unit's lanes (stages L / 2 ... 1; register moves and DPP, xor_lane_add).  Lanes
//     past the row's end hold +0.0.  The order depends on the row length alone.
// Longer rows of a per-row plan: one wave per row, looping (bc_long_row); the K float64 accumulators do not fit next to a
// row that is not in registers, so the candidates are taken kClipLongAtOnce at a time and the row is read again from the
// cache for each such group, and once more for the clamp.
// Longer per-tensor tensors: the flat 4096-float pieces of dfq_batch_shared.hpp, four launches, none with a wait inside:
//   1. bc_range_kernel: a piece's (min, max) into its tensor's pair of order-preserving words (cleared in front of it);
//   2. bc_search_kernel: a lane keeps its 16 elements across the K candidates (threads 0..K-1 form the parameters, once per
//      piece, into LDS); per candidate wave_sum, then the four waves in fixed order -- block_sum's arithmetic with one barrier
//      for all candidates -- into the plan's scratch [n_nets, pieces, K];
//   3. bc_fold_kernel: one wave per network and tensor, lane k adds the pieces of candidate k in rising order; lane 0 draws
//      k* and writes the outputs;
//   4. bc_clamp_kernel (only with `apply`): the same pieces once more, a 16-byte vector stored only where the clamp changed it.
// No floating-point atomic anywhere: two runs are bit-identical, and a network's numbers depend on nothing but its weights.
// Every value from memory meets a min / max only through dfq_range.hpp (NaN skipped; nothing but NaN: (NaN, NaN)).
#include <math.h>

#include <vector>

#include "dfq_batch_shared.hpp"
#include "dfq_range.hpp"

namespace dfq {

constexpr int kClipRegPerLane = 24;                    // register slots per lane of the 64-lane class (kRegPerLane of dfq_quant_batch.hip)
constexpr int64_t kClipRegElems = (int64_t)kWave * kClipRegPerLane;   // longest unit kept in registers
constexpr int kClipSmallPerLane = 4;                   // the classes L < 64 hold rows of at most 4 L elements,
constexpr int kClipGroupRows = 4;                      // kClipGroupRows sets of them per wave
constexpr int kClipMaxCand = 64;
constexpr int kClipLongAtOnce = 4;                     // candidates a looping wave carries through one pass over its row

typedef DFQ_GLOBAL_AS int32_t gint32c;
typedef DFQ_GLOBAL_AS double gdouble;

struct BcRowDev {                 // a tensor searched unit by unit in registers or by a looping wave (network 0)
    float* data;
    int64_t out_off;              // its first unit in a network's part of the blocks
    int32_t rows, len;
    int32_t cls;                  // 0: one wave per row, looping; c > 0: L = 2 << c lanes per row
    int32_t wave_begin;           // first wave (within one network)
};

struct BcFlatDev {                // a per-tensor tensor of more than kClipRegElems elements (network 0)
    float* data;
    int64_t n;
    int64_t out_off;
    int32_t row_len;              // (batch_piece wants one: the whole tensor)
    int32_t piece_begin, n_pieces;
    int32_t index;                // among the flat tensors
};

struct BcArgs {
    const BcRowDev* rows;
    const int32_t* wave_tensor;   // row tensor of every wave of network 0
    const BcFlatDev* flats;
    const int32_t* piece_tensor;  // flat tensor of every piece of network 0
    const int64_t* delta;         // bases[n] - bases[0], bytes
    const double* alpha;          // [K] shrink factors
    uint32_t* words;              // [n_nets, n_flats, 2]: ~enc_ord(min), enc_ord(max)
    double* partial;              // [n_nets, pieces_pn, K]
    float* ranges;                // [n_nets, stride, 2]
    int32_t* chosen;              // [n_nets, stride]
    double* errors;               // [n_nets, stride, K] or null
    int64_t stride;
    int32_t row_wpn, row_waves;
    int32_t pieces_pn, n_flats, n_nets;
    int32_t num_bits, symmetric, K, apply;
};

// the ends of the candidate with shrink factor alpha (include/dfq_hip.h); (NaN, NaN) for a unit of nothing but NaN
__device__ __forceinline__ void bc_candidate(float mn, float mx, double alpha, float& l, float& h) {
    const double a = (double)mn, b = (double)mx;
    double z = a > 0.0 ? a : 0.0;                      // max(0, mn)
    z = z < b ? z : b;                                 // min(., mx)
    l = (float)(z + alpha * (a - z));
    h = (float)(z + alpha * (b - z));
}

__device__ __forceinline__ float bc_clamp(float w, float l, float h) { return w < l ? l : (w > h ? h : w); }

// e^2 of one weight under a candidate: what quant_plan stores for the weight clamped to (l, h), minus the weight as it is
__device__ __forceinline__ double bc_sq_error(float w, const QParams& q, float l, float h) {
    float code;
    const double d = (double)(fake_quant_one(bc_clamp(w, l, h), q, &code) - w);
    return d * d;
}

// lane kk of the L lanes of this lane's unit
template <int L>
__device__ __forceinline__ float bc_bcast(float v, int kk) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (L == kWave) return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), kk));
#endif
    const int lane = threadIdx.x % kWave;
    return __shfl(v, (lane & ~(L - 1)) | kk);
}

// wave_sum's butterfly inside the L lanes of a unit
template <int L>
__device__ __forceinline__ double bc_group_sum(double v) {
    if constexpr (L > 32) xor_lane_add<32>(v);
    if constexpr (L > 16) xor_lane_add<16>(v);
    if constexpr (L > 8) xor_lane_add<8>(v);
    if constexpr (L > 4) xor_lane_add<4>(v);
    if constexpr (L > 2) xor_lane_add<2>(v);
    if constexpr (L > 1) xor_lane_add<1>(v);
    return v;
}

struct BcOut {                    // one network's part of the blocks
    gfloat* ranges;
    gint32c* chosen;
    gdouble* errors;              // null: not kept
};

// R sets of 64 / L rows of one tensor from first_row on (row first_row + j * 64 / L + lane / L), L lanes each, S register
// slots per lane and row (len <= S * L).  A lane holds element g + k L of its row in slot k for the len / L FULL slots, which
// need no condition per lane, and the one element behind them (if the row has one for it) apart: 24 lane conditions that
// stay alive through the candidate loop were 48 scalar registers, and spills.
template <int L, int S, int R>
__device__ __forceinline__ void bc_rows(const BcArgs& a, const BcRowDev& T, float* x, const BcOut& o, int first_row) {
    constexpr int G = kWave / L;
    const int lane = threadIdx.x % kWave;
    const int g = lane % L;
    const int r0 = first_row + lane / L;
    const int len = T.len, K = a.K;
    const int nfull = len / L;                         // <= S
    const int it = g + nfull * L;                      // this lane's element behind the full slots
    const bool any_tail = nfull * L < len;             // (wave-uniform)
    gfloat* xr0 = (gfloat*)x;
    float v[R][S], vt[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {                      // every load first (bq_rows)
#pragma unroll
        for (int k = 0; k < S; ++k) v[j][k] = 0.0f;
        vt[j] = 0.0f;
        if (first_row + j * G >= T.rows) break;        // (wave-uniform)
        const int r = r0 + j * G;
        const bool live = r < T.rows;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            if (k >= nfull) break;                     // (wave-uniform)
            if (live) v[j][k] = xr0[(int64_t)r * len + g + k * L];
        }
        if (live && it < len) vt[j] = xr0[(int64_t)r * len + it];
    }
    QParams q = qparams_double(0.0, 1.0, a.num_bits, a.symmetric);       // qmin and qmax; the rest comes per candidate
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (first_row + j * G >= T.rows) break;
        const int r = r0 + j * G;
        const bool live = r < T.rows;
        const bool tail = live && it < len;
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < S; ++k) {                  // (a row past the tensor's end folds its zeros: nobody reads its range)
            if (k < nfull) range_fold(v[j][k], mn, mx);    // (wave-uniform)
        }
        if (tail) range_fold(vt[j], mn, mx);
        if constexpr (L > 1) xor_lane_minmax<1>(mn, mx);
        if constexpr (L > 2) xor_lane_minmax<2>(mn, mx);
        if constexpr (L > 4) xor_lane_minmax<4>(mn, mx);
        if constexpr (L > 8) xor_lane_minmax<8>(mn, mx);
        if constexpr (L > 16) xor_lane_minmax<16>(mn, mx);
        if constexpr (L > 32) xor_lane_minmax<32>(mn, mx);
        if (!(mn <= mx)) mn = mx = NAN;                // nothing but NaN
        const int64_t u = T.out_off + r;
        double best = 0.0;
        int kstar = 0;
        for (int base = 0; base < K; base += L) {      // (wave-uniform)
            // this lane's candidate of the pass: one run through the division for L candidates
            const int kc = base + g;
            float cl, ch;
            bc_candidate(mn, mx, a.alpha[kc < K ? kc : 0], cl, ch);
            const QParams cq = qparams_double((double)cl, (double)ch, a.num_bits, a.symmetric);
            const int n = K - base < L ? K - base : L;
            for (int kk = 0; kk < n; ++kk) {
                q.scale = bc_bcast<L>(cq.scale, kk);
                q.min_value = bc_bcast<L>(cq.min_value, kk);
                const float kl = bc_bcast<L>(cl, kk), kh = bc_bcast<L>(ch, kk);
                q.neg_min = -q.min_value;              // (in both recipes of qparams_double)
                double s = 0.0;                        // a lane without the element adds +0.0: s + 0.0 == s
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    if (k >= nfull) break;
                    const double e2 = bc_sq_error(v[j][k], q, kl, kh);
                    s += live ? e2 : 0.0;
                }
                if (any_tail) {
                    const double e2 = bc_sq_error(vt[j], q, kl, kh);
                    s += tail ? e2 : 0.0;
                }
                s = bc_group_sum<L>(s);
                if (o.errors && live && g == kk) o.errors[u * K + base + kk] = s;
                if (base + kk == 0) best = s;
                else if (s < best) { best = s; kstar = base + kk; }
            }
        }
        if (!live) continue;
        float l, h;
        bc_candidate(mn, mx, a.alpha[kstar], l, h);
        if (g == 0) {
            o.ranges[2 * u + 0] = l;
            o.ranges[2 * u + 1] = h;
            o.chosen[u] = kstar;
        }
        if (!a.apply || kstar == 0) continue;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            if (k >= nfull) break;
            const float w = v[j][k];
            if (w < l || w > h) xr0[(int64_t)r * len + g + k * L] = bc_clamp(w, l, h);
        }
        if (tail && (vt[j] < l || vt[j] > h)) xr0[(int64_t)r * len + it] = bc_clamp(vt[j], l, h);
    }
}

// one row longer than kClipRegElems: one wave; the row is read for the range, once per kClipLongAtOnce candidates and for the clamp
__device__ __forceinline__ void bc_long_row(const BcArgs& a, const BcRowDev& T, float* x, const BcOut& o, int r) {
    const int lane = threadIdx.x % kWave;
    const int len = T.len, K = a.K;
    gfloat* xr = (gfloat*)x + (int64_t)r * len;
    float mn, mx;
    wave_row_range(xr, len, mn, mx);
    if (!(mn <= mx)) mn = mx = NAN;
    const int64_t u = T.out_off + r;
    float cl, ch;                                      // lane k forms candidate k (K <= 64)
    bc_candidate(mn, mx, a.alpha[lane < K ? lane : 0], cl, ch);
    const QParams cq = qparams_double((double)cl, (double)ch, a.num_bits, a.symmetric);
    double best = 0.0;
    int kstar = 0;
    for (int base = 0; base < K; base += kClipLongAtOnce) {
        const int n = K - base < kClipLongAtOnce ? K - base : kClipLongAtOnce;
        QParams q[kClipLongAtOnce];
        float kl[kClipLongAtOnce], kh[kClipLongAtOnce];
        double s[kClipLongAtOnce];
#pragma unroll
        for (int c = 0; c < kClipLongAtOnce; ++c) {
            const int kk = c < n ? base + c : base;
            q[c] = cq;
            q[c].scale = bc_bcast<kWave>(cq.scale, kk);
            q[c].min_value = bc_bcast<kWave>(cq.min_value, kk);
            kl[c] = bc_bcast<kWave>(cl, kk);
            kh[c] = bc_bcast<kWave>(ch, kk);
            q[c].neg_min = -q[c].min_value;
            s[c] = 0.0;
        }
        for (int i = lane; i < len; i += kWave) {
            const float w = xr[i];
#pragma unroll
            for (int c = 0; c < kClipLongAtOnce; ++c)
                if (c < n) s[c] += bc_sq_error(w, q[c], kl[c], kh[c]);   // (wave-uniform)
        }
#pragma unroll
        for (int c = 0; c < kClipLongAtOnce; ++c) {
            if (c >= n) continue;                      // (wave-uniform)
            const double t = wave_sum(s[c]);
            if (o.errors && lane == 0) o.errors[u * K + base + c] = t;
            if (base + c == 0) best = t;
            else if (t < best) { best = t; kstar = base + c; }
        }
    }
    float l, h;
    bc_candidate(mn, mx, a.alpha[kstar], l, h);
    if (lane == 0) {
        o.ranges[2 * u + 0] = l;
        o.ranges[2 * u + 1] = h;
        o.chosen[u] = kstar;
    }
    if (!a.apply || kstar == 0) return;
    for (int i = lane; i < len; i += kWave) {
        const float w = xr[i];
        if (w < l || w > h) xr[i] = bc_clamp(w, l, h);
    }
}

__device__ __forceinline__ BcOut bc_out(const BcArgs& a, int net) {
    BcOut o;
    o.ranges = (gfloat*)a.ranges + 2 * (int64_t)net * a.stride;
    o.chosen = (gint32c*)a.chosen + (int64_t)net * a.stride;
    o.errors = a.errors ? (gdouble*)a.errors + (int64_t)net * a.stride * a.K : nullptr;
    return o;
}

// the units held in registers and the long rows: one launch
__global__ __launch_bounds__(kBlock) void bc_row_kernel(BcArgs a) {
    const int w = (int)blockIdx.x * (kBlock / kWave) + (int)threadIdx.x / kWave;
    if (w >= a.row_waves) return;                      // (wave-uniform)
    const int net = w / a.row_wpn;
    const int lw = w - net * a.row_wpn;
    const BcRowDev T = a.rows[a.wave_tensor[lw]];
    float* x = (float*)((char*)T.data + a.delta[net]);
    const BcOut o = bc_out(a, net);
    const int wi = lw - T.wave_begin;
    switch (T.cls) {
        case 1: bc_rows<4, kClipSmallPerLane, kClipGroupRows>(a, T, x, o, wi * 16 * kClipGroupRows); break;
        case 2: bc_rows<8, kClipSmallPerLane, kClipGroupRows>(a, T, x, o, wi * 8 * kClipGroupRows); break;
        case 3: bc_rows<16, kClipSmallPerLane, kClipGroupRows>(a, T, x, o, wi * 4 * kClipGroupRows); break;
        case 4: bc_rows<32, kClipSmallPerLane, kClipGroupRows>(a, T, x, o, wi * 2 * kClipGroupRows); break;
        case 5: bc_rows<64, kClipRegPerLane, 1>(a, T, x, o, wi); break;
        default: bc_long_row(a, T, x, o, wi); break;
    }
}

// ---- per-tensor tensors of more than kClipRegElems elements: flat pieces ---------------------------------------------------
struct BcPiece : BatchPiece {
    BcFlatDev T;
    gfloat* w;
    uint32_t* words;              // the tensor's pair
};

__device__ __forceinline__ BcPiece bc_piece(const BcArgs& a) {
    BcPiece p;
    (BatchPiece&)p = batch_piece(a.pieces_pn, a.piece_tensor, a.flats, p.T);
    p.w = (gfloat*)(float*)((char*)p.T.data + a.delta[p.net]) + p.start;
    p.words = a.words + 2 * ((int64_t)p.net * a.n_flats + p.T.index);
    return p;
}

// launch 1: the piece's (min, max) into its tensor's words
__global__ __launch_bounds__(kBlock) void bc_range_kernel(BcArgs a) {
    const BcPiece p = bc_piece(a);
    const int t = threadIdx.x;
    fvec4 x[kPieceInFlight];
    float xt;
    batch_piece_load<false>(p, p.w, x, xt);
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kPieceInFlight; ++j)
        if (j * kBlock + t < p.nv) range_fold4(x[j], mn, mx);
    if ((p.nv << 2) + t < p.count) range_fold(xt, mn, mx);
    block_range(mn, mx);
    if (t == 0) range_publish(mn, mx, p.words + 0, p.words + 1);      // (nothing for a piece of NaNs)
}

// launch 2: the piece's K sums
__global__ __launch_bounds__(kBlock) void bc_search_kernel(BcArgs a) {
    __shared__ float q_scale[kClipMaxCand];
    __shared__ float q_minv[kClipMaxCand];
    __shared__ float q_lo[kClipMaxCand];
    __shared__ float q_hi[kClipMaxCand];
    __shared__ double sh[kClipMaxCand][kBlock / kWave];
    const BcPiece p = bc_piece(a);
    const int t = threadIdx.x;
    const int K = a.K;
    fvec4 x[kPieceInFlight];
    float xt;
    batch_piece_load<false>(p, p.w, x, xt);
    const float mn = slot_min(p.words[0]), mx = slot_max(p.words[1]);      // cleared words: (NaN, NaN)
    if (t < K) {
        float cl, ch;
        bc_candidate(mn, mx, a.alpha[t], cl, ch);
        const QParams cq = qparams_double((double)cl, (double)ch, a.num_bits, a.symmetric);
        q_scale[t] = cq.scale;
        q_minv[t] = cq.min_value;
        q_lo[t] = cl;
        q_hi[t] = ch;
    }
    __syncthreads();
    QParams q = qparams_double(0.0, 1.0, a.num_bits, a.symmetric);
    const bool has_tail = (p.nv << 2) + t < p.count;
    for (int k = 0; k < K; ++k) {
        q.scale = q_scale[k];
        q.min_value = q_minv[k];
        q.neg_min = -q.min_value;
        const float kl = q_lo[k], kh = q_hi[k];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < kPieceInFlight; ++j) {
            if (j * kBlock + t < p.nv) {
#pragma unroll
                for (int c = 0; c < 4; ++c) s += bc_sq_error(x[j][c], q, kl, kh);
            }
        }
        if (has_tail) s += bc_sq_error(xt, q, kl, kh);
        s = wave_sum(s);
        if (t % kWave == 0) sh[k][t / kWave] = s;
    }
    __syncthreads();
    if (t < K) {                                       // block_sum's order: the four waves one after another
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) tot += sh[t][w];
        ((gdouble*)a.partial)[((int64_t)p.net * a.pieces_pn + p.lp) * K + t] = tot;
    }
}

// launch 3: one wave per network and tensor; lane k adds the pieces of candidate k in rising order
__global__ __launch_bounds__(kWave) void bc_fold_kernel(BcArgs a) {
    __shared__ double err[kClipMaxCand];
    const int net = (int)blockIdx.x / a.n_flats;
    const BcFlatDev T = a.flats[(int)blockIdx.x - net * a.n_flats];
    const int t = threadIdx.x, K = a.K;
    const BcOut o = bc_out(a, net);
    if (t < K) {
        const gdouble* part = (const gdouble*)a.partial + ((int64_t)net * a.pieces_pn + T.piece_begin) * K + t;
        double s = 0.0;
        for (int q = 0; q < T.n_pieces; ++q) s += part[(int64_t)q * K];
        err[t] = s;
        if (o.errors) o.errors[T.out_off * K + t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    double best = err[0];
    int kstar = 0;
    for (int k = 1; k < K; ++k)
        if (err[k] < best) { best = err[k]; kstar = k; }
    const uint32_t* words = a.words + 2 * ((int64_t)net * a.n_flats + T.index);
    float l, h;
    bc_candidate(slot_min(words[0]), slot_max(words[1]), a.alpha[kstar], l, h);
    o.ranges[2 * T.out_off + 0] = l;
    o.ranges[2 * T.out_off + 1] = h;
    o.chosen[T.out_off] = kstar;
}

// launch 4 (apply): the pieces clamped to their tensor's choice
__global__ __launch_bounds__(kBlock) void bc_clamp_kernel(BcArgs a) {
    const BcPiece p = bc_piece(a);
    const BcOut o = bc_out(a, p.net);
    if (o.chosen[p.T.out_off] == 0) return;            // (workgroup-uniform) candidate 0 is the tensor's own range
    const float l = o.ranges[2 * p.T.out_off + 0], h = o.ranges[2 * p.T.out_off + 1];
    const int t = threadIdx.x;
    fvec4 x[kPieceInFlight];
    float xt;
    batch_piece_load<false>(p, p.w, x, xt);
#pragma unroll
    for (int j = 0; j < kPieceInFlight; ++j) {
        const int v = j * kBlock + t;
        if (v >= p.nv) continue;
        fvec4 y;
        bool changed = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float w = x[j][c];
            changed = changed || w < l || w > h;
            y[c] = bc_clamp(w, l, h);
        }
        if (changed) *(gfvec4*)(p.w + 4 * v) = y;
    }
    const int tail = (p.nv << 2) + t;
    if (tail < p.count && (xt < l || xt > h)) p.w[tail] = bc_clamp(xt, l, h);
}

// lane class of a unit of `len` elements: the fewest lanes that hold it in kClipSmallPerLane slots, 64 up to kClipRegElems, else 0
inline int bc_class(int64_t len) {
    for (int c = 1; c <= 4; ++c)
        if (len <= (int64_t)(2 << c) * kClipSmallPerLane) return c;
    return len <= kClipRegElems ? 5 : 0;
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_clip_plan {
    DevSlab mem;
    BcArgs args{};
    size_t word_bytes = 0;
    int row_blocks = 0, piece_blocks = 0, fold_blocks = 0;
    int launches = 0;
};

extern "C" {

int32_t dfq_batch_clip_plan_launches(const dfq_batch_clip_plan* p) { return p ? p->launches : 0; }

void dfq_batch_clip_plan_destroy(dfq_batch_clip_plan* p) { batch_plan_destroy(p); }

int dfq_batch_clip_plan_create(const dfq_batch_clip_tensor* tensors, int32_t n_tensors, const dfq_batch_clip_config* config,
                               const void* const* bases, int32_t n_nets, float* ranges, int32_t* chosen, double* errors, int64_t stride,
                               dfq_batch_clip_plan** out_plan) {
    const char* me = "dfq_batch_clip_plan_create";
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (!tensors || n_tensors <= 0) return fail_arg("%s: the tensor table is null or empty (n_tensors %d)", me, (int)n_tensors);
    if (!config) return fail_arg("%s: no configuration", me);
    const dfq_batch_clip_config cfg = *config;
    if (cfg.num_bits < 2 || cfg.num_bits > 16) return fail_arg("%s: num_bits %d outside [2, 16]", me, (int)cfg.num_bits);
    if (cfg.candidates < 1 || cfg.candidates > kClipMaxCand)
        return fail_arg("%s: %d candidates (1..%d)", me, (int)cfg.candidates, kClipMaxCand);
    if (!(cfg.alpha_min > 0.0 && cfg.alpha_min <= 1.0)) return fail_arg("%s: alpha_min %g is not in (0, 1]", me, cfg.alpha_min);
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    for (int n = 1; n < n_nets; ++n)                   // the 16-byte accesses of network 0 must be 16-byte accesses everywhere
        if (((uintptr_t)bases[n] - (uintptr_t)bases[0]) % 16 != 0) return fail_arg("%s: network %d is not 16-byte aligned to network 0", me, n);
    if (!ranges || !chosen) return fail_arg("%s: the block of the ranges or of the choices is null", me);
    if (stride <= 0) return fail_arg("%s: stride %lld", me, (long long)stride);
    const int K = cfg.candidates;
    if (stride > INT64_MAX / 8 / K / n_nets) return fail_arg("%s: blocks of %d x %lld units", me, (int)n_nets, (long long)stride);

    std::vector<BcRowDev> rows;
    std::vector<BcFlatDev> flats;
    std::vector<int32_t> wave_tensor, piece_tensor;
    int64_t waves = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_clip_tensor& t = tensors[i];
        if (!t.data) return fail_arg("%s: tensor %d: null weight", me, i);
        if (t.rows <= 0 || t.row_len <= 0) return fail_arg("%s: tensor %d: empty shape [%lld, %lld]", me, i, (long long)t.rows, (long long)t.row_len);
        if (t.rows > 0x7fffffff - kWave || t.row_len > 0x7fffffff - 2 * kBatchPiece || t.rows > (0x7fffffff - 2 * kBatchPiece) / t.row_len)
            return fail_arg("%s: tensor %d: a shape of [%lld, %lld]", me, i, (long long)t.rows, (long long)t.row_len);
        if ((uintptr_t)t.data % 16 != 0) return fail_arg("%s: tensor %d: the weight is not 16-byte aligned", me, i);
        const int64_t numel = t.rows * t.row_len, units = cfg.per_row ? t.rows : 1;
        if (t.out_offset < 0 || t.out_offset > stride - units)
            return fail_arg("%s: tensor %d: %lld units at %lld lie outside the stride %lld", me, i, (long long)units, (long long)t.out_offset,
                            (long long)stride);
        if (!cfg.per_row && numel > kClipRegElems) {
            BcFlatDev f{t.data, numel, t.out_offset, (int32_t)numel, 0, 0, (int32_t)flats.size()};
            const int64_t begin = batch_add_pieces(piece_tensor, (int32_t)flats.size(), numel, 0x7fffffff / n_nets / K);
            if (begin < 0) return fail_arg("%s: too much work for one launch", me);
            f.piece_begin = (int32_t)begin;
            f.n_pieces = (int32_t)((int64_t)piece_tensor.size() - begin);
            flats.push_back(f);
        } else {
            BcRowDev r;
            r.data = t.data;
            r.out_off = t.out_offset;
            r.rows = (int32_t)units;
            r.len = (int32_t)(cfg.per_row ? t.row_len : numel);
            r.cls = bc_class(r.len);
            r.wave_begin = (int32_t)waves;
            const int64_t per_wave = r.cls == 5 || r.cls == 0 ? 1 : kWave / (2 << r.cls) * kClipGroupRows;
            const int64_t w = (r.rows + per_wave - 1) / per_wave;
            if ((waves + w) * n_nets > 0x7fffffff - kBlock) return fail_arg("%s: too much work for one launch", me);
            wave_tensor.insert(wave_tensor.end(), (size_t)w, (int32_t)rows.size());
            rows.push_back(r);
            waves += w;
        }
    }
    const int64_t pieces = (int64_t)piece_tensor.size();
    if ((int64_t)flats.size() * n_nets > 0x7fffffff) return fail_arg("%s: too much work for one launch", me);
    std::vector<double> alpha(K);
    for (int k = 0; k < K; ++k) alpha[k] = K == 1 ? 1.0 : 1.0 - (double)k * (1.0 - cfg.alpha_min) / (double)(K - 1);

    dfq_batch_clip_plan* p = new dfq_batch_clip_plan();
    BcArgs& a = p->args;
    a.ranges = ranges;
    a.chosen = chosen;
    a.errors = errors;
    a.stride = stride;
    a.row_wpn = (int32_t)waves;
    a.row_waves = (int32_t)(waves * n_nets);
    a.pieces_pn = (int32_t)pieces;
    a.n_flats = (int32_t)flats.size();
    a.n_nets = n_nets;
    a.num_bits = cfg.num_bits;
    a.symmetric = cfg.symmetric ? 1 : 0;
    a.K = K;
    a.apply = cfg.apply ? 1 : 0;
    p->row_blocks = (int)((waves * n_nets + kBlock / kWave - 1) / (kBlock / kWave));
    p->piece_blocks = (int)(pieces * n_nets);
    p->fold_blocks = (int)((int64_t)flats.size() * n_nets);
    p->launches = (p->row_blocks ? 1 : 0) + (p->piece_blocks ? 3 + a.apply : 0);
    BatchUpload up{p->mem};
    a.rows = up.put(rows);
    a.wave_tensor = up.put(wave_tensor);
    a.flats = up.put(flats);
    a.piece_tensor = up.put(piece_tensor);
    a.delta = up.put(batch_delta(bases, n_nets));
    a.alpha = up.put(alpha);
    p->word_bytes = sizeof(uint32_t) * 2 * flats.size() * (size_t)n_nets;
    a.words = (uint32_t*)up.raw(nullptr, p->word_bytes);
    a.partial = (double*)up.raw(nullptr, sizeof(double) * (size_t)pieces * (size_t)n_nets * (size_t)K);
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch clip plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_clip_plan_run(dfq_batch_clip_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_clip_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    const BcArgs& a = p->args;
    if (p->piece_blocks > 0) {
        DFQ_HIP_TRY(hipMemsetAsync(a.words, 0, p->word_bytes, st));
        hipLaunchKernelGGL(bc_range_kernel, dim3(p->piece_blocks), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
        hipLaunchKernelGGL(bc_search_kernel, dim3(p->piece_blocks), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
        hipLaunchKernelGGL(bc_fold_kernel, dim3(p->fold_blocks), dim3(kWave), 0, st, a);
        DFQ_CHECK_LAUNCH();
        if (a.apply) {
            hipLaunchKernelGGL(bc_clamp_kernel, dim3(p->piece_blocks), dim3(kBlock), 0, st, a);
            DFQ_CHECK_LAUNCH();
        }
    }
    if (p->row_blocks > 0) {
        hipLaunchKernelGGL(bc_row_kernel, dim3(p->row_blocks), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
    }
    return DFQ_OK;
}

}  // extern "C"
