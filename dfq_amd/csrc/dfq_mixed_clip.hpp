// Clip-aware mixed precision: the device side of dfq_batch_mixed_plan_create_clipped (include/dfq_hip.h holds the definition).
// Included by dfq_mixed_batch.hip alone, behind its own kernels, which it leaves as they are.  The work is cut as the clip plan
// cuts it (dfq_clip_batch.hip), because every unit error must be bit for bit the clip plan's: the same lane classes, the same
// register bound, the same 4096-float pieces and the same fold order -- restated here, not shared.  Order of the search: the
// WIDTHS OUTSIDE, the candidates inside.  A unit's registers are loaded once and its (min, max) found once; then, per width, the
// clip kernel's own candidate loop runs over them (its register shape: no array of B best values next to the 24 slots), and the
// width's k*, its ends and its error leave the lane before the next width starts.  Launches of a clipped plan:
//   ALLOCATE  bx_range_kernel, bx_search_kernel, bx_fold_kernel (only with flat tensors); bx_row_kernel (units in registers and
//             looping rows); bm_alloc_kernel, unchanged, on the plan's scratch [n_nets, units, B] -- a unit is a part, so a
//             per-row tensor's E is the sum of its rows' U in rising row order; bx_finish_kernel: the allocation as an INDEX into
//             the plan's own state, and `ranges` = (l, h) of the chosen width for every unit.
//   CLAMP     bx_apply_kernel<false> (+ bx_apply_flat_kernel<false>): only what the clamp changes is stored, nothing where k* = 0.
//   QUANTISE  bx_apply_kernel<true> (+ bx_apply_flat_kernel<true>): clamp, qparams_double(l, h, b_j), fake_quant_one.
// No floating-point atomic, no workgroup waits for another, nothing synchronises with the host.
#pragma once

namespace dfq {

constexpr int kMxMaxCand = 64;
constexpr int kMxMaxPairs = 512;                       // B * K one plan may ask for
constexpr int kMxLongAtOnce = 4;                       // candidates a looping wave carries through one pass over its row

struct BxRowDev {                 // a tensor searched unit by unit in registers or by a looping wave (network 0)
    float* data;
    int64_t unit_off;             // its first unit in a network's part of the clip blocks
    int64_t code_off, range_off;  // into one network's block, -1 = none
    int32_t rows, len;
    int32_t cls;                  // 0: one wave per row, looping; c > 0: L = 2 << c lanes per row
    int32_t wave_begin;           // first wave (within one network)
    int32_t tensor, part_begin;   // its place in the caller's table; its first unit among the parts of one network
};

struct BxFlatDev {                // a per-tensor tensor of more than kMixRegElems elements (network 0)
    float* data;
    int64_t n;
    int64_t unit_off, code_off, range_off;
    int32_t row_len;              // (batch_piece wants one: the whole tensor)
    int32_t piece_begin, n_pieces;
    int32_t index;                // among the flat tensors
    int32_t tensor, part;
};

struct BxTensorDev {              // a tensor as bx_finish_kernel sees it, in the caller's order
    int64_t unit_off, range_off;
    int32_t part_begin, pad;
};

struct BxArgs {
    const BxRowDev* rows;
    const int32_t* wave_tensor;   // row tensor of every wave of network 0
    const BxFlatDev* flats;
    const int32_t* piece_tensor;  // flat tensor of every piece of network 0
    const BxTensorDev* tensors;
    const int32_t* part_tensor;   // tensor of every part (unit) of network 0
    const int32_t* width_tab;     // [B]
    const int64_t* delta;         // bases[n] - bases[0], bytes
    const double* alpha;          // [K] shrink factors
    uint32_t* words;              // [n_nets, n_flats, 2]: ~enc_ord(min), enc_ord(max)
    double* scratch;              // [n_nets, pieces_pn, B * K]
    double* partial;              // [n_nets, parts_pn, B]: U at k*, what bm_alloc_kernel folds
    float* clip_ranges;           // [n_nets, unit_stride, B, 2]
    int32_t* clip_chosen;         // [n_nets, unit_stride, B]
    double* unit_errors;          // [n_nets, unit_stride, B] or null
    const int32_t* bits;          // [n_nets, n_tensors]: read by bx_finish_kernel only, straight behind the allocation
    int32_t* state;               // [n_nets, n_tensors]: the index j_t, the plan's own
    unsigned char* codes;
    float* ranges;
    int64_t code_stride, range_stride, unit_stride;
    int32_t n_widths, symmetric, code_bytes, n_tensors, K;
    int32_t row_wpn, row_waves, pieces_pn, n_flats, parts_pn, n_nets;
};

// the ends of the candidate with shrink factor alpha (include/dfq_hip.h); (NaN, NaN) for a unit of nothing but NaN
__device__ __forceinline__ void bx_candidate(float mn, float mx, double alpha, float& l, float& h) {
    const double a = (double)mn, b = (double)mx;
    double z = a > 0.0 ? a : 0.0;                      // max(0, mn)
    z = z < b ? z : b;                                 // min(., mx)
    l = (float)(z + alpha * (a - z));
    h = (float)(z + alpha * (b - z));
}

__device__ __forceinline__ float bx_clamp(float w, float l, float h) { return w < l ? l : (w > h ? h : w); }

// e^2 of one weight under a candidate: what the quantiser stores for the weight clamped to (l, h), minus the weight as it is
__device__ __forceinline__ double bx_sq_error(float w, const QParams& q, float l, float h) {
    float code;
    const double d = (double)(fake_quant_one(bx_clamp(w, l, h), q, &code) - w);
    return d * d;
}

// lane kk of the L lanes of this lane's unit
template <int L>
__device__ __forceinline__ float bx_bcast(float v, int kk) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (L == kWave) return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), kk));
#endif
    const int lane = threadIdx.x % kWave;
    return __shfl(v, (lane & ~(L - 1)) | kk);
}

// wave_sum's butterfly inside the L lanes of a unit
template <int L>
__device__ __forceinline__ double bx_group_sum(double v) {
    if constexpr (L > 32) xor_lane_add<32>(v);
    if constexpr (L > 16) xor_lane_add<16>(v);
    if constexpr (L > 8) xor_lane_add<8>(v);
    if constexpr (L > 4) xor_lane_add<4>(v);
    if constexpr (L > 2) xor_lane_add<2>(v);
    if constexpr (L > 1) xor_lane_add<1>(v);
    return v;
}

// what the search leaves for unit u (within its network) at width index b
__device__ __forceinline__ void bx_unit_out(const BxArgs& a, int net, int64_t u, int part, int b, float l, float h, int kstar, double err) {
    const int B = a.n_widths;
    const int64_t at = ((int64_t)net * a.unit_stride + u) * B + b;
    ((gfloat*)a.clip_ranges)[2 * at + 0] = l;
    ((gfloat*)a.clip_ranges)[2 * at + 1] = h;
    ((gint32m*)a.clip_chosen)[at] = kstar;
    if (a.unit_errors) ((gdouble*)a.unit_errors)[at] = err;
    ((gdouble*)a.partial)[((int64_t)net * a.parts_pn + part) * B + b] = err;
}

// bc_rows (dfq_clip_batch.hip) with the widths around its candidate loop and without its clamp: R sets of 64 / L rows of one
// tensor from first_row on, L lanes each, S register slots per lane and row; the len / L full slots need no condition per lane,
// the one element behind them is kept apart.
template <int L, int S, int R>
__device__ __forceinline__ void bx_rows(const BxArgs& a, const BxRowDev& T, float* x, int net, int first_row) {
    constexpr int G = kWave / L;
    const int lane = threadIdx.x % kWave;
    const int g = lane % L;
    const int r0 = first_row + lane / L;
    const int len = T.len, K = a.K, B = a.n_widths;
    const int nfull = len / L;                         // <= S
    const int it = g + nfull * L;                      // this lane's element behind the full slots
    const bool any_tail = nfull * L < len;             // (wave-uniform)
    gfloat* xr0 = (gfloat*)x;
    float v[R][S], vt[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {                      // every load first
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
        for (int b = 0; b < B; ++b) {                  // (uniform over the launch)
            const int num_bits = a.width_tab[b];
            QParams q = qparams_double(0.0, 1.0, num_bits, a.symmetric);     // qmin and qmax; the rest comes per candidate
            double best = 0.0;
            int kstar = 0;
            for (int base = 0; base < K; base += L) {  // (wave-uniform)
                // this lane's candidate of the pass: one run through the division for L candidates
                const int kc = base + g;
                float cl, ch;
                bx_candidate(mn, mx, a.alpha[kc < K ? kc : 0], cl, ch);
                const QParams cq = qparams_double((double)cl, (double)ch, num_bits, a.symmetric);
                const int n = K - base < L ? K - base : L;
                for (int kk = 0; kk < n; ++kk) {
                    q.scale = bx_bcast<L>(cq.scale, kk);
                    q.min_value = bx_bcast<L>(cq.min_value, kk);
                    const float kl = bx_bcast<L>(cl, kk), kh = bx_bcast<L>(ch, kk);
                    q.neg_min = -q.min_value;          // (in both recipes of qparams_double)
                    double s = 0.0;                    // a lane without the element adds +0.0: s + 0.0 == s
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        if (k >= nfull) break;
                        const double e2 = bx_sq_error(v[j][k], q, kl, kh);
                        s += live ? e2 : 0.0;
                    }
                    if (any_tail) {
                        const double e2 = bx_sq_error(vt[j], q, kl, kh);
                        s += tail ? e2 : 0.0;
                    }
                    s = bx_group_sum<L>(s);
                    if (base + kk == 0) best = s;
                    else if (s < best) { best = s; kstar = base + kk; }
                }
            }
            if (live && g == 0) {
                float l, h;
                bx_candidate(mn, mx, a.alpha[kstar], l, h);
                bx_unit_out(a, net, T.unit_off + r, T.part_begin + r, b, l, h, kstar, best);
            }
        }
    }
}

// bc_long_row with the widths around it: one wave per row longer than kMixRegElems; the row is read for the range and once per
// kMxLongAtOnce (candidate, width) pairs
__device__ __forceinline__ void bx_long_row(const BxArgs& a, const BxRowDev& T, float* x, int net, int r) {
    const int lane = threadIdx.x % kWave;
    const int len = T.len, K = a.K, B = a.n_widths;
    gfloat* xr = (gfloat*)x + (int64_t)r * len;
    float mn, mx;
    wave_row_range(xr, len, mn, mx);
    if (!(mn <= mx)) mn = mx = NAN;
    float cl, ch;                                      // lane k forms candidate k (K <= 64)
    bx_candidate(mn, mx, a.alpha[lane < K ? lane : 0], cl, ch);
    for (int b = 0; b < B; ++b) {
        const int num_bits = a.width_tab[b];
        const QParams cq = qparams_double((double)cl, (double)ch, num_bits, a.symmetric);
        double best = 0.0;
        int kstar = 0;
        for (int base = 0; base < K; base += kMxLongAtOnce) {
            const int n = K - base < kMxLongAtOnce ? K - base : kMxLongAtOnce;
            QParams q[kMxLongAtOnce];
            float kl[kMxLongAtOnce], kh[kMxLongAtOnce];
            double s[kMxLongAtOnce];
#pragma unroll
            for (int c = 0; c < kMxLongAtOnce; ++c) {
                const int kk = c < n ? base + c : base;
                q[c] = cq;
                q[c].scale = bx_bcast<kWave>(cq.scale, kk);
                q[c].min_value = bx_bcast<kWave>(cq.min_value, kk);
                kl[c] = bx_bcast<kWave>(cl, kk);
                kh[c] = bx_bcast<kWave>(ch, kk);
                q[c].neg_min = -q[c].min_value;
                s[c] = 0.0;
            }
            for (int i = lane; i < len; i += kWave) {
                const float w = xr[i];
#pragma unroll
                for (int c = 0; c < kMxLongAtOnce; ++c)
                    if (c < n) s[c] += bx_sq_error(w, q[c], kl[c], kh[c]);   // (wave-uniform)
            }
#pragma unroll
            for (int c = 0; c < kMxLongAtOnce; ++c) {
                if (c >= n) continue;                  // (wave-uniform)
                const double t = wave_sum(s[c]);
                if (base + c == 0) best = t;
                else if (t < best) { best = t; kstar = base + c; }
            }
        }
        if (lane == 0) {
            float l, h;
            bx_candidate(mn, mx, a.alpha[kstar], l, h);
            bx_unit_out(a, net, T.unit_off + r, T.part_begin + r, b, l, h, kstar, best);
        }
    }
}

// the units held in registers and the long rows: one launch
__global__ __launch_bounds__(kBlock) void bx_row_kernel(BxArgs a) {
    const int w = (int)blockIdx.x * (kBlock / kWave) + (int)threadIdx.x / kWave;
    if (w >= a.row_waves) return;                      // (wave-uniform)
    const int net = w / a.row_wpn;
    const int lw = w - net * a.row_wpn;
    const BxRowDev T = a.rows[a.wave_tensor[lw]];
    float* x = (float*)((char*)T.data + a.delta[net]);
    const int wi = lw - T.wave_begin;
    switch (T.cls) {
        case 1: bx_rows<4, kMixSmallPerLane, kMixGroupRows>(a, T, x, net, wi * 16 * kMixGroupRows); break;
        case 2: bx_rows<8, kMixSmallPerLane, kMixGroupRows>(a, T, x, net, wi * 8 * kMixGroupRows); break;
        case 3: bx_rows<16, kMixSmallPerLane, kMixGroupRows>(a, T, x, net, wi * 4 * kMixGroupRows); break;
        case 4: bx_rows<32, kMixSmallPerLane, kMixGroupRows>(a, T, x, net, wi * 2 * kMixGroupRows); break;
        case 5: bx_rows<64, kMixRegPerLane, 1>(a, T, x, net, wi); break;
        default: bx_long_row(a, T, x, net, wi); break;
    }
}

// ---- per-tensor tensors of more than kMixRegElems elements: flat pieces -------------------------------------------------------
struct BxPiece : BatchPiece {
    BxFlatDev T;
    gfloat* w;
    uint32_t* words;              // the tensor's pair
};

__device__ __forceinline__ BxPiece bx_piece(const BxArgs& a) {
    BxPiece p;
    (BatchPiece&)p = batch_piece(a.pieces_pn, a.piece_tensor, a.flats, p.T);
    p.w = (gfloat*)(float*)((char*)p.T.data + a.delta[p.net]) + p.start;
    p.words = a.words + 2 * ((int64_t)p.net * a.n_flats + p.T.index);
    return p;
}

// the piece's (min, max) into its tensor's words
__global__ __launch_bounds__(kBlock) void bx_range_kernel(BxArgs a) {
    const BxPiece p = bx_piece(a);
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

// the piece's B * K sums: a lane keeps its 16 elements across all of them
__global__ __launch_bounds__(kBlock) void bx_search_kernel(BxArgs a) {
    __shared__ float q_scale[kMxMaxPairs];
    __shared__ float q_minv[kMxMaxPairs];
    __shared__ float q_lo[kMxMaxCand];
    __shared__ float q_hi[kMxMaxCand];
    __shared__ double sh[kMxMaxPairs][kBlock / kWave];
    const BxPiece p = bx_piece(a);
    const int t = threadIdx.x;
    const int K = a.K, B = a.n_widths, BK = B * K;
    fvec4 x[kPieceInFlight];
    float xt;
    batch_piece_load<false>(p, p.w, x, xt);
    const float mn = slot_min(p.words[0]), mx = slot_max(p.words[1]);      // cleared words: (NaN, NaN)
    for (int i = t; i < BK; i += kBlock) {             // pair i = (width i / K, candidate i % K)
        const int b = i / K, k = i - b * K;
        float cl, ch;
        bx_candidate(mn, mx, a.alpha[k], cl, ch);
        const QParams cq = qparams_double((double)cl, (double)ch, a.width_tab[b], a.symmetric);
        q_scale[i] = cq.scale;
        q_minv[i] = cq.min_value;
        if (b == 0) { q_lo[k] = cl; q_hi[k] = ch; }
    }
    __syncthreads();
    const bool has_tail = (p.nv << 2) + t < p.count;
    for (int b = 0; b < B; ++b) {
        QParams q = qparams_double(0.0, 1.0, a.width_tab[b], a.symmetric);
        for (int k = 0; k < K; ++k) {
            q.scale = q_scale[b * K + k];
            q.min_value = q_minv[b * K + k];
            q.neg_min = -q.min_value;
            const float kl = q_lo[k], kh = q_hi[k];
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < kPieceInFlight; ++j) {
                if (j * kBlock + t < p.nv) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) s += bx_sq_error(x[j][c], q, kl, kh);
                }
            }
            if (has_tail) s += bx_sq_error(xt, q, kl, kh);
            s = wave_sum(s);
            if (t % kWave == 0) sh[b * K + k][t / kWave] = s;
        }
    }
    __syncthreads();
    for (int i = t; i < BK; i += kBlock) {             // block_sum's order: the four waves one after another
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) tot += sh[i][w];
        ((gdouble*)a.scratch)[((int64_t)p.net * a.pieces_pn + p.lp) * BK + i] = tot;
    }
}

// one wave per network and flat tensor; per width, lane k adds the pieces of candidate k in rising order and lane 0 draws k*
__global__ __launch_bounds__(kWave) void bx_fold_kernel(BxArgs a) {
    __shared__ double err[kMxMaxCand];
    const int net = (int)blockIdx.x / a.n_flats;
    const BxFlatDev T = a.flats[(int)blockIdx.x - net * a.n_flats];
    const int t = threadIdx.x, K = a.K, B = a.n_widths, BK = B * K;
    const uint32_t* words = a.words + 2 * ((int64_t)net * a.n_flats + T.index);
    const float mn = slot_min(words[0]), mx = slot_max(words[1]);
    for (int b = 0; b < B; ++b) {
        if (t < K) {
            const gdouble* part = (const gdouble*)a.scratch + ((int64_t)net * a.pieces_pn + T.piece_begin) * BK + b * K + t;
            double s = 0.0;
            for (int q = 0; q < T.n_pieces; ++q) s += part[(int64_t)q * BK];
            err[t] = s;
        }
        __syncthreads();
        if (t == 0) {
            double best = err[0];
            int kstar = 0;
            for (int k = 1; k < K; ++k)
                if (err[k] < best) { best = err[k]; kstar = k; }
            float l, h;
            bx_candidate(mn, mx, a.alpha[kstar], l, h);
            bx_unit_out(a, net, T.unit_off, T.part, b, l, h, kstar, best);
        }
        __syncthreads();
    }
}

// behind bm_alloc_kernel: the width it wrote for (network, tensor) as an index into the plan's own state, and the range
// block: (l, h) of the chosen width for every unit.  One thread per (network, unit).
__global__ __launch_bounds__(kBlock) void bx_finish_kernel(BxArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)a.n_nets * a.parts_pn) return;
    const int net = (int)(i / a.parts_pn);
    const int part = (int)(i - (int64_t)net * a.parts_pn);
    const int t = a.part_tensor[part];
    const BxTensorDev T = a.tensors[t];
    const int r = part - T.part_begin;
    const int B = a.n_widths;
    const int bits = ((const gint32m*)a.bits)[(int64_t)net * a.n_tensors + t];
    int j = 0;
    for (int b = 1; b < B; ++b)
        if (a.width_tab[b] == bits) j = b;
    if (r == 0) ((gint32m*)a.state)[(int64_t)net * a.n_tensors + t] = j;
    if (T.range_off < 0) return;
    const gfloat* cr = (const gfloat*)a.clip_ranges + 2 * (((int64_t)net * a.unit_stride + T.unit_off + r) * B + j);
    gfloat* rg = (gfloat*)a.ranges + (int64_t)net * a.range_stride + T.range_off + 2 * r;
    rg[0] = cr[0];
    rg[1] = cr[1];
}

// what the apply stages read for unit u of tensor `tensor` of network `net`: the chosen width, its ends and its k*
struct BxChoice {
    float l, h;
    int num_bits, kstar;
};

__device__ __forceinline__ BxChoice bx_choice(const BxArgs& a, int net, int tensor, int64_t u) {
    const int j = ((const gint32m*)a.state)[(int64_t)net * a.n_tensors + tensor];
    const int64_t at = ((int64_t)net * a.unit_stride + u) * a.n_widths + j;
    BxChoice c;
    c.l = ((const gfloat*)a.clip_ranges)[2 * at + 0];
    c.h = ((const gfloat*)a.clip_ranges)[2 * at + 1];
    c.kstar = ((const gint32m*)a.clip_chosen)[at];
    c.num_bits = a.width_tab[j];
    return c;
}

// one element of an apply stage: QUANT clamps and quantises it, else it is stored only if the clamp changes it
template <bool QUANT>
__device__ __forceinline__ void bx_apply_one(const BxArgs& a, gfloat* at, float w, const BxChoice& c, const QParams& q, unsigned char* codes, int64_t i) {
    if constexpr (QUANT) {
        float code;
        *at = fake_quant_one(bx_clamp(w, c.l, c.h), q, &code);
        if (codes) bm_store_code(codes, a.code_bytes, i, code);
    } else {
        if (w < c.l || w > c.h) *at = bx_clamp(w, c.l, c.h);
    }
}

// the rows of bx_rows once more, every load first, then the stage
template <int L, int S, int R, bool QUANT>
__device__ __forceinline__ void bx_apply_rows(const BxArgs& a, const BxRowDev& T, float* x, unsigned char* codes, int net, int first_row) {
    constexpr int G = kWave / L;
    const int lane = threadIdx.x % kWave;
    const int g = lane % L;
    const int r0 = first_row + lane / L;
    const int len = T.len;
    gfloat* xr0 = (gfloat*)x;
    float v[R][S];
#pragma unroll
    for (int j = 0; j < R; ++j) {
#pragma unroll
        for (int k = 0; k < S; ++k) v[j][k] = 0.0f;
        if (first_row + j * G >= T.rows) break;        // (wave-uniform)
        const int r = r0 + j * G;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            if (k * L >= len) break;                   // (wave-uniform)
            const int i = g + k * L;
            if (r < T.rows && i < len) v[j][k] = xr0[(int64_t)r * len + i];
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (first_row + j * G >= T.rows) break;
        const int r = r0 + j * G;
        if (r >= T.rows) continue;
        const BxChoice c = bx_choice(a, net, T.tensor, T.unit_off + r);
        if (!QUANT && c.kstar == 0) continue;          // candidate 0 is the unit's own range: nothing to store
        QParams q{};
        if constexpr (QUANT) q = qparams_double((double)c.l, (double)c.h, c.num_bits, a.symmetric);
#pragma unroll
        for (int k = 0; k < S; ++k) {
            if (k * L >= len) break;
            const int i = g + k * L;
            if (i < len) bx_apply_one<QUANT>(a, xr0 + (int64_t)r * len + i, v[j][k], c, q, codes, (int64_t)r * len + i);
        }
    }
}

template <bool QUANT>
__device__ __forceinline__ void bx_apply_long_row(const BxArgs& a, const BxRowDev& T, float* x, unsigned char* codes, int net, int r) {
    const int lane = threadIdx.x % kWave;
    const int len = T.len;
    gfloat* xr = (gfloat*)x + (int64_t)r * len;
    const BxChoice c = bx_choice(a, net, T.tensor, T.unit_off + r);
    if (!QUANT && c.kstar == 0) return;
    QParams q{};
    if constexpr (QUANT) q = qparams_double((double)c.l, (double)c.h, c.num_bits, a.symmetric);
    for (int i = lane; i < len; i += kWave) bx_apply_one<QUANT>(a, xr + i, xr[i], c, q, codes, (int64_t)r * len + i);
}

template <bool QUANT>
__device__ __forceinline__ void bx_apply_units(const BxArgs& a) {
    const int w = (int)blockIdx.x * (kBlock / kWave) + (int)threadIdx.x / kWave;
    if (w >= a.row_waves) return;                      // (wave-uniform)
    const int net = w / a.row_wpn;
    const int lw = w - net * a.row_wpn;
    const BxRowDev T = a.rows[a.wave_tensor[lw]];
    float* x = (float*)((char*)T.data + a.delta[net]);
    unsigned char* codes = QUANT && T.code_off >= 0 ? a.codes + ((int64_t)net * a.code_stride + T.code_off) * a.code_bytes : nullptr;
    const int wi = lw - T.wave_begin;
    switch (T.cls) {
        case 1: bx_apply_rows<4, kMixSmallPerLane, kMixGroupRows, QUANT>(a, T, x, codes, net, wi * 16 * kMixGroupRows); break;
        case 2: bx_apply_rows<8, kMixSmallPerLane, kMixGroupRows, QUANT>(a, T, x, codes, net, wi * 8 * kMixGroupRows); break;
        case 3: bx_apply_rows<16, kMixSmallPerLane, kMixGroupRows, QUANT>(a, T, x, codes, net, wi * 4 * kMixGroupRows); break;
        case 4: bx_apply_rows<32, kMixSmallPerLane, kMixGroupRows, QUANT>(a, T, x, codes, net, wi * 2 * kMixGroupRows); break;
        case 5: bx_apply_rows<64, kMixRegPerLane, 1, QUANT>(a, T, x, codes, net, wi); break;
        default: bx_apply_long_row<QUANT>(a, T, x, codes, net, wi); break;
    }
}

__global__ __launch_bounds__(kBlock) void bx_clamp_kernel(BxArgs a) { bx_apply_units<false>(a); }
__global__ __launch_bounds__(kBlock) void bx_quant_kernel(BxArgs a) { bx_apply_units<true>(a); }

// the flat pieces once more: a 16-byte vector stored only where the clamp changed it, or quantised
template <bool QUANT>
__device__ __forceinline__ void bx_apply_flat(const BxArgs& a) {
    const BxPiece p = bx_piece(a);
    const BxChoice c = bx_choice(a, p.net, p.T.tensor, p.T.unit_off);
    if (!QUANT && c.kstar == 0) return;                // (workgroup-uniform)
    QParams q{};
    if constexpr (QUANT) q = qparams_double((double)c.l, (double)c.h, c.num_bits, a.symmetric);
    unsigned char* codes = QUANT && p.T.code_off >= 0 ? a.codes + ((int64_t)p.net * a.code_stride + p.T.code_off) * a.code_bytes : nullptr;
    const int t = threadIdx.x;
    fvec4 x[kPieceInFlight];
    float xt;
    batch_piece_load<false>(p, p.w, x, xt);
#pragma unroll
    for (int j = 0; j < kPieceInFlight; ++j) {
        const int v = j * kBlock + t;
        if (v >= p.nv) continue;
        fvec4 y;
        bool changed = QUANT;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float w = x[j][e];
            if constexpr (QUANT) {
                float code;
                y[e] = fake_quant_one(bx_clamp(w, c.l, c.h), q, &code);
                if (codes) bm_store_code(codes, a.code_bytes, p.start + 4 * v + e, code);
            } else {
                changed = changed || w < c.l || w > c.h;
                y[e] = bx_clamp(w, c.l, c.h);
            }
        }
        if (changed) *(gfvec4*)(p.w + 4 * v) = y;
    }
    const int tail = (p.nv << 2) + t;
    if (tail < p.count) bx_apply_one<QUANT>(a, p.w + tail, xt, c, q, codes, p.start + tail);
}

__global__ __launch_bounds__(kBlock) void bx_clamp_flat_kernel(BxArgs a) { bx_apply_flat<false>(a); }
__global__ __launch_bounds__(kBlock) void bx_quant_flat_kernel(BxArgs a) { bx_apply_flat<true>(a); }

// stages of a plan WITHOUT clipping: the allocation bm_alloc_kernel left in the caller's bits block as an index in the plan's
// own state (capture, straight behind it), and back into the bits block in front of bm_quant_kernel (restore), which reads it
// there -- a caller's write in between changes nothing and cannot index past the tables.
__global__ __launch_bounds__(kBlock) void bm_state_kernel(const int32_t* width_tab, int n_widths, int32_t* bits, int32_t* state, int64_t n, int restore) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (restore) {
        ((gint32m*)bits)[i] = width_tab[((const gint32m*)state)[i]];
        return;
    }
    const int b = ((const gint32m*)bits)[i];
    int j = 0;
    for (int k = 1; k < n_widths; ++k)
        if (width_tab[k] == b) j = k;
    ((gint32m*)state)[i] = j;
}

}  // namespace dfq
