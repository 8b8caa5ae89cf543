// Data-free layer sensitivities of a whole batch of networks of one architecture (extension; the costs dfq_batch_mixed_plan
// allocates on when they are set: dfq_batch_mixed_plan_set_costs).  The definition -- input moments, the noise-to-signal ratio
// of every output row at every candidate width, the fold per tensor -- is the comment of dfq_batch_nsr_plan_create
// (include/dfq_hip.h).  The plan holds network 0's tensor and source tables and one byte offset per network, like the other
// batch plans.  Launches, none with a wait inside:
//   0. bn_moment_kernel, one workgroup per (network, layer): a thread per input channel walks the layer's sources in order
//      (moments_of of dfq_act_shared.hpp: bit for bit dfq_relu_moments; float32 adds for `add`, the next channels for `cat`),
//      clamps and writes a_c.  A layer without sources gets input_moment.
//   1. (only per tensor) bn_chunk_minmax_kernel: every chunk of kNsrChunk elements into its tensor's pair of cleared
//      order-preserving words (atomicMax of enc_ord: min and max do not depend on the order of the merges).
//   2. bn_row_kernel, the hot one: a row of at most kNsrRegElems elements is held by L lanes, L in {4, 8, 16, 32, 64} by the
//      row length (the lane classes of dfq_mixed_batch.hip), in registers from its range through S and all B numerators --
//      B + 1 float64 accumulators per lane, the widths in the outer loop and the lane's elements in the inner one, then an
//      L-lane butterfly per accumulator (xor_lane_add: every lane ends with the same bits) and one division per width by the
//      row's first lane.  A row whose length is a multiple of 4 starts on 16 bytes and is loaded as 16-byte vectors (a lane
//      holds elements 4 (g + q L) .. + 3), any other row float by float (elements g + k L); which of the two, and L, follow
//      from the row length alone, and with them the order of the sums.  Rows longer than kNsrRegElems get a looping wave that
//      reads the row for its range and once more (from the cache) for the sums.  a_c is read through the cache: a layer's
//      vector is a few KB and every row of a group reads the same one.
//   3. bn_fold_kernel, one wave per (network, layer): lane j < B adds R[0][j], R[1][j], ... in rising o.
// No floating-point atomic anywhere: two runs are bit-identical, and network n's values depend on nothing but its own tensors.
#include <limits.h>
#include <math.h>

#include <vector>

#include "dfq_act_shared.hpp"
#include "dfq_batch_shared.hpp"
#include "dfq_range.hpp"

namespace dfq {

constexpr int kNsrMaxWidths = 8;
constexpr int kNsrRegPerLane = 24;                     // register slots per lane of the 64-lane class (kMixRegPerLane)
constexpr int64_t kNsrRegElems = (int64_t)kWave * kNsrRegPerLane;   // longest row kept in registers
constexpr int kNsrSmallPerLane = 4;                    // the classes L < 64 hold rows of at most 4 L elements,
constexpr int kNsrGroupRows = 4;                       // kNsrGroupRows of them per lane group
constexpr int kNsrChunk = kBlock * 16;                 // elements of a tensor one workgroup folds into the tensor's range

typedef DFQ_GLOBAL_AS double gdoublen;

struct BnSourceDev {
    const float* fw;              // gamma~ (null: mean = beta~, var = 0), network 0
    const float* fb;              // beta~
    int32_t channels, relu, concat, pad;
};

struct BnTensorDev {
    const float* data;            // network 0
    int64_t mom_off, row_off;     // into one network's moment / row block
    int32_t rows, len, klen;
    int32_t ipg, rpg;             // input channels per group (len / klen), rows per group
    int32_t channels;             // groups * ipg
    int32_t cls;                  // 0: one wave per row, looping; c > 0: L = 2 << c lanes per row
    int32_t vec;                  // len % 4 == 0: every row starts on 16 bytes
    int32_t wave_begin;           // first wave (within one network)
    int32_t chunk_begin;          // first chunk of the range launch (within one network)
    int32_t src_begin, src_count;
};

struct BnArgs {
    const BnTensorDev* tensors;
    const BnSourceDev* sources;
    const int32_t* wave_tensor;   // tensor of every wave of network 0
    const int32_t* chunk_tensor;  // tensor of every chunk of network 0
    const int64_t* delta;         // bases[n] - bases[0], bytes
    uint32_t* slots;              // [n_nets, n_tensors, 2]: ~enc_ord(min), enc_ord(max)
    float* moments;               // [n_nets, moment_stride]
    double* rows;                 // [n_nets, row_stride, n_widths]
    double* signal;               // [n_nets, row_stride], may be null
    double* costs;                // [n_nets, n_tensors, n_widths]
    int64_t moment_stride, row_stride;
    int32_t widths[kNsrMaxWidths];
    int32_t n_widths, symmetric, per_row, moment, n_tensors;
    int32_t row_wpn, row_waves, chunks_pn;
    float input_moment;
};

// launch 0: the input moments of layer blockIdx.x % T of network blockIdx.x / T
__global__ __launch_bounds__(kBlock) void bn_moment_kernel(BnArgs a) {
    const int net = (int)blockIdx.x / a.n_tensors;
    const BnTensorDev T = a.tensors[(int)blockIdx.x - net * a.n_tensors];
    gfloat* out = (gfloat*)a.moments + (int64_t)net * a.moment_stride + T.mom_off;
    for (int c = threadIdx.x; c < T.channels; c += kBlock) {
        if (T.src_count == 0) {                        // (uniform over the workgroup)
            out[c] = a.input_moment;
            continue;
        }
        float mean = 0.0f, var = 0.0f;
        int cur = 0;                                   // channels merged so far
        for (int m = 0; m < T.src_count; ++m) {
            const BnSourceDev s = a.sources[T.src_begin + m];
            const bool append = m == 0 || s.concat != 0;
            const int at = append ? c - cur : c;
            if (at >= 0 && at < s.channels) {
                const float b = ((const gfloat*)(const float*)((const char*)s.fb + a.delta[net]))[at];
                float mu = b, v = 0.0f;
                if (s.fw) moments_of(s.relu ? 1 : 0, ((const gfloat*)(const float*)((const char*)s.fw + a.delta[net]))[at], b, mu, v);
                if (append) { mean = mu; var = v; }
                else { mean = mean + mu; var = var + v; }                  // accumulate of dfq_relu_moments
            }
            if (append) cur += s.channels;
        }
        const float vc = var < 0.0f ? 0.0f : var;      // (NaN stays NaN)
        out[c] = a.moment == 0 ? vc : (float)((double)mean * (double)mean + (double)vc);
    }
}

// launch 1 (per tensor only): every chunk of every network folded into its tensor's slots
__global__ __launch_bounds__(kBlock) void bn_chunk_minmax_kernel(BnArgs a) {
    const int net = (int)blockIdx.x / a.chunks_pn;
    const int c = (int)blockIdx.x - net * a.chunks_pn;
    const int t = a.chunk_tensor[c];
    const BnTensorDev T = a.tensors[t];
    const int64_t n = (int64_t)T.rows * T.len;
    const int64_t b = (int64_t)(c - T.chunk_begin) * kNsrChunk;
    const float* x = (const float*)((const char*)T.data + a.delta[net]) + b;      // (16-byte aligned: so are data, delta and a chunk)
    float mn = INFINITY, mx = -INFINITY;
    range_span<4>(x, n - b < kNsrChunk ? n - b : kNsrChunk, mn, mx);
    block_range(mn, mx);
    if (threadIdx.x == 0) {                            // (nothing for a chunk of NaNs)
        uint32_t* slot = a.slots + 2 * ((int64_t)net * a.n_tensors + t);
        range_publish(mn, mx, slot + 0, slot + 1);
    }
}

// a_c * e^2 of one element, in float64: the square of two float32 is exact there, the product with a is one rounding
__device__ __forceinline__ double bn_noise(float w, double aa, const QParams& q) {
    float code;
    const double e = (double)(fake_quant_one(w, q, &code) - w);
    return aa * (e * e);
}

// the input channel of element i of a row whose group starts at channel cb
__device__ __forceinline__ int bn_channel(int cb, int i, int klen) { return cb + (klen == 1 ? i : (int)((uint32_t)i / (uint32_t)klen)); }

template <int L>
__device__ __forceinline__ void bn_lanes_add(double& v) {
    if constexpr (L > 1) xor_lane_add<1>(v);
    if constexpr (L > 2) xor_lane_add<2>(v);
    if constexpr (L > 4) xor_lane_add<4>(v);
    if constexpr (L > 8) xor_lane_add<8>(v);
    if constexpr (L > 16) xor_lane_add<16>(v);
    if constexpr (L > 32) xor_lane_add<32>(v);
}

// the row's results, by one lane of those that hold them
__device__ __forceinline__ void bn_store_row(const BnArgs& a, gdoublen* rout, gdoublen* sout, int r, double s, const double (&ne)[kNsrMaxWidths]) {
    if (sout) sout[r] = s;
#pragma unroll
    for (int b = 0; b < kNsrMaxWidths; ++b) {
        if (b >= a.n_widths) break;
        rout[(int64_t)r * a.n_widths + b] = s == 0.0 ? 0.0 : ne[b] / s;
    }
}

// R sets of 64 / L rows of one tensor from first_row on (row first_row + j * 64 / L + lane / L), L lanes each, K register slots
// per lane and row (len <= K * L).  VEC: slot k of lane g is element 4 (g + (k / 4) L) + k % 4, loaded four at a time; else
// element g + k L.  (tmn, tmx): the tensor's range of a per-tensor plan.
template <int L, int K, int R, bool VEC>
__device__ __forceinline__ void bn_rows(const BnArgs& a, const BnTensorDev& T, const gfloat* x, const gfloat* am, gdoublen* rout, gdoublen* sout,
                                        int first_row, float tmn, float tmx) {
    constexpr int G = kWave / L;
    const int lane = threadIdx.x % kWave;
    const int g = lane % L;
    const int r0 = first_row + lane / L;
    const int len = T.len;
    float v[R][K];                                     // every load first, the folds after them (see bq_rows)
#pragma unroll
    for (int j = 0; j < R; ++j) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[j][k] = 0.0f;
        if (first_row + j * G >= T.rows) break;        // (wave-uniform)
        const int r = r0 + j * G;
        if constexpr (VEC) {
#pragma unroll
            for (int q = 0; q < K / 4; ++q) {
                if (4 * q * L >= len) break;           // (wave-uniform)
                const int i = 4 * (g + q * L);
                if (r < T.rows && i < len) {           // (len % 4 == 0: the whole vector lies in the row)
                    const fvec4 t = *(const gfvec4*)(x + (int64_t)r * len + i);
                    v[j][4 * q + 0] = t[0]; v[j][4 * q + 1] = t[1]; v[j][4 * q + 2] = t[2]; v[j][4 * q + 3] = t[3];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (k * L >= len) break;               // (wave-uniform)
                const int i = g + k * L;
                if (r < T.rows && i < len) v[j][k] = x[(int64_t)r * len + i];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (first_row + j * G >= T.rows) break;
        const int r = r0 + j * G;
        const bool live = r < T.rows;
        const int cb = live ? (r / T.rpg) * T.ipg : 0;
        float mn = tmn, mx = tmx;
        if (a.per_row) {                               // (uniform over the launch)
            mn = INFINITY; mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = VEC ? 4 * (g + (k / 4) * L) + k % 4 : g + k * L;
                if ((VEC ? 4 * (k / 4) * L : k * L) >= len) break;
                if (live && i < len) range_fold(v[j][k], mn, mx);
            }
            if constexpr (L > 1) xor_lane_minmax<1>(mn, mx);
            if constexpr (L > 2) xor_lane_minmax<2>(mn, mx);
            if constexpr (L > 4) xor_lane_minmax<4>(mn, mx);
            if constexpr (L > 8) xor_lane_minmax<8>(mn, mx);
            if constexpr (L > 16) xor_lane_minmax<16>(mn, mx);
            if constexpr (L > 32) xor_lane_minmax<32>(mn, mx);
        }
        float av[K];                                   // the moments of the lane's elements
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            av[k] = 0.0f;
            const int i = VEC ? 4 * (g + (k / 4) * L) + k % 4 : g + k * L;
            if ((VEC ? 4 * (k / 4) * L : k * L) >= len) break;
            if (live && i < len) {
                av[k] = am[bn_channel(cb, i, T.klen)];
                const double w = (double)v[j][k];
                s += (double)av[k] * (w * w);
            }
        }
        double ne[kNsrMaxWidths];
#pragma unroll
        for (int b = 0; b < kNsrMaxWidths; ++b) {
            ne[b] = 0.0;
            if (b >= a.n_widths) continue;             // (uniform over the launch)
            const QParams p = qparams_double((double)mn, (double)mx, a.widths[b], a.symmetric);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = VEC ? 4 * (g + (k / 4) * L) + k % 4 : g + k * L;
                if ((VEC ? 4 * (k / 4) * L : k * L) >= len) break;
                if (live && i < len) ne[b] += bn_noise(v[j][k], (double)av[k], p);
            }
        }
        bn_lanes_add<L>(s);
#pragma unroll
        for (int b = 0; b < kNsrMaxWidths; ++b) {
            if (b >= a.n_widths) break;
            bn_lanes_add<L>(ne[b]);
        }
        if (live && g == 0) bn_store_row(a, rout, sout, r, s, ne);
    }
}

// one row longer than kNsrRegElems: one wave, the row read for its range (per row) and once more (from the cache) for the sums;
// VEC: lane l takes the vectors l, l + 64, ..., else the elements l, l + 64, ...
template <bool VEC>
__device__ __forceinline__ void bn_long_row(const BnArgs& a, const BnTensorDev& T, const gfloat* x, const gfloat* am, gdoublen* rout,
                                            gdoublen* sout, int r, float tmn, float tmx) {
    const int lane = threadIdx.x % kWave;
    const int len = T.len;
    const gfloat* xr = x + (int64_t)r * len;
    const int cb = (r / T.rpg) * T.ipg;
    float mn = tmn, mx = tmx;
    if (a.per_row) {
        if constexpr (VEC) {
            mn = INFINITY; mx = -INFINITY;
            for (int i = 4 * lane; i < len; i += 4 * kWave) {
                const fvec4 t = *(const gfvec4*)(xr + i);
                range_fold4(t, mn, mx);
            }
            wave_minmax(mn, mx);
        } else {
            wave_row_range(xr, len, mn, mx);
        }
    }
    QParams q[kNsrMaxWidths];
#pragma unroll
    for (int b = 0; b < kNsrMaxWidths; ++b)            // (constant indices: the table stays in registers)
        q[b] = qparams_double((double)mn, (double)mx, b < a.n_widths ? a.widths[b] : a.widths[0], a.symmetric);
    double s = 0.0, ne[kNsrMaxWidths];
#pragma unroll
    for (int b = 0; b < kNsrMaxWidths; ++b) ne[b] = 0.0;
    constexpr int E = VEC ? 4 : 1;
    for (int i = E * lane; i < len; i += E * kWave) {
        float w[E];
        if constexpr (VEC) {
            const fvec4 t = *(const gfvec4*)(xr + i);
            w[0] = t[0]; w[1] = t[1]; w[2] = t[2]; w[3] = t[3];
        } else {
            w[0] = xr[i];
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double aa = (double)am[bn_channel(cb, i + e, T.klen)];
            const double wd = (double)w[e];
            s += aa * (wd * wd);
#pragma unroll
            for (int b = 0; b < kNsrMaxWidths; ++b) {
                if (b >= a.n_widths) break;
                ne[b] += bn_noise(w[e], aa, q[b]);
            }
        }
    }
    s = wave_sum(s);
#pragma unroll
    for (int b = 0; b < kNsrMaxWidths; ++b) {
        if (b >= a.n_widths) break;
        ne[b] = wave_sum(ne[b]);
    }
    if (lane == 0) bn_store_row(a, rout, sout, r, s, ne);
}

template <bool VEC>
__device__ __forceinline__ void bn_dispatch(const BnArgs& a, const BnTensorDev& T, const gfloat* x, const gfloat* am, gdoublen* rout,
                                            gdoublen* sout, int wi, float tmn, float tmx) {
    switch (T.cls) {
        case 1: bn_rows<4, kNsrSmallPerLane, kNsrGroupRows, VEC>(a, T, x, am, rout, sout, wi * 16 * kNsrGroupRows, tmn, tmx); break;
        case 2: bn_rows<8, kNsrSmallPerLane, kNsrGroupRows, VEC>(a, T, x, am, rout, sout, wi * 8 * kNsrGroupRows, tmn, tmx); break;
        case 3: bn_rows<16, kNsrSmallPerLane, kNsrGroupRows, VEC>(a, T, x, am, rout, sout, wi * 4 * kNsrGroupRows, tmn, tmx); break;
        case 4: bn_rows<32, kNsrSmallPerLane, kNsrGroupRows, VEC>(a, T, x, am, rout, sout, wi * 2 * kNsrGroupRows, tmn, tmx); break;
        case 5: bn_rows<64, kNsrRegPerLane, 1, VEC>(a, T, x, am, rout, sout, wi, tmn, tmx); break;
        default: bn_long_row<VEC>(a, T, x, am, rout, sout, wi, tmn, tmx); break;
    }
}

// launch 2: a wave per row set
__global__ __launch_bounds__(kBlock) void bn_row_kernel(BnArgs a) {
    const int w = (int)blockIdx.x * (kBlock / kWave) + (int)threadIdx.x / kWave;
    if (w >= a.row_waves) return;                      // (wave-uniform)
    const int net = w / a.row_wpn;
    const int lw = w - net * a.row_wpn;
    const int t = a.wave_tensor[lw];
    const BnTensorDev T = a.tensors[t];
    const gfloat* x = (const gfloat*)(const float*)((const char*)T.data + a.delta[net]);
    const gfloat* am = (const gfloat*)a.moments + (int64_t)net * a.moment_stride + T.mom_off;
    gdoublen* rout = (gdoublen*)a.rows + ((int64_t)net * a.row_stride + T.row_off) * a.n_widths;
    gdoublen* sout = a.signal ? (gdoublen*)a.signal + (int64_t)net * a.row_stride + T.row_off : nullptr;
    float tmn = 0.0f, tmx = 0.0f;
    if (!a.per_row) {
        const uint32_t* slot = a.slots + 2 * ((int64_t)net * a.n_tensors + t);
        tmn = slot_min(slot[0]);
        tmx = slot_max(slot[1]);
    }
    if (T.vec) bn_dispatch<true>(a, T, x, am, rout, sout, lw - T.wave_begin, tmn, tmx);
    else bn_dispatch<false>(a, T, x, am, rout, sout, lw - T.wave_begin, tmn, tmx);
}

// launch 3: one wave per (network, tensor), lane j < B: N[j] = R[0][j] + R[1][j] + ... from 0.0
__global__ __launch_bounds__(kWave) void bn_fold_kernel(BnArgs a) {
    const int net = (int)blockIdx.x / a.n_tensors;
    const int t = (int)blockIdx.x - net * a.n_tensors;
    const int j = threadIdx.x;
    if (j >= a.n_widths) return;
    const BnTensorDev T = a.tensors[t];
    const gdoublen* r = (const gdoublen*)a.rows + ((int64_t)net * a.row_stride + T.row_off) * a.n_widths + j;
    double s = 0.0;
#pragma unroll 8
    for (int o = 0; o < T.rows; ++o) s += r[(int64_t)o * a.n_widths];
    ((gdoublen*)a.costs)[((int64_t)net * a.n_tensors + t) * a.n_widths + j] = s;
}

// lane class of a row of `len` elements: the fewest lanes that hold it in kNsrSmallPerLane slots, 64 up to kNsrRegElems, else 0
inline int bn_class(int64_t len) {
    for (int c = 1; c <= 4; ++c)
        if (len <= (int64_t)(2 << c) * kNsrSmallPerLane) return c;
    return len <= kNsrRegElems ? 5 : 0;
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_nsr_plan {
    DevSlab mem;
    BnArgs args{};
    int n_nets = 0, launches = 0;
};

extern "C" {

int32_t dfq_batch_nsr_plan_launches(const dfq_batch_nsr_plan* p) { return p ? p->launches : 0; }

void dfq_batch_nsr_plan_destroy(dfq_batch_nsr_plan* p) { batch_plan_destroy(p); }

int dfq_batch_nsr_plan_create(const dfq_batch_nsr_tensor* tensors, int32_t n_tensors, const dfq_bc_source* sources, int32_t n_sources,
                              const dfq_batch_nsr_config* config, const void* const* bases, int32_t n_nets, float* moments,
                              int64_t moment_stride, double* rows, double* signal, int64_t row_stride, double* costs,
                              dfq_batch_nsr_plan** out_plan) {
    const char* me = "dfq_batch_nsr_plan_create";
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (!tensors || n_tensors <= 0) return fail_arg("%s: the tensor table is null or empty (n_tensors %d)", me, (int)n_tensors);
    if (n_sources < 0 || (n_sources > 0 && !sources)) return fail_arg("%s: the source table is null (n_sources %d)", me, (int)n_sources);
    if (!config) return fail_arg("%s: no configuration", me);
    const dfq_batch_nsr_config cfg = *config;
    const int nb = cfg.n_widths;
    if (nb < 1 || nb > kNsrMaxWidths) return fail_arg("%s: %d candidate widths (1..%d)", me, nb, kNsrMaxWidths);
    for (int j = 0; j < nb; ++j) {
        if (cfg.widths[j] < 2 || cfg.widths[j] > 16) return fail_arg("%s: width %d is %d, outside [2, 16]", me, j, (int)cfg.widths[j]);
        if (j > 0 && cfg.widths[j] <= cfg.widths[j - 1])
            return fail_arg("%s: the widths do not rise (%d behind %d)", me, (int)cfg.widths[j], (int)cfg.widths[j - 1]);
    }
    if (cfg.moment != 0 && cfg.moment != 1) return fail_arg("%s: moment %d (0: variance, 1: second moment)", me, (int)cfg.moment);
    if (!(cfg.input_moment >= 0.0f) || !(cfg.input_moment <= 3.402823466e38f))
        return fail_arg("%s: an input_moment of %g (finite, >= 0)", me, (double)cfg.input_moment);
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    for (int n = 1; n < n_nets; ++n)
        if (((uintptr_t)bases[n] - (uintptr_t)bases[0]) % 16 != 0) return fail_arg("%s: network %d is not 16-byte aligned to network 0", me, n);
    if (!moments || !rows || !costs) return fail_arg("%s: a null output block (moments, rows, costs)", me);
    if (moment_stride < 0 || row_stride < 0) return fail_arg("%s: negative stride", me);
    const int per_row = cfg.per_row ? 1 : 0;

    std::vector<BnSourceDev> srcs((size_t)n_sources);
    for (int i = 0; i < n_sources; ++i) {
        const dfq_bc_source& s = sources[i];
        if (!s.fake_bias || (s.relu && !s.fake_weight) || s.channels <= 0) return fail_arg("%s: source %d: null BN proxy", me, i);
        srcs[i] = BnSourceDev{s.fake_weight, s.fake_bias, s.channels, s.relu ? 1 : 0, s.concat ? 1 : 0, 0};
    }
    std::vector<BnTensorDev> tens;
    std::vector<int32_t> wave_tensor, chunk_tensor;
    const int64_t most = 0x7fffffff / 4;               // waves or chunks of the whole batch in one launch
    int64_t waves = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_nsr_tensor& t = tensors[i];
        if (!t.data) return fail_arg("%s: tensor %d: null weight", me, i);
        if (t.rows <= 0 || t.row_len <= 0 || t.rows > 0x7fffffff - kWave || t.row_len > 0x7fffffff - 4 * kWave)
            return fail_arg("%s: tensor %d: a shape of [%lld, %lld]", me, i, (long long)t.rows, (long long)t.row_len);
        if ((uintptr_t)t.data % 16 != 0) return fail_arg("%s: tensor %d: the weight is not 16-byte aligned", me, i);
        if (t.kernel_len <= 0 || t.row_len % t.kernel_len != 0)
            return fail_arg("%s: tensor %d: rows of %lld weights in kernels of %lld", me, i, (long long)t.row_len, (long long)t.kernel_len);
        if (t.groups <= 0 || t.rows % t.groups != 0) return fail_arg("%s: tensor %d: %lld rows in %d groups", me, i, (long long)t.rows, (int)t.groups);
        const int64_t ipg = t.row_len / t.kernel_len, channels = ipg * t.groups;
        if (channels > 0x7fffffff - kBlock) return fail_arg("%s: tensor %d: %lld input channels", me, i, (long long)channels);
        if (t.source_count < 0 || t.source_begin < 0 || t.source_begin > n_sources - t.source_count)
            return fail_arg("%s: tensor %d: sources [%d, +%d) of %d", me, i, (int)t.source_begin, (int)t.source_count, (int)n_sources);
        if (t.source_count > 0) {
            int64_t have = 0;
            for (int m = 0; m < t.source_count; ++m) {
                const dfq_bc_source& s = sources[t.source_begin + m];
                if (m == 0) have = s.channels;
                else if (s.concat) have += s.channels;
                else if (s.channels != have)
                    return fail_arg("%s: tensor %d source %d: add of %d channels onto %lld", me, i, m, (int)s.channels, (long long)have);
            }
            if (have != channels)
                return fail_arg("%s: tensor %d: its sources give %lld channels, its shape reads %lld", me, i, (long long)have, (long long)channels);
        }
        if (t.moment_offset < 0 || t.moment_offset > moment_stride - channels) return fail_arg("%s: tensor %d: moments overflow the moment stride", me, i);
        if (t.row_offset < 0 || t.row_offset > row_stride - t.rows) return fail_arg("%s: tensor %d: rows overflow the row stride", me, i);
        BnTensorDev d{};
        d.data = t.data; d.mom_off = t.moment_offset; d.row_off = t.row_offset;
        d.rows = (int32_t)t.rows; d.len = (int32_t)t.row_len; d.klen = (int32_t)t.kernel_len;
        d.ipg = (int32_t)ipg; d.rpg = (int32_t)(t.rows / t.groups); d.channels = (int32_t)channels;
        d.cls = bn_class(t.row_len);
        d.vec = t.row_len % 4 == 0 ? 1 : 0;
        d.wave_begin = (int32_t)waves;
        d.chunk_begin = (int32_t)chunk_tensor.size();
        d.src_begin = t.source_begin; d.src_count = t.source_count;
        const int64_t per_wave = d.cls == 5 ? 1 : d.cls ? kWave / (2 << d.cls) * kNsrGroupRows : 1;
        const int64_t w = (t.rows + per_wave - 1) / per_wave;
        if ((waves + w) * n_nets > most) return fail_arg("%s: too much work for one launch", me);
        wave_tensor.insert(wave_tensor.end(), (size_t)w, (int32_t)i);
        waves += w;
        if (!per_row) {
            const int64_t k = (t.rows * t.row_len + kNsrChunk - 1) / kNsrChunk;
            if (((int64_t)chunk_tensor.size() + k) * n_nets > most) return fail_arg("%s: too much work for one launch", me);
            chunk_tensor.insert(chunk_tensor.end(), (size_t)k, (int32_t)i);
        }
        tens.push_back(d);
    }
    if ((int64_t)n_tensors * n_nets > most) return fail_arg("%s: too much work for one launch", me);

    dfq_batch_nsr_plan* p = new dfq_batch_nsr_plan();
    BnArgs& a = p->args;
    a.moments = moments;
    a.rows = rows;
    a.signal = signal;
    a.costs = costs;
    a.moment_stride = moment_stride;
    a.row_stride = row_stride;
    for (int j = 0; j < kNsrMaxWidths; ++j) a.widths[j] = j < nb ? cfg.widths[j] : 0;
    a.n_widths = nb;
    a.symmetric = cfg.symmetric ? 1 : 0;
    a.per_row = per_row;
    a.moment = cfg.moment;
    a.input_moment = cfg.input_moment;
    a.n_tensors = n_tensors;
    a.row_wpn = (int32_t)waves;
    a.row_waves = (int32_t)(waves * n_nets);
    a.chunks_pn = (int32_t)chunk_tensor.size();
    p->n_nets = n_nets;
    p->launches = 3 + (per_row ? 0 : 1);
    BatchUpload up{p->mem};
    a.tensors = up.put(tens);
    a.sources = up.put(srcs);
    a.wave_tensor = up.put(wave_tensor);
    a.chunk_tensor = up.put(chunk_tensor);
    a.delta = up.put(batch_delta(bases, n_nets));
    a.slots = per_row ? nullptr : (uint32_t*)up.raw(nullptr, sizeof(uint32_t) * 2 * (size_t)n_tensors * (size_t)n_nets);
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch nsr plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_nsr_plan_run(dfq_batch_nsr_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_nsr_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    const BnArgs& a = p->args;
    hipLaunchKernelGGL(bn_moment_kernel, dim3(a.n_tensors * p->n_nets), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    if (!a.per_row) {
        DFQ_HIP_TRY(hipMemsetAsync(a.slots, 0, sizeof(uint32_t) * 2 * (size_t)a.n_tensors * (size_t)p->n_nets, st));
        hipLaunchKernelGGL(bn_chunk_minmax_kernel, dim3(a.chunks_pn * p->n_nets), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(bn_row_kernel, dim3((a.row_waves + kBlock / kWave - 1) / (kBlock / kWave)), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_fold_kernel, dim3(a.n_tensors * p->n_nets), dim3(kWave), 0, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
