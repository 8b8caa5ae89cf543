// Bias absorption and weight clipping of a whole batch of networks of one architecture (extension: bias_absorption,
// dfq.py:121-164, followed by clip_weight, dfq.py:167-170, for every network of an arena.NetworkBatch at once).  The plan
// holds network 0's tables and one byte offset per network, like the replicated LE / BC plans and dfq_batch_quant_plan.
//
// Two launches, neither with a wait inside:
//   1. ab_shift_kernel, one thread per channel of every absorbed relation: c = max(0, beta~ - N*gamma~) goes to the
//      caller's block (the SNAPSHOT every later reader uses), beta~ -= c, and b1 -= c where the first layer's bias has
//      no other update in this plan.
//   2. ab_stream_kernel reads every weight once.  A second layer of an absorbed relation is read row by row into LDS with
//      coalesced 16-byte loads; the clamped values are stored from the same registers, a 16-byte piece only where the
//      clamp changed something, and the row sums are formed from the UNCLAMPED copy in LDS in the arithmetic order of
//      absorb_matvec_kernel (dfq_misc.hip): k sequentially in float32, channel i on lane i % 64 in float64 in rising i,
//      then wave_sum's butterfly.  Rows of at most 32 input channels get L = 2^k >= channels lanes, 64 / L rows per wave:
//      the lanes a row would leave idle in absorb_matvec_kernel hold +0.0 there, x + 0.0 == x for every x an accumulator
//      that started at +0.0 can hold, so the butterfly stages >= L change nothing and the stages < L stay inside the
//      row's lanes -- the sum is the same bit pattern.  The lane that owns bias element o applies its updates in the
//      order of the relations list: (b - c) + wc or (b + wc) - c when the layer is also a first layer.
//      Every other clipped layer is clamped in flat pieces of kFlatPerBlock floats.
// All waves of a workgroup work on the same layer, so the loop counts around __syncthreads are uniform.
#include <math.h>

#include <vector>

#include "dfq_batch_shared.hpp"

namespace dfq {

constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kAbLds = kWave * 49;                     // floats of LDS per wave: 64 channels of a 7x7 kernel
constexpr int kAbInFlight = 4;                         // 16-byte loads a lane issues before it uses the first
constexpr int kFlatPerWave = kWave * 4 * kAbInFlight;  // floats of a clip-only layer one wave clamps
constexpr int kFlatPerBlock = kFlatPerWave * kWavesPerBlock;

struct AbLayerDev {               // a weight tensor the streaming launch reads (network 0)
    float* w;
    float* b2;                    // null: clip only, in flat pieces
    int64_t n;                    // elements
    int64_t c2_off;               // the shift vector of the relation this layer is second of (floats into a network's block)
    int64_t c1_off;               // >= 0: the layer is also first of an absorbed relation, its bias shift is applied here
    int32_t first_before;         // ... in front of (1) or behind (0) the row sum, as the relations list orders them
    int32_t rows, ipg, khkw, step_o;
    int32_t lanes;                // lanes per row: 64 = a wave per row, looping over tiles of tile_ch channels
    int32_t tile_ch;
    int32_t clip;
    int32_t block_begin;          // first workgroup (within one network)
};

struct AbRelDev {                 // an absorbed relation (network 0)
    const float* fw;
    float* fb;
    float* b1;                    // null: the first layer's bias is shifted by the row owners of the streaming launch
    int64_t c_off;
    int32_t o1;
};

struct AbArgs {
    const AbLayerDev* layers;
    const int32_t* block_layer;   // layer of every workgroup of network 0
    const AbRelDev* rels;
    const int32_t* chan_rel;      // relation of every float of a network's shift block, -1 = padding
    const int64_t* delta;         // bases[n] - bases[0], bytes
    float* c_block;
    int64_t c_stride;
    float n_sigma, lo, hi;
    int32_t blocks_pn, n_nets;
};

__device__ __forceinline__ float ab_clamp(float v, float lo, float hi) {   // clamp_kernel's two selects (dfq_misc.hip)
    v = (v < lo) ? lo : v;
    v = (v > hi) ? hi : v;
    return v;
}

// `count` floats of `w` from element `start` on, by one wave: a copy to `lds` (if given), the clamped values back to memory
// (if `clip`) where they differ.  16-byte accesses when `start` allows them (every tensor starts on a 256-byte boundary).
__device__ __forceinline__ void ab_tile(gfloat* w, int64_t start, int count, float* lds, int clip, float lo, float hi) {
    const int lane = threadIdx.x % kWave;
    gfloat* p = w + start;
    int done = 0;
    if ((start & 3) == 0) {
        const int nv = count >> 2;
        for (int v0 = 0; v0 < nv; v0 += kWave * kAbInFlight) {
            fvec4 x[kAbInFlight];
#pragma unroll
            for (int j = 0; j < kAbInFlight; ++j) {
                const int v = v0 + j * kWave + lane;
                if (v < nv) x[j] = *(const gfvec4*)(p + 4 * v);
            }
#pragma unroll
            for (int j = 0; j < kAbInFlight; ++j) {
                const int v = v0 + j * kWave + lane;
                if (v >= nv) continue;
                if (lds) *(fvec4*)(lds + 4 * v) = x[j];
                if (clip) {
                    fvec4 y;
                    bool changed = false;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        y[e] = ab_clamp(x[j][e], lo, hi);
                        changed = changed || __float_as_uint(y[e]) != __float_as_uint(x[j][e]);
                    }
                    if (changed) *(gfvec4*)(p + 4 * v) = y;
                }
            }
        }
        done = nv << 2;
    }
    for (int e0 = done; e0 < count; e0 += kWave * kAbInFlight) {
        float x[kAbInFlight];
#pragma unroll
        for (int j = 0; j < kAbInFlight; ++j) {
            const int e = e0 + j * kWave + lane;
            if (e < count) x[j] = p[e];
        }
#pragma unroll
        for (int j = 0; j < kAbInFlight; ++j) {
            const int e = e0 + j * kWave + lane;
            if (e >= count) continue;
            if (lds) lds[e] = x[j];
            if (clip) {
                const float y = ab_clamp(x[j], lo, hi);
                if (__float_as_uint(y) != __float_as_uint(x[j])) p[e] = y;
            }
        }
    }
}

// bias element o of a second layer: the relations list's order of its (at most) two updates
__device__ __forceinline__ void ab_bias(const AbLayerDev& T, gfloat* b2, const gfloat* c1, int o, double acc) {
    float b = b2[o];
    if (c1 && T.first_before) b = b + (-c1[o]);
    b = b + (float)acc;
    if (c1 && !T.first_before) b = b + (-c1[o]);
    b2[o] = b;
}

// launch 1: the shift vectors, the BatchNorm proxies' means and the first layers' biases nobody else touches
__global__ __launch_bounds__(kBlock) void ab_shift_kernel(AbArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= a.c_stride * a.n_nets) return;
    const int net = (int)(t / a.c_stride);
    const int64_t j = t - (int64_t)net * a.c_stride;
    const int r = a.chan_rel[j];
    if (r < 0) return;
    const AbRelDev R = a.rels[r];
    const int i = (int)(j - R.c_off);
    const int64_t d = a.delta[net];
    const gfloat* fw = (const gfloat*)(const float*)((const char*)R.fw + d);
    gfloat* fb = (gfloat*)(float*)((char*)R.fb + d);
    const float nw = a.n_sigma * fw[i];            // absorb_shift_kernel, dfq_misc.hip
    float c = fb[i] - nw;
    c = (c < 0.0f) ? 0.0f : c;
    ((gfloat*)a.c_block)[t] = c;
    const float neg = -c;
    fb[i] = fb[i] + neg;
    if (R.b1) {
        gfloat* b1 = (gfloat*)(float*)((char*)R.b1 + d);
        b1[i] = b1[i] + neg;
    }
}

// launch 2: every weight read once
__global__ __launch_bounds__(kBlock) void ab_stream_kernel(AbArgs a) {
    __shared__ __attribute__((aligned(16))) float sh[kWavesPerBlock][kAbLds];
    const int net = (int)blockIdx.x / a.blocks_pn;
    const int lb = (int)blockIdx.x - net * a.blocks_pn;
    const AbLayerDev T = a.layers[a.block_layer[lb]];
    const int bi = lb - T.block_begin;
    const int64_t d = a.delta[net];
    gfloat* w = (gfloat*)(float*)((char*)T.w + d);
    const int wave = threadIdx.x / kWave;
    const int lane = threadIdx.x % kWave;
    if (!T.b2) {                                       // (block-uniform) a clip-only layer
        const int64_t s = (int64_t)bi * kFlatPerBlock + (int64_t)wave * kFlatPerWave;
        if (s < T.n) ab_tile(w, s, (int)(T.n - s < kFlatPerWave ? T.n - s : kFlatPerWave), nullptr, 1, a.lo, a.hi);
        return;
    }
    gfloat* b2 = (gfloat*)(float*)((char*)T.b2 + d);
    const gfloat* cn = (const gfloat*)a.c_block + (int64_t)net * a.c_stride;
    const gfloat* c2 = cn + T.c2_off;
    const gfloat* c1 = T.c1_off >= 0 ? cn + T.c1_off : nullptr;
    float* lds = sh[wave];
    const int khkw = T.khkw, ipg = T.ipg;
    const int len = ipg * khkw;
    if (T.lanes < kWave) {                             // (block-uniform) 64 / lanes whole rows per wave
        const int L = T.lanes, G = kWave / L;
        const int r0 = (bi * kWavesPerBlock + wave) * G;
        int nrows = T.rows - r0;
        nrows = nrows < 0 ? 0 : (nrows > G ? G : nrows);
        ab_tile(w, (int64_t)r0 * len, nrows * len, lds, T.clip, a.lo, a.hi);
        __syncthreads();
        const int q = lane / L, i = lane % L;
        const int r = r0 + q;
        double acc = 0.0;
        if (q < nrows && i < ipg) {
            const float* e = lds + q * len + i * khkw;
            float ws = 0.0f;
            for (int k = 0; k < khkw; ++k) ws = ws + e[k];
            acc += (double)ws * (double)c2[(r / T.step_o) * ipg + i];
        }
        if (L > 16) xor_lane_add<16>(acc);             // wave_sum's stages below L
        if (L > 8) xor_lane_add<8>(acc);
        if (L > 4) xor_lane_add<4>(acc);
        if (L > 2) xor_lane_add<2>(acc);
        if (L > 1) xor_lane_add<1>(acc);
        if (q < nrows && i == 0) ab_bias(T, b2, c1, r, acc);
        return;
    }
    const int r = bi * kWavesPerBlock + wave;          // a wave per row
    const bool live = r < T.rows;
    const gfloat* cg = c2 + (live ? (r / T.step_o) * ipg : 0);
    double acc = 0.0;
    for (int t0 = 0; t0 < ipg; t0 += T.tile_ch) {      // (block-uniform)
        const int tc = ipg - t0 < T.tile_ch ? ipg - t0 : T.tile_ch;
        if (t0) __syncthreads();                       // the tile before has been summed
        if (live) ab_tile(w, (int64_t)r * len + (int64_t)t0 * khkw, tc * khkw, lds, T.clip, a.lo, a.hi);
        __syncthreads();
        if (live)
            for (int i = t0 + ((lane - t0) & (kWave - 1)); i < t0 + tc; i += kWave) {   // channel i belongs to lane i % 64
                const float* e = lds + (i - t0) * khkw;
                float ws = 0.0f;
                for (int k = 0; k < khkw; ++k) ws = ws + e[k];
                acc += (double)ws * (double)cg[i];
            }
    }
    acc = wave_sum(acc);
    if (live && lane == 0) ab_bias(T, b2, c1, r, acc);
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_absorb_plan {
    DevSlab mem;
    AbArgs args{};
    int shift_blocks = 0, stream_blocks = 0;
    int64_t absorbed_elems = 0, clip_only_elems = 0;
};

extern "C" {

int32_t dfq_batch_absorb_plan_launches(const dfq_batch_absorb_plan* p) { return p ? (p->shift_blocks > 0) + (p->stream_blocks > 0) : 0; }

int dfq_batch_absorb_plan_elements(const dfq_batch_absorb_plan* p, int64_t* absorbed, int64_t* clip_only) {
    if (!p) return fail_arg("dfq_batch_absorb_plan_elements: null plan");
    if (absorbed) *absorbed = p->absorbed_elems;
    if (clip_only) *clip_only = p->clip_only_elems;
    return DFQ_OK;
}

void dfq_batch_absorb_plan_destroy(dfq_batch_absorb_plan* p) { batch_plan_destroy(p); }

int dfq_batch_absorb_plan_create(const dfq_batch_absorb_relation* relations, int32_t n_relations, const dfq_batch_absorb_clip* clips,
                                 int32_t n_clips, const void* const* bases, int32_t n_nets, float n_sigma, float lo, float hi,
                                 float* shifts, int64_t shift_stride, dfq_batch_absorb_plan** out_plan) {
    const char* me = "dfq_batch_absorb_plan_create";
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (n_relations < 0 || n_clips < 0 || (n_relations > 0 && !relations) || (n_clips > 0 && !clips))
        return fail_arg("%s: a table is null or its count negative", me);
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    if (n_relations > 0 && !isfinite(n_sigma)) return fail_arg("%s: n_sigma is not finite", me);
    if (n_clips > 0 && !(lo <= hi)) return fail_arg("%s: clip range [%g, %g] is empty or not a number", me, (double)lo, (double)hi);
    if (n_relations > 0 && (!shifts || shift_stride <= 0)) return fail_arg("%s: no block for the shift vectors", me);
    if (shift_stride < 0 || shift_stride > 0x7fffffff / n_nets) return fail_arg("%s: shift stride %lld out of range", me, (long long)shift_stride);

    std::vector<AbLayerDev> layers;
    std::vector<AbRelDev> rels;
    std::vector<int32_t> chan_rel(n_relations > 0 ? (size_t)shift_stride : 0, -1);
    for (int i = 0; i < n_relations; ++i) {
        const dfq_batch_absorb_relation& r = relations[i];
        if (!r.w2 || !r.b1 || !r.b2 || !r.bn_weight || !r.bn_bias || r.o2 <= 0 || r.in_per_group <= 0 || r.khkw <= 0 || r.o1 <= 0)
            return fail_arg("%s: relation %d: null tensor or empty shape", me, i);
        const int num_group = r.o1 / r.in_per_group;                                   // dfq.py:144, as dfq_bias_absorb
        if (num_group < 1 || num_group * r.in_per_group != r.o1 || r.o2 % num_group != 0)
            return fail_arg("%s: relation %d: unsupported geometry O1=%d I2/g=%d O2=%d", me, i, (int)r.o1, (int)r.in_per_group, (int)r.o2);
        if (r.khkw > kAbLds) return fail_arg("%s: relation %d: a kernel of %d taps", me, i, (int)r.khkw);
        if ((int64_t)r.in_per_group * r.khkw > 0x7fffffff / 2) return fail_arg("%s: relation %d: a row too long", me, i);
        if (r.shift_offset < 0 || r.shift_offset > shift_stride - r.o1)
            return fail_arg("%s: relation %d: shift vector overflows the shift stride", me, i);
        for (int j = 0; j < i; ++j) {
            const dfq_batch_absorb_relation& q = relations[j];
            if (q.w2 == r.w2 || q.b2 == r.b2) return fail_arg("%s: relations %d and %d share a second layer", me, j, i);
            if (q.b1 == r.b1 || q.bn_bias == r.bn_bias) return fail_arg("%s: relations %d and %d share a first layer", me, j, i);
        }
        for (int c = 0; c < r.o1; ++c) {
            if (chan_rel[r.shift_offset + c] >= 0) return fail_arg("%s: relation %d: shift vector overlaps another", me, i);
            chan_rel[r.shift_offset + c] = i;
        }
    }
    int64_t blocks = 0, absorbed = 0, clip_only = 0;
    std::vector<int32_t> block_layer;
    std::vector<char> clip_used((size_t)n_clips, 0);
    for (int i = 0; i < n_clips; ++i) {
        if (!clips[i].data || clips[i].n <= 0) return fail_arg("%s: clip tensor %d is empty", me, i);
        for (int j = 0; j < i; ++j)
            if (clips[j].data == clips[i].data) return fail_arg("%s: clip tensors %d and %d are the same", me, j, i);
    }
    auto add_blocks = [&](AbLayerDev& L, int64_t k) {
        L.block_begin = (int32_t)blocks;
        block_layer.insert(block_layer.end(), (size_t)k, (int32_t)layers.size());
        layers.push_back(L);
        blocks += k;
    };
    for (int i = 0; i < n_relations; ++i) {
        const dfq_batch_absorb_relation& r = relations[i];
        AbLayerDev L{};
        L.w = (float*)r.w2;
        L.b2 = r.b2;
        L.rows = r.o2; L.ipg = r.in_per_group; L.khkw = r.khkw;
        L.n = (int64_t)r.o2 * r.in_per_group * r.khkw;
        L.step_o = r.o2 / (r.o1 / r.in_per_group);
        L.c2_off = r.shift_offset;
        L.c1_off = -1;
        AbRelDev R{r.bn_weight, r.bn_bias, r.b1, r.shift_offset, r.o1};
        for (int j = 0; j < n_relations; ++j)          // is this second layer the first layer of relation j?
            if (relations[j].b1 == r.b2) {
                if (relations[j].o1 != r.o2) return fail_arg("%s: relations %d and %d disagree about a layer's channels", me, i, j);
                L.c1_off = relations[j].shift_offset;
                L.first_before = j < i;
            }
        for (int j = 0; j < n_relations; ++j)          // is this relation's first layer somebody's second layer?
            if (relations[j].b2 == r.b1) R.b1 = nullptr;
        for (int j = 0; j < n_clips; ++j)
            if (clips[j].data == r.w2) {
                if (clips[j].n != L.n) return fail_arg("%s: clip tensor %d and relation %d disagree about a weight's size", me, j, i);
                L.clip = 1;
                clip_used[j] = 1;
            }
        int lanes = 1;
        while (lanes < r.in_per_group && lanes < kWave) lanes *= 2;
        if (lanes < kWave && (int64_t)(kWave / lanes) * L.ipg * L.khkw > kAbLds) lanes = kWave;
        L.lanes = lanes;
        L.tile_ch = kAbLds / r.khkw >= kWave ? kAbLds / r.khkw / kWave * kWave : kAbLds / r.khkw;
        const int64_t rows_per_block = (int64_t)kWavesPerBlock * (kWave / lanes);
        add_blocks(L, (r.o2 + rows_per_block - 1) / rows_per_block);
        rels.push_back(R);
        absorbed += L.n;
    }
    for (int i = 0; i < n_clips; ++i) {
        if (clip_used[i]) continue;
        AbLayerDev L{};
        L.w = clips[i].data;
        L.n = clips[i].n;
        L.clip = 1;
        L.c1_off = L.c2_off = -1;
        add_blocks(L, (L.n + kFlatPerBlock - 1) / kFlatPerBlock);
        clip_only += L.n;
    }
    if (blocks * n_nets > 0x7fffffff) return fail_arg("%s: too much work for one launch", me);

    dfq_batch_absorb_plan* p = new dfq_batch_absorb_plan();
    AbArgs& a = p->args;
    a.c_block = shifts;
    a.c_stride = n_relations > 0 ? shift_stride : 0;
    a.n_sigma = n_sigma; a.lo = lo; a.hi = hi;
    a.blocks_pn = (int32_t)blocks;
    a.n_nets = n_nets;
    p->stream_blocks = (int)(blocks * n_nets);
    p->shift_blocks = (int)((a.c_stride * n_nets + kBlock - 1) / kBlock);
    p->absorbed_elems = absorbed;
    p->clip_only_elems = clip_only;
    BatchUpload up{p->mem};
    a.layers = up.put(layers);
    a.block_layer = up.put(block_layer);
    a.rels = up.put(rels);
    a.chan_rel = up.put(chan_rel);
    a.delta = up.put(batch_delta(bases, n_nets));
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch absorb plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_absorb_plan_run(dfq_batch_absorb_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_absorb_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    const AbArgs& a = p->args;
    if (p->shift_blocks > 0) {
        hipLaunchKernelGGL(ab_shift_kernel, dim3(p->shift_blocks), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
    }
    if (p->stream_blocks > 0) {
        hipLaunchKernelGGL(ab_stream_kernel, dim3(p->stream_blocks), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
    }
    return DFQ_OK;
}

}  // extern "C"
