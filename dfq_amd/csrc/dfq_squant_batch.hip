// Data-free adaptive rounding of weights (extension; SQuant, ICLR 2022): round to nearest, then flip the few roundings that
// cost least so that every kernel's and every output row's sum of rounding errors is within half a quantum.  The DEFINITION
// is in include/dfq_hip.h ("Adaptive rounding"); everything below is integer arithmetic on P = llrint(p * 2^30), so a result
// depends on no summation order and on no launch shape.
//
// Work is per output row.  A row gets L lanes: L in {4, 8, 16, 32, 64} of one wave for rows of up to 4 L elements (so a wave
// takes 16 depthwise rows of 9 at a time), a whole wave with kRegPerLane register slots per lane up to kWaveElems, the
// workgroup up to kMaxRow (nothing in registers there: the row is read again from the cache).  A lane keeps t = clamp((w + neg_min) / scale) of its elements (i = g, g + L,
// ...) in registers from the one read to the one write; P lies in the LDS between the stages, where the lane that OWNS a
// kernel (kernel j: lane j % L) reaches all of its elements.
//   stage K  the owner of a kernel sums it and flips its n best elements one argmax at a time (n is a few; a flipped element
//            stops being a candidate, so n argmaxes are "the first n by key, ties by index").  Kernels longer than
//            kLaneKernel are selected by the whole group instead, one kernel after the other.
//   stage C  the owner holds its kernels' sums e_j in registers; the group finds "the first N by key, ties by j" by a
//            threshold search on the integer key (two bits a step, 15 steps) with shuffle-reduced counts, then a search on j among the keys that
//            equal the threshold, and every owner moves one element of each of its selected kernels.
// Every loop that holds a shuffle has a wave-uniform trip count (it depends on the tensor alone): lanes of rows past the
// tensor's end run along on zeros and store nothing.
#include <vector>

#include "dfq_batch_shared.hpp"
#include "dfq_range.hpp"

namespace dfq {

constexpr int kSqSmallPerLane = 4;                     // the classes L < 64 hold rows of at most 4 L elements
constexpr int kSqRegPerLane = 24;                      // slots per lane of the one-wave class
constexpr int kSqWaveElems = kWave * kSqRegPerLane;    // 1536
constexpr int kSqMaxRow = 16384;                       // longest row: the workgroup class, P of a row in the LDS
constexpr int kSqLaneKernel = 64;                      // longest kernel its owner lane selects on its own
constexpr int kSqChunkPerThread = 16;
constexpr int kSqChunk = kBlock * kSqChunkPerThread;   // elements of a per-tensor tensor one workgroup folds into its range
constexpr int32_t kSqOne = 1 << 30, kSqHalf = 1 << 29;

typedef DFQ_GLOBAL_AS int32_t sq_gint32;
typedef DFQ_GLOBAL_AS uint8_t sq_guint8;
typedef DFQ_GLOBAL_AS long long sq_gint64;

struct SqTensorDev {              // addresses in network 0
    const float* x;
    float* y;
    const float* mins;            // given ranges per row, or null
    const float* maxs;
    int64_t code_off, range_off, stats_off;   // into one network's block, -1 = none
    int32_t rows, len, klen;
    int32_t num_bits, symmetric;
    int32_t per_row;              // the range block holds a pair per row (else one for the tensor)
    int32_t slot;                 // per tensor: its pair of range words, -1 = none
    int32_t cls;                  // c in 1..5: L = 2 << c lanes, 4 slots; 6: a wave; 7: the workgroup
    int32_t item_begin;           // first wave (cls < 7) or workgroup (cls 7) within one network
    int32_t chunk_begin;          // first min/max chunk within one network (slot >= 0)
};

struct SqArgs {
    SqTensorDev one;              // the tensor of a single call (tensors == null)
    const SqTensorDev* tensors;
    const int32_t* wave_tensor;   // tensor of every wave item of network 0
    const int32_t* big_tensor;    // tensor of every workgroup item of network 0
    const int32_t* chunk_tensor;  // tensor of every min/max chunk of network 0
    const int64_t* delta;         // bases[n] - bases[0], bytes (null: one network)
    uint32_t* slots;              // [n_nets, n_slots, 2]: ~enc_ord(min), enc_ord(max)
    unsigned char* codes;
    float* ranges;
    long long* stats;
    int64_t code_stride, range_stride, stats_stride;
    int32_t code_bytes, n_slots;
    int32_t waves_pn, waves;      // wave items of one network, of all
    int32_t bigs_pn, bigs;
    int32_t chunks_pn, chunks;
};

// ---- a group of L lanes -------------------------------------------------------------------------------------------------------
// L <= 64: lanes of one wave, everything by shuffles.  L == kBlock: the workgroup, one LDS hop over its waves.
__device__ __forceinline__ void sq_wave_fence() {      // LDS written by one lane of the wave, read by another
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#else
    (void)__shfl_xor(0, 1);                            // (the emulation's lanes meet in a shuffle)
#endif
}

template <int L>
struct SqGroup {
    long long* sh;                // kBlock / kWave + 1 words of LDS (L == kBlock only)
    __device__ __forceinline__ void sync() const {
        if constexpr (L == kBlock) __syncthreads(); else sq_wave_fence();
    }
    __device__ __forceinline__ long long sum(long long v) const {
        constexpr int W = L < kWave ? L : kWave;
#pragma unroll
        for (int d = 1; d < W; d <<= 1) v += __shfl_xor(v, d);
        if constexpr (L == kBlock) {
            __syncthreads();                           // (the words may still be read from the sum before)
            if (threadIdx.x % kWave == 0) sh[threadIdx.x / kWave] = v;
            __syncthreads();
            v = 0;
#pragma unroll
            for (int w = 0; w < kBlock / kWave; ++w) v += sh[w];
        }
        return v;
    }
    __device__ __forceinline__ int sum(int v) const {
        if constexpr (L == kBlock) {
            return (int)sum((long long)v);
        } else {
#pragma unroll
            for (int d = 1; d < L; d <<= 1) v += __shfl_xor(v, d);
            return v;
        }
    }
    __device__ __forceinline__ void minmax(float& mn, float& mx) const {
        if constexpr (L == kBlock) { block_range(mn, mx); return; }
        if constexpr (L > 1) xor_lane_minmax<1>(mn, mx);
        if constexpr (L > 2) xor_lane_minmax<2>(mn, mx);
        if constexpr (L > 4) xor_lane_minmax<4>(mn, mx);
        if constexpr (L > 8) xor_lane_minmax<8>(mn, mx);
        if constexpr (L > 16) xor_lane_minmax<16>(mn, mx);
        if constexpr (L > 32 && L <= kWave) xor_lane_minmax<32>(mn, mx);
    }
};

// "The first n by key, ties by index" over the keys of the whole group: lane g answers key_of(m) for item g + m L, m < slots
// (0: no candidate); bit m of the result: the item is taken.  There are at least n candidates (n = 0: nothing is taken).  The
// largest T with #(key >= T) >= n, bit by bit; of the keys equal to T the r = n - #(key > T) lowest items, by the largest J
// with #(key == T, item < J) < r.  `slots` and idx_bits (items are below 1 << idx_bits) are wave-uniform.
template <int L, typename KeyOf>
__device__ __forceinline__ uint64_t sq_select(const SqGroup<L>& grp, KeyOf key_of, int g, int n, int slots, int idx_bits) {
    // two bits a step: the counts at three thresholds travel as one 64-bit sum (21 bits each; a row has at most 2^14 items),
    // and every key is read once per step
    constexpr long long kField = (1ll << 21) - 1;
    int32_t T = 0;
    for (int b = 28; b >= 0; b -= 2) {
        const int32_t c1 = T | (1 << b), c2 = T | (2 << b), c3 = T | (3 << b);
        long long cnt = 0;
        for (int m = 0; m < slots; ++m) {
            const int32_t key = key_of(m);
            cnt += (key >= c1 ? 1ll : 0ll) + (key >= c2 ? 1ll << 21 : 0ll) + (key >= c3 ? 1ll << 42 : 0ll);
        }
        cnt = grp.sum(cnt);
        if ((int)(cnt >> 42) >= n) T = c3;
        else if ((int)((cnt >> 21) & kField) >= n) T = c2;
        else if ((int)(cnt & kField) >= n) T = c1;
    }
    int above = 0;
    for (int m = 0; m < slots; ++m) above += key_of(m) > T ? 1 : 0;
    const int r = n - grp.sum(above);
    int J = 0;
    for (int b = (idx_bits + 1) / 2 * 2 - 2; b >= 0; b -= 2) {
        const int c1 = J | (1 << b), c2 = J | (2 << b), c3 = J | (3 << b);
        long long cnt = 0;
        for (int m = 0; m < slots; ++m) {
            const int item = g + m * L;
            if (key_of(m) == T) cnt += (item < c1 ? 1ll : 0ll) + (item < c2 ? 1ll << 21 : 0ll) + (item < c3 ? 1ll << 42 : 0ll);
        }
        cnt = grp.sum(cnt);
        if ((int)(cnt >> 42) < r) J = c3;
        else if ((int)((cnt >> 21) & kField) < r) J = c2;
        else if ((int)(cnt & kField) < r) J = c1;
    }
    uint64_t take = 0;
    if (n > 0 && T > 0) {
        for (int m = 0; m < slots; ++m) {
            const int32_t key = key_of(m);
            if (key > T || (key == T && g + m * L <= J)) take |= 1ull << m;
        }
    }
    return take;
}

// The value again, as one the compiler knows nothing about: the predicates `k < mine` of the three unrolled passes over a lane's
// slots are then compared afresh in each pass instead of being kept, E lane masks in scalar registers, across the stages
// between them (which spilled scalar registers).
__device__ __forceinline__ int sq_again(int x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#endif
    return x;
}

__device__ __forceinline__ int32_t sq_p_of(float t) {             // P of an element from its t (0 for a NaN)
    const float p = rintf(t) - t;
    return p == p ? (int32_t)llrint((double)p * 1073741824.0) : 0;
}

__device__ __forceinline__ int sq_bits_for(int n) {               // smallest b with n <= 1 << b
    int b = 0;
    while ((1 << b) < n) ++b;
    return b;
}

// in kernel [base, base + K) of sP: the element with the largest s P > 0, the lowest on a tie, moved by one (there is one)
__device__ __forceinline__ void sq_move_best(int32_t* sP, int base, int K, int s) {
    int32_t best = 0;
    int at = -1;
    for (int k = 0; k < K; ++k) {
        const int32_t key = s * sP[base + k];
        if (key > best) { best = key; at = k; }
    }
    if (at >= 0) sP[base + at] -= s * kSqOne;
}

// One row `r` of tensor T (network `net`) by a group of L lanes with E register slots each.  LDS of the group: sP, L * E words
// (P of every element), sE, half as many (the sums of the kernels, K > 1).  `live`: the row exists (group-uniform).
template <int L, int E>
__device__ __forceinline__ void sq_row(const SqArgs& a, const SqTensorDev& T, int net, int r, bool live, int32_t* sP, int32_t* sE,
                                       const SqGroup<L>& grp) {
    const int g = (int)threadIdx.x % L;
    const int len = T.len, K = T.klen;
    const int slots = (len + L - 1) / L;               // register slots in use (wave-uniform)
    const int64_t dbytes = a.delta ? a.delta[net] : 0;
    const gfloat* x = (const gfloat*)(const float*)((const char*)T.x + dbytes) + (int64_t)r * len;
    gfloat* y = (gfloat*)(float*)((char*)T.y + dbytes) + (int64_t)r * len;

    // E > 0: the lane's elements stay in v[] from the one read to the one write.  E == 0 (the workgroup's rows): nothing is
    // kept, the row is read again for t and for the write (from the cache, as dfq_batch_quant_plan reads its long rows)
    float v[E > 0 ? E : 1];
    const int mine0 = live && g < len ? (len - g + L - 1) / L : 0;      // the lane's elements: g + k L, k < mine
    int mine = sq_again(mine0);
    if constexpr (E > 0) {
#pragma unroll
        for (int k = 0; k < E; ++k) {
            v[k] = 0.0f;
            if (k < mine) v[k] = x[g + k * L];
        }
    }
    float mn = 0.0f, mx = 0.0f;
    if (T.slot >= 0) {
        const uint32_t* slot = a.slots + 2 * ((int64_t)net * a.n_slots + T.slot);
        mn = slot_min(slot[0]);
        mx = slot_max(slot[1]);
    } else if (T.mins) {
        if (live) { mn = ((const gfloat*)T.mins)[r]; mx = ((const gfloat*)T.maxs)[r]; }
    } else {
        mn = INFINITY;
        mx = -INFINITY;
        if constexpr (E > 0) {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                if (k < mine) range_fold(v[k], mn, mx);
            }
        } else {
            for (int i = g; i < len; i += L) range_fold(x[i], mn, mx);
        }
        grp.minmax(mn, mx);
        if (!live) { mn = 0.0f; mx = 0.0f; }
    }
    if (live && g == 0 && T.range_off >= 0 && (T.per_row || r == 0)) {
        gfloat* rg = (gfloat*)a.ranges + (int64_t)net * a.range_stride + T.range_off + (T.per_row ? 2 * (int64_t)r : 0);
        rg[0] = mn;
        rg[1] = mx;
    }
    const QParams q = qparams_double((double)mn, (double)mx, T.num_bits, T.symmetric);
    const float fin = q.scale - q.scale + (q.neg_min - q.neg_min) + (q.min_value - q.min_value);   // 0, or NaN for a non-finite one

    // t in the registers, P in the LDS
    int bad = fin == fin ? 0 : 1;
    const auto t_of = [&](float w) -> float {
        float t = w + q.neg_min;
        t = t / q.scale;
        t = (t < q.qmin) ? q.qmin : t;     // NaN-propagating clamp, as fake_quant_one
        t = (t > q.qmax) ? q.qmax : t;
        return t;
    };
    if constexpr (E > 0) {
        mine = sq_again(len > g ? (len - g + L - 1) / L : 0);          // (a row that is not there computes on zeros)
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const float t = t_of(v[k]);
            v[k] = t;
            if (k < mine) {
                bad |= t == t ? 0 : 1;
                sP[g + k * L] = sq_p_of(t);
            }
        }
    } else {
        for (int i = g; i < len; i += L) {
            const float t = t_of(x[i]);
            bad |= t == t ? 0 : 1;
            sP[i] = sq_p_of(t);
        }
    }
    const bool flip = grp.sum(bad) == 0 && live;       // else: the row is stored as rounded to nearest
    grp.sync();

    const int G = len / K;
    const int kslots = (G + L - 1) / L;                // kernels per lane (wave-uniform); lane g owns the kernels g + m L

    // ---- stage K ---------------------------------------------------------------------------------------------------------------
    if (K > 1 && K <= kSqLaneKernel) {
        for (int m = 0; m < kslots; ++m) {
            const int j = g + m * L;
            if (j >= G) break;
            long long e0 = 0;
            for (int k = 0; k < K; ++k) e0 += sP[j * K + k];
            const int s = e0 > 0 ? 1 : (e0 < 0 ? -1 : 0);
            const int n = flip ? (int)(((e0 < 0 ? -e0 : e0) + kSqHalf) >> 30) : 0;
            for (int c = 0; c < n; ++c) sq_move_best(sP, j * K, K, s);
            sE[j] = (int32_t)(e0 - (long long)n * s * kSqOne);
        }
        grp.sync();
    } else if (K > 1) {
        // a long kernel: the group selects among the elements of kernel j, each lane among its own
        const int ebits = sq_bits_for(len);
        for (int j = 0; j < G; ++j) {
            const int lo = j * K, hi = lo + K;
            long long e0 = 0;
            for (int m = 0; m < slots; ++m) {
                const int i = g + m * L;
                e0 += (i >= lo && i < hi) ? sP[i] : 0;
            }
            e0 = grp.sum(e0);
            const int s = e0 > 0 ? 1 : (e0 < 0 ? -1 : 0);
            const int n = flip ? (int)(((e0 < 0 ? -e0 : e0) + kSqHalf) >> 30) : 0;
            const uint64_t take = sq_select<L>(grp, [&](int m) -> int32_t {
                const int i = g + m * L;
                const int32_t key = (i >= lo && i < hi) ? s * sP[i] : 0;
                return key > 0 ? key : 0;
            }, g, n, slots, ebits);
            for (int m = 0; m < slots; ++m)
                if ((take >> m) & 1) sP[g + m * L] -= s * kSqOne;
            if (g == 0) sE[j] = (int32_t)(e0 - (long long)n * s * kSqOne);
        }
        grp.sync();
    }

    // ---- stage C ---------------------------------------------------------------------------------------------------------------
    const int32_t* e_at = K == 1 ? sP : sE;
    long long Erow = 0;
    for (int m = 0; m < kslots; ++m) {
        const int j = g + m * L;
        Erow += (flip && j < G) ? e_at[j] : 0;
    }
    Erow = grp.sum(Erow);
    const int S = Erow > 0 ? 1 : (Erow < 0 ? -1 : 0);
    const int N = (int)(((Erow < 0 ? -Erow : Erow) + kSqHalf) >> 30);
    const uint64_t take = sq_select<L>(grp, [&](int m) -> int32_t {
        const int j = g + m * L;
        const int32_t key = (flip && j < G) ? S * e_at[j] : 0;
        return key > 0 ? key : 0;
    }, g, N, kslots, sq_bits_for(G));
    for (int m = 0; m < kslots; ++m) {
        if (!((take >> m) & 1)) continue;
        if (K == 1) sP[g + m * L] -= S * kSqOne;
        else sq_move_best(sP, (g + m * L) * K, K, S);
    }
    grp.sync();

    // ---- the one write -----------------------------------------------------------------------------------------------------------
    unsigned char* codes = T.code_off >= 0 ? a.codes + ((int64_t)net * a.code_stride + T.code_off + (int64_t)r * len) * a.code_bytes : nullptr;
    long long psum = 0;
    int moved = 0;
    const auto store = [&](int i, float t) {
        const int32_t pf = sP[i];
        const int d = (sq_p_of(t) - pf) >> 30;          // -1, 0, 1
        const float c = rintf(t) - (float)d;
        float w = c * q.scale;
        w = w + q.min_value;
        y[i] = w;
        if (codes) {
            const int32_t ci = c == c ? (int32_t)c : 0;
            if (a.code_bytes == 4) ((sq_gint32*)codes)[i] = ci;
            else ((sq_guint8*)codes)[i] = (uint8_t)ci;
        }
        psum += flip ? pf : 0;
        moved += d != 0 ? 1 : 0;
    };
    if constexpr (E > 0) {
        mine = sq_again(mine0);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            if (k < mine) store(g + k * L, v[k]);
        }
    } else {
        for (int i = g; i < len; i += L) store(i, t_of(x[i]));
    }
    if (T.stats_off >= 0) {                            // (uniform over the tensor)
        psum = grp.sum(psum);
        moved = grp.sum(moved);
        if (live && g == 0) {
            sq_gint64* st = (sq_gint64*)a.stats + (int64_t)net * a.stats_stride + T.stats_off + 2 * (int64_t)r;
            st[0] = psum;
            st[1] = moved;
        }
    }
}

// A width per (network, tensor), read on the device (dfq_batch_squant_plan_set_widths): the second argument of the two
// *_widths_kernel instantiations.  An item -- a wave of the rows kernel, a workgroup of the long-rows kernel -- belongs to one
// tensor of one network, so its width is one scalar load.
struct SqWidths {
    const int32_t* widths;        // [n_nets, stride]
    const int32_t* index;         // [n_tensors]: the tensor's place in a network's row of `widths`
    int32_t* status;              // [n_nets], cleared in front of the launches; 2: a width that is no width
    int64_t stride;
};

// The width of tensor ti of network `net`, or 0: it is no width (outside [2, 16], or above 8 where the tensor writes one-byte
// codes); status[net] is then 2 and the item must write nothing else.  Everything here is uniform over the item.
__device__ __forceinline__ int sq_width_of(const SqArgs& a, const SqWidths& wd, int net, int ti) {
    const int bits = __builtin_amdgcn_readfirstlane(wd.widths[(int64_t)net * wd.stride + wd.index[ti]]);
    if (bits < 2 || bits > 16 || (bits > 8 && a.code_bytes == 1 && a.tensors[ti].code_off >= 0)) {
        if (threadIdx.x % kWave == 0) ((sq_gint32*)wd.status)[net] = 2;
        return 0;
    }
    return bits;
}

// rows of up to kSqWaveElems elements: a wave per item, 64 / L rows of one tensor each
template <bool kDeviceWidths>
__device__ __forceinline__ void sq_rows_item(const SqArgs& a, const SqWidths& wd) {
    __shared__ int32_t sP[kBlock / kWave][kSqWaveElems];       // (of the one kernel this instantiation is the body of)
    __shared__ int32_t sE[kBlock / kWave][kSqWaveElems / 2];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int w = (int)blockIdx.x * (kBlock / kWave) + wave;
    if (w >= a.waves) return;                          // (wave-uniform; no workgroup barrier in this kernel)
    const int net = w / a.waves_pn;
    const int lw = w - net * a.waves_pn;
    int bits = 0;
    if constexpr (kDeviceWidths) {                     // (a plan's launch: the tensors are a table)
        bits = sq_width_of(a, wd, net, a.wave_tensor[lw]);
        if (bits == 0) return;                         // (the whole wave, before any shuffle)
    }
    SqTensorDev T = a.tensors ? a.tensors[a.wave_tensor[lw]] : a.one;
    if constexpr (kDeviceWidths) T.num_bits = bits;
    const int wi = lw - T.item_begin;
    const int lane = (int)threadIdx.x % kWave;
    int32_t* mine = sP[wave];
    int32_t* sums = sE[wave];
    switch (T.cls) {
#define DFQ_SQ_CASE(c, L)                                                                                              \
    case c: {                                                                                                          \
        const int r = wi * (kWave / L) + lane / L;                                                                     \
        sq_row<L, kSqSmallPerLane>(a, T, net, r, r < T.rows, mine + (lane / L) * L * kSqSmallPerLane,                \
                                   sums + (lane / L) * L * kSqSmallPerLane / 2, SqGroup<L>{nullptr});                  \
    } break;
        DFQ_SQ_CASE(1, 4)
        DFQ_SQ_CASE(2, 8)
        DFQ_SQ_CASE(3, 16)
        DFQ_SQ_CASE(4, 32)
        DFQ_SQ_CASE(5, 64)
#undef DFQ_SQ_CASE
        default: sq_row<kWave, kSqRegPerLane>(a, T, net, wi, wi < T.rows, mine, sums, SqGroup<kWave>{nullptr}); break;
    }
}

__global__ __launch_bounds__(kBlock) void squant_rows_kernel(SqArgs a) { sq_rows_item<false>(a, SqWidths{}); }
__global__ __launch_bounds__(kBlock) void squant_rows_widths_kernel(SqArgs a, SqWidths wd) { sq_rows_item<true>(a, wd); }

// rows of up to kSqMaxRow elements: a workgroup per row
template <bool kDeviceWidths>
__device__ __forceinline__ void sq_long_rows_item(const SqArgs& a, const SqWidths& wd) {
    __shared__ int32_t sP[kSqMaxRow];
    __shared__ int32_t sE[kSqMaxRow / 2];
    __shared__ long long sh[kBlock / kWave];
    const int net = (int)blockIdx.x / a.bigs_pn;
    const int lb = (int)blockIdx.x - net * a.bigs_pn;
    int bits = 0;
    if constexpr (kDeviceWidths) {
        bits = sq_width_of(a, wd, net, a.big_tensor[lb]);
        if (bits == 0) return;                         // (the whole workgroup, before any barrier)
    }
    SqTensorDev T = a.tensors ? a.tensors[a.big_tensor[lb]] : a.one;
    if constexpr (kDeviceWidths) T.num_bits = bits;
    sq_row<kBlock, 0>(a, T, net, lb - T.item_begin, true, sP, sE, SqGroup<kBlock>{sh});
}

__global__ __launch_bounds__(kBlock) void squant_long_rows_kernel(SqArgs a) { sq_long_rows_item<false>(a, SqWidths{}); }
__global__ __launch_bounds__(kBlock) void squant_long_rows_widths_kernel(SqArgs a, SqWidths wd) { sq_long_rows_item<true>(a, wd); }

// per-tensor ranges: every chunk of every network folded into its tensor's pair of words
__global__ __launch_bounds__(kBlock) void squant_minmax_kernel(SqArgs a) {
    const int net = (int)blockIdx.x / a.chunks_pn;
    const int c = (int)blockIdx.x - net * a.chunks_pn;
    const SqTensorDev T = a.tensors[a.chunk_tensor[c]];
    const gfloat* x = (const gfloat*)(const float*)((const char*)T.x + a.delta[net]);
    const int64_t n = (int64_t)T.rows * T.len;
    const int64_t b = (int64_t)(c - T.chunk_begin) * kSqChunk;
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kSqChunkPerThread; ++j) {
        const int64_t i = b + j * kBlock + threadIdx.x;
        if (i < n) range_fold(x[i], mn, mx);
    }
    block_range(mn, mx);
    if (threadIdx.x == 0) {
        uint32_t* slot = a.slots + 2 * ((int64_t)net * a.n_slots + T.slot);
        range_publish(mn, mx, slot + 0, slot + 1);
    }
}

// class of a row of `len` elements
inline int sq_class(int64_t len) {
    for (int c = 1; c <= 5; ++c)
        if (len <= (int64_t)(2 << c) * kSqSmallPerLane) return c;
    return len <= kSqWaveElems ? 6 : 7;
}
inline int64_t sq_rows_per_wave(int cls) { return cls <= 5 ? kWave / (2 << cls) : 1; }

// wd: null, or the widths of a plan (its tensors are a table), read by the *_widths_kernel pair in place of the other two
inline int sq_launch(const SqArgs& a, hipStream_t st, const SqWidths* wd = nullptr, int n_nets = 0) {
    if (wd) DFQ_HIP_TRY(hipMemsetAsync(wd->status, 0, sizeof(int32_t) * (size_t)n_nets, st));
    if (a.chunks > 0) {
        DFQ_HIP_TRY(hipMemsetAsync(a.slots, 0, sizeof(uint32_t) * 2 * (size_t)a.n_slots * (size_t)(a.chunks / a.chunks_pn), st));
        hipLaunchKernelGGL(squant_minmax_kernel, dim3(a.chunks), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
    }
    if (a.waves > 0) {
        const dim3 grid((a.waves + kBlock / kWave - 1) / (kBlock / kWave));
        if (wd) {
            hipLaunchKernelGGL(squant_rows_widths_kernel, grid, dim3(kBlock), 0, st, a, *wd);
        } else {
            hipLaunchKernelGGL(squant_rows_kernel, grid, dim3(kBlock), 0, st, a);
        }
        DFQ_CHECK_LAUNCH();
    }
    if (a.bigs > 0) {
        if (wd) {
            hipLaunchKernelGGL(squant_long_rows_widths_kernel, dim3(a.bigs), dim3(kBlock), 0, st, a, *wd);
        } else {
            hipLaunchKernelGGL(squant_long_rows_kernel, dim3(a.bigs), dim3(kBlock), 0, st, a);
        }
        DFQ_CHECK_LAUNCH();
    }
    return DFQ_OK;
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_squant_plan {
    DevSlab mem;
    SqArgs args{};
    SqWidths widths{};            // widths.widths null: the table's widths (set_widths)
    int32_t n_nets = 0, n_tensors = 0;
    int launches = 1;
};

extern "C" {

int64_t dfq_squant_max_row_len(void) { return kSqMaxRow; }

int dfq_squant_rows(const float* x, float* y, int64_t rows, int64_t row_len, int64_t kernel_len, const float* mins, const float* maxs,
                    int32_t num_bits, int32_t symmetric, int32_t* codes, int64_t* stats, void* stream) {
    const char* me = "dfq_squant_rows";
    if (!x || !y || rows <= 0 || row_len <= 0) return fail_arg("%s: null or empty tensor", me);
    if ((mins == nullptr) != (maxs == nullptr)) return fail_arg("%s: mins and maxs go together", me);
    if (num_bits < 2 || num_bits > 16) return fail_arg("%s: num_bits %d outside [2, 16]", me, (int)num_bits);
    if (kernel_len <= 0 || row_len % kernel_len != 0) return fail_arg("%s: row_len %lld is no multiple of kernel_len %lld", me, (long long)row_len, (long long)kernel_len);
    if (row_len > kSqMaxRow) return fail_arg("%s: row_len %lld above dfq_squant_max_row_len() = %d", me, (long long)row_len, kSqMaxRow);
    if (rows > 0x7fffffff / 2) return fail_arg("%s: too many rows", me);
    SqArgs a{};
    SqTensorDev& t = a.one;
    t.x = x; t.y = y; t.mins = mins; t.maxs = maxs;
    t.code_off = codes ? 0 : -1; t.range_off = -1; t.stats_off = stats ? 0 : -1;
    t.rows = (int32_t)rows; t.len = (int32_t)row_len; t.klen = (int32_t)kernel_len;
    t.num_bits = num_bits; t.symmetric = symmetric ? 1 : 0; t.per_row = 1; t.slot = -1;
    t.cls = sq_class(row_len);
    a.codes = (unsigned char*)codes;
    a.stats = (long long*)stats;
    a.code_bytes = 4;
    if (t.cls == 7) { a.bigs_pn = a.bigs = t.rows; }
    else {
        const int64_t per = sq_rows_per_wave(t.cls);
        a.waves_pn = a.waves = (int32_t)((rows + per - 1) / per);
    }
    return sq_launch(a, as_stream(stream));
}

int32_t dfq_batch_squant_plan_launches(const dfq_batch_squant_plan* p) { return p ? p->launches : 0; }

void dfq_batch_squant_plan_destroy(dfq_batch_squant_plan* p) { batch_plan_destroy(p); }

int dfq_batch_squant_plan_create(const dfq_batch_squant_tensor* tensors, int32_t n_tensors, const void* const* bases, int32_t n_nets,
                                 void* codes, int32_t code_bytes, int64_t code_stride, float* ranges, int64_t range_stride,
                                 int64_t* stats, int64_t stats_stride, dfq_batch_squant_plan** out_plan) {
    const char* me = "dfq_batch_squant_plan_create";
    if (!tensors || n_tensors <= 0 || !out_plan) return fail_arg("%s: no tensors", me);
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    if (code_stride < 0 || range_stride < 0 || stats_stride < 0) return fail_arg("%s: negative stride", me);
    std::vector<SqTensorDev> table;
    std::vector<int32_t> wave_tensor, big_tensor, chunk_tensor;
    int32_t n_slots = 0;
    const int64_t most = 0x7fffffff / 4;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_squant_tensor& t = tensors[i];
        if (!t.data || t.rows <= 0 || t.row_len <= 0) return fail_arg("%s: tensor %d is empty", me, i);
        if (t.num_bits < 2 || t.num_bits > 16) return fail_arg("%s: tensor %d: num_bits %d outside [2, 16]", me, i, (int)t.num_bits);
        if (t.kernel_len <= 0 || t.row_len % t.kernel_len != 0)
            return fail_arg("%s: tensor %d: row_len %lld is no multiple of kernel_len %lld", me, i, (long long)t.row_len, (long long)t.kernel_len);
        if (t.row_len > kSqMaxRow) return fail_arg("%s: tensor %d: row_len %lld above dfq_squant_max_row_len() = %d", me, i, (long long)t.row_len, kSqMaxRow);
        if (t.rows > most) return fail_arg("%s: tensor %d: too many rows", me, i);
        const int64_t numel = t.rows * t.row_len;
        if (t.code_offset < -1 || t.range_offset < -1 || t.stats_offset < -1) return fail_arg("%s: tensor %d: negative offset", me, i);
        if (t.code_offset >= 0) {
            if (!codes) return fail_arg("%s: tensor %d writes codes, but the code block is null", me, i);
            if (code_bytes != 1 && code_bytes != 4) return fail_arg("%s: code width %d bytes (1 or 4)", me, (int)code_bytes);
            if (code_bytes == 1 && t.num_bits > 8) return fail_arg("%s: tensor %d: 1-byte codes of %d bits", me, i, (int)t.num_bits);
            if (t.code_offset > code_stride - numel) return fail_arg("%s: tensor %d: codes overflow the code stride", me, i);
        }
        if (t.range_offset >= 0) {
            if (!ranges) return fail_arg("%s: tensor %d writes ranges, but the range block is null", me, i);
            if (t.range_offset > range_stride - 2 * (t.per_row ? t.rows : 1)) return fail_arg("%s: tensor %d: ranges overflow the range stride", me, i);
        }
        if (t.stats_offset >= 0) {
            if (!stats) return fail_arg("%s: tensor %d writes stats, but the stats block is null", me, i);
            if (t.stats_offset > stats_stride - 2 * t.rows) return fail_arg("%s: tensor %d: stats overflow the stats stride", me, i);
        }
        SqTensorDev d{};
        d.x = t.data; d.y = t.data;
        d.code_off = t.code_offset; d.range_off = t.range_offset; d.stats_off = t.stats_offset;
        d.rows = (int32_t)t.rows; d.len = (int32_t)t.row_len; d.klen = (int32_t)t.kernel_len;
        d.num_bits = t.num_bits; d.symmetric = t.symmetric ? 1 : 0; d.per_row = t.per_row ? 1 : 0;
        d.slot = -1;
        d.cls = sq_class(t.row_len);
        if (!t.per_row) {
            d.slot = n_slots++;
            d.chunk_begin = (int32_t)chunk_tensor.size();
            const int64_t k = (numel + kSqChunk - 1) / kSqChunk;
            if (k > most - (int64_t)chunk_tensor.size()) return fail_arg("%s: too much work for one launch", me);
            chunk_tensor.insert(chunk_tensor.end(), (size_t)k, i);
        }
        std::vector<int32_t>& items = d.cls == 7 ? big_tensor : wave_tensor;
        const int64_t per = sq_rows_per_wave(d.cls), k = (t.rows + per - 1) / per;
        if (k > most - (int64_t)items.size()) return fail_arg("%s: too much work for one launch", me);
        d.item_begin = (int32_t)items.size();
        items.insert(items.end(), (size_t)k, i);
        table.push_back(d);
    }
    const int64_t biggest = (int64_t)std::max(std::max(wave_tensor.size(), big_tensor.size()), chunk_tensor.size());
    if (biggest * n_nets > most) return fail_arg("%s: too much work for one launch", me);

    dfq_batch_squant_plan* p = new dfq_batch_squant_plan();
    SqArgs& a = p->args;
    a.codes = (unsigned char*)codes;
    a.ranges = ranges;
    a.stats = (long long*)stats;
    a.code_stride = code_stride; a.range_stride = range_stride; a.stats_stride = stats_stride;
    a.code_bytes = code_bytes;
    a.n_slots = n_slots;
    a.waves_pn = (int32_t)wave_tensor.size(); a.waves = a.waves_pn * n_nets;
    a.bigs_pn = (int32_t)big_tensor.size(); a.bigs = a.bigs_pn * n_nets;
    a.chunks_pn = (int32_t)chunk_tensor.size(); a.chunks = a.chunks_pn * n_nets;
    p->launches = (a.chunks > 0) + (a.waves > 0) + (a.bigs > 0);
    BatchUpload up{p->mem};
    a.tensors = up.put(table);
    a.wave_tensor = up.put(wave_tensor);
    a.big_tensor = up.put(big_tensor);
    a.chunk_tensor = up.put(chunk_tensor);
    a.delta = up.put(batch_delta(bases, n_nets));
    a.slots = (uint32_t*)up.raw(nullptr, sizeof(uint32_t) * 2 * (size_t)n_slots * n_nets);
    p->widths.index = (const int32_t*)up.raw(nullptr, sizeof(int32_t) * (size_t)n_tensors);      // (filled by set_widths)
    p->n_nets = n_nets;
    p->n_tensors = n_tensors;
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch squant plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_squant_plan_run(dfq_batch_squant_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_squant_plan_run: null plan");
    return sq_launch(p->args, as_stream(stream), p->widths.widths ? &p->widths : nullptr, p->n_nets);
}

int dfq_batch_squant_plan_set_widths(dfq_batch_squant_plan* p, const int32_t* widths, int64_t width_stride, const int32_t* width_index,
                                     int32_t* status) {
    const char* me = "dfq_batch_squant_plan_set_widths";
    if (!p) return fail_arg("%s: null plan", me);
    if (!widths) {
        p->widths.widths = nullptr;
        p->widths.status = nullptr;
        return DFQ_OK;
    }
    if (!width_index || !status) return fail_arg("%s: widths without width_index or status", me);
    for (int i = 0; i < p->n_tensors; ++i)
        if (width_index[i] < 0 || width_index[i] >= width_stride)
            return fail_arg("%s: tensor %d: width_index %d outside [0, %lld)", me, i, (int)width_index[i], (long long)width_stride);
    dev_quiesce();                                         // (a run in flight may still read the index of the widths before)
    DFQ_HIP_TRY(hipMemcpy((void*)p->widths.index, width_index, sizeof(int32_t) * (size_t)p->n_tensors, hipMemcpyHostToDevice));
    p->widths.widths = widths;
    p->widths.stride = width_stride;
    p->widths.status = status;
    return DFQ_OK;
}

}  // extern "C"
