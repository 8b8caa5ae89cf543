// Lazy-scale cross-layer equalisation (opt-in; SURVEY.md 7.3 item 9, 8d "alternative byte count") for gfx950.
//
// Every update of dfq.py:62-73 is a positive diagonal scaling, so after any number of sweeps
//     W_l = diag(S_out) . W0_l . diag(1 / S_in),     S_* = cumulative per-relation scales (utils/relation.py:20-24).
// The eager engines (dfq_le.hip, dfq_le_resident.hip) keep W itself up to date: 8 B per paired element and sweep.  This one
// never writes a weight inside the loop: a sweep only READS -- the per-channel ranges the scale solve needs (dfq.py:39-55)
// are taken from W0 with the cumulative factors applied on the fly,
//     r1[c] = range_i  fl(W0_1[c, i] * (1/S_in)[i]) * S_out[c]        (rows of the relation's first layer)
//     r2[c] = range_o,k fl(W0_2[o, c, k] * S_out[o]) * (1/S_in)[c]    (columns of its second layer)
// (fl(v * s) is monotone in v for s > 0, so the factor that is constant along the reduced dimension is applied to the two
// extrema only) -- 4 B per paired element and sweep, 17 instead of 31 MB for a MobileNetV2 -- and the weights, biases and BN
// proxies are materialised ONCE at the end by the batched rebuild launch of dfq_rebuild.hip (8 B per weight).
//
// Contract: the sweep count is GIVEN (the reference's own count for the network: the data-dependent exit test of
// dfq.py:105-115 needs mean |dW| of every sweep, which this formulation does not produce) and the result is within 1e-5
// (relative) of the sequentially rescaled tensors -- the float32 contract of BASELINE.json -- not bit-identical to them:
// the cumulative products round differently from the reference's sweep-by-sweep in-place products (measured <= 3e-6).
// That is why it is an opt-in next to the bit-exact default, and why bench.py prices it on its own byte count.
//
// Sweep-invariant ranges.  A pass whose element factors never change needs to run ONCE: the row pass of a chain's first layer
// (nothing rescales its input channels), the column pass of a chain's last layer, and both passes of a depthwise layer (a row
// is one channel: every factor is constant along the row and can be applied to the row's two extrema).  Their raw extrema are
// kept; every sweep the solve launch multiplies them by the current cumulative factors (two rounded multiplications in the
// order the pass would apply them).  What a sweep still READS are the layers in the interior of a chain that are not
// depthwise -- for MobileNetV2 0.74 of its 3.47 M weights, twice (5.9 MB per sweep); a ResNet-18 (independent pairs) reads
// its weights once per run.  bench.py prices the engine on exactly these bytes.
//
// Order of a sweep = the reference's Gauss-Seidel order (dfq.py:85): relations that share no layer form a level; per level
// one statistics launch (all row and column passes of its relations, every network of the batch) and one small solve launch
// (s per channel, dfq.py:58-59; S *= s, 1/S *= 1/s).  Networks of a batch may run different sweep counts.
#include <algorithm>
#include <vector>

#include "dfq_common.hpp"
#include "dfq_le_shared.hpp"

namespace dfq {

constexpr int kLzTileElems = 16384;   // elements a statistics workgroup streams (64 KB)
constexpr int kLzTrip = 8;            // 16-byte loads a lane keeps in flight
constexpr int kLzColTab = 1040;       // LDS entries of a column tile: input channels its positions span

struct LzRel {
    const float* w1;
    const float* w2;
    int32_t o1, row_len1, khkw1;         // first layer: rows (= paired channels), floats per row, taps per input channel
    int32_t o2, row_len2, i2g, khkw2;    // second layer
    int32_t go, gi;                      // paired channel of second-layer element (o, ii) = (o / go) * gi + ii
    int32_t ch_off;                      // this relation's channels in the S / 1/S / statistics arrays
    int32_t a_off, a_go, a_gi;           // relation A whose SECOND layer is w1: channel of element (o, pos) = a_off + (o / a_go) * a_gi + pos / khkw1; -1: none
    int32_t b_off;                       // relation B whose FIRST layer is w2: row factor S[b_off + o]; -1: none
    int32_t net;
    int32_t vec1, vec2;                  // 4: 16-byte vectors (row length % 4 == 0, base aligned), 1: scalars
    int32_t r1_mode, r2_mode;            // 0: the pass runs every sweep; 1: once (sweep-invariant extrema); 2: once, and the solve
                                         // also applies the per-row factor of the other relation (depthwise layer: see lz_solve_kernel)
};

enum { kLzRow = 0, kLzCol = 1, kLzDw = 2 };

struct LzTile {
    int32_t rel, kind;
    int32_t r0, nr;                      // rows [r0, r0 + nr)
    int32_t c0, nc;                      // kLzCol: row positions [c0, c0 + nc) (one group's rows per tile)
    int32_t once, pad1;                  // once: sweep-invariant, runs in sweep 0 only
};

struct LzArrays {
    float* S;                            // cumulative scale per paired channel (all relations, all networks)
    float* invS;                         // cumulative reciprocal factor (product of the 1/s the reference multiplies by, dfq.py:73)
    uint32_t* r1;                        // [channel][2] (min slot, max slot): RAW row extrema (element factors applied, the factor that is
                                         // constant along the row not yet), one producer per row: plain stores
    uint32_t* r2;                        // raw column extrema, merged over row blocks with atomicMax; the solve launch clears the per-sweep ones
    const int32_t* sweeps;               // sweeps each network runs
};

// ---- rows: one range per row (row pass of a first layer; column pass of a depthwise second layer) --------------------
// G = 2^k lanes share a row (64 / G rows per wave and trip), a lane walks the row in steps of G vectors; kLzTrip vectors
// of a lane are requested before the first one is used.  The factor of an element is either one number per ROW
// (rowfac(o): requested together with the row's data) or, with TAB, one per input channel from an LDS table the caller
// staged (tab[(pos + k) / khkw]; a 16-byte LDS read per vector for 1x1 layers).  emit(o, mn, mx) receives the row's extrema.
template <int VEC, bool TAB, class RowFac, class Emit>
__device__ __forceinline__ void lz_rows(const float* __restrict__ w, int row_len, int r0, int nr, const float* tab, int khkw,
                                        RowFac rowfac, Emit emit) {
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int nvec = (row_len + VEC - 1) / VEC;
    int lg = 0;
    while ((1 << lg) < nvec && lg < 6) ++lg;
    const int G = 1 << lg, rpw = kWave >> lg;
    const int sub = lane >> lg, ln = lane & (G - 1);
    const int npi = (nvec + G - 1) >> lg;                              // trips along a row
    const int nri = (nr + 4 * rpw - 1) / (4 * rpw);                    // row blocks of this wave
    const int total = npi * nri;
    float mn = INFINITY, mx = -INFINITY;
    int ri = 0, pi = 0;                                                // position of slot q in (row block, trip along the row)
    for (int q0 = 0; q0 < total; q0 += kLzTrip) {
        float x[kLzTrip][VEC], f[kLzTrip];
        {
            int ri2 = ri, pi2 = pi;
#pragma unroll
            for (int u = 0; u < kLzTrip; ++u) {
                if (q0 + u < total) {                                  // uniform
                    const int row = min((ri2 * 4 + wave) * rpw + sub, nr - 1);
                    const int pos = min((pi2 * G + ln) * VEC, (nvec - 1) * VEC);
                    const float* src = w + (int64_t)(r0 + row) * row_len + pos;
                    if constexpr (VEC == 4) {
                        const fvec4 v = DFQ_NT_LOAD((const fvec4*)src);
                        x[u][0] = v[0]; x[u][1] = v[1]; x[u][2] = v[2]; x[u][3] = v[3];
                    } else {
                        x[u][0] = *src;
                    }
                    f[u] = TAB ? 1.0f : rowfac(r0 + row);
                    if (++pi2 == npi) { pi2 = 0; ++ri2; }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kLzTrip; ++u) {
            if (q0 + u < total) {
                const int rowi = (ri * 4 + wave) * rpw + sub;
                const int row = min(rowi, nr - 1);
                const int pos = min((pi * G + ln) * VEC, (nvec - 1) * VEC);          // clamped duplicates are harmless for min / max
                float fk[VEC];
                if constexpr (TAB) {
                    if constexpr (VEC == 4) {
                        if (khkw == 1) {
                            const fvec4 t = *(const fvec4*)(tab + pos);
                            fk[0] = t[0]; fk[1] = t[1]; fk[2] = t[2]; fk[3] = t[3];
                        } else {
#pragma unroll
                            for (int k = 0; k < VEC; ++k) fk[k] = tab[small_div(pos + k, khkw)];
                        }
                    } else {
                        fk[0] = tab[khkw == 1 ? pos : small_div(pos, khkw)];
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) fk[k] = f[u];
                }
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float y = quiet_nan(x[u][k] * fk[k]);         // (free behind a real product; a constant factor of 1 leaves the loaded value)
                    mn = vmin_raw(mn, y); mx = vmax_raw(mx, y);
                }
                if (++pi == npi) {                                     // the row is complete: reduce over its G lanes
                    if (G > 1) xor_lane_minmax<1>(mn, mx);
                    if (G > 2) xor_lane_minmax<2>(mn, mx);
                    if (G > 4) xor_lane_minmax<4>(mn, mx);
                    if (G > 8) xor_lane_minmax<8>(mn, mx);
                    if (G > 16) xor_lane_minmax<16>(mn, mx);
                    if (G > 32) xor_lane_minmax<32>(mn, mx);
                    if (ln == 0 && rowi < nr) emit(r0 + row, mn, mx);
                    mn = INFINITY; mx = -INFINITY;
                    pi = 0; ++ri;
                }
            }
        }
    }
}

// ---- columns: one range per input channel over a block of rows of ONE group (column pass of a second layer) ------------
// A thread keeps one vector position and walks down the rows (kLzTrip loads in flight); its column extrema stay in registers,
// the row groups of the workgroup merge through LDS, the row blocks of the layer through global atomicMax -- tiles are TALL
// (up to 256 rows) and only as wide as that leaves room for: a layer publishes (rows / tile rows) x columns x 2 atomics per
// sweep, and those, not the data, set the pace of a launch made of flat tiles (17-row tiles of a 960-wide layer: 57 per word).
template <int VEC>
__device__ __forceinline__ void lz_cols(const LzRel& R, const LzTile& T, const LzArrays& a, uint32_t* sh_col) {
    const int tid = threadIdx.x;
    const int nvec = (T.nc + VEC - 1) / VEC;
    int lg = 0;
    while ((1 << lg) < nvec && lg < 8) ++lg;
    const int lanes = 1 << lg, rgs = kBlock >> lg;
    const int cl = tid & (lanes - 1), rg = tid >> lg;
    const bool col_on = cl < nvec;
    const int pos = T.c0 + min(cl, nvec - 1) * VEC;
    const int i0 = small_div(T.c0, R.khkw2);
    const int nci = small_div(T.c0 + T.nc - 1, R.khkw2) - i0 + 1;
    for (int i = tid; i < 2 * nci; i += kBlock) sh_col[i] = 0u;
    __syncthreads();
    float cmn[VEC], cmx[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { cmn[k] = INFINITY; cmx[k] = -INFINITY; }
    const float* base = R.w2 + (int64_t)T.r0 * R.row_len2 + pos;
    const float* so = (R.b_off >= 0) ? a.S + R.b_off + T.r0 : nullptr;
    for (int r = rg; r < T.nr; r += rgs * kLzTrip) {
        float x[kLzTrip][VEC], f[kLzTrip];
#pragma unroll
        for (int u = 0; u < kLzTrip; ++u) {
            const int row = min(r + u * rgs, T.nr - 1);
            const float* src = base + (int64_t)row * R.row_len2;
            if constexpr (VEC == 4) {
                const fvec4 v = DFQ_NT_LOAD((const fvec4*)src);
                x[u][0] = v[0]; x[u][1] = v[1]; x[u][2] = v[2]; x[u][3] = v[3];
            } else {
                x[u][0] = *src;
            }
            f[u] = so ? so[row] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < kLzTrip; ++u) {                            // rows past the end are clamped duplicates: harmless
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float y = quiet_nan(x[u][k] * f[u]);
                cmn[k] = vmin_raw(cmn[k], y); cmx[k] = vmax_raw(cmx[k], y);
            }
        }
    }
    // lanes of a wave that hold the same columns (ids differing in bits >= lg) merge in the register file first
#define DFQ_LZ_STEP(M) if ((M) >= lanes) { _Pragma("unroll") for (int k = 0; k < VEC; ++k) xor_lane_minmax<M>(cmn[k], cmx[k]); }
    DFQ_LZ_STEP(1) DFQ_LZ_STEP(2) DFQ_LZ_STEP(4) DFQ_LZ_STEP(8) DFQ_LZ_STEP(16) DFQ_LZ_STEP(32)
#undef DFQ_LZ_STEP
    const bool wave_first = lanes >= kWave || (tid % kWave) < lanes;  // one lane per column position and wave
    if (col_on && wave_first) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (pos + k < T.c0 + T.nc) {
                const int ii = small_div(pos + k, R.khkw2) - i0;
                atomicMax(sh_col + 2 * ii, ~enc_ord(cmn[k]));
                atomicMax(sh_col + 2 * ii + 1, enc_ord(cmx[k]));
            }
        }
    }
    __syncthreads();
    const int g = small_div(T.r0, R.go);
    for (int i = tid; i < nci; i += kBlock) {
        if (sh_col[2 * i + 1] == 0u) continue;
        const int ch = R.ch_off + g * R.gi + i0 + i;
        atomicMax(a.r2 + 2 * (int64_t)ch, sh_col[2 * i]);
        atomicMax(a.r2 + 2 * (int64_t)ch + 1, sh_col[2 * i + 1]);
    }
}

__global__ __launch_bounds__(kBlock) void lz_stats_kernel(const LzRel* __restrict__ rels, const LzTile* __restrict__ tiles, LzArrays a,
                                                          int sweep) {
    __shared__ __attribute__((aligned(16))) uint32_t sh_col[2 * kLzColTab];
    const LzTile T = tiles[blockIdx.x];
    const LzRel R = rels[T.rel];
    if (sweep >= a.sweeps[R.net]) return;                              // this network has run its sweeps
    if (T.kind == kLzRow) {
        // raw r1[c] = range_i fl(w0[c, i] * (1/S_A)[channel of i]); the solve launch multiplies by S[c]
        auto emit = [&](int o, float mn, float mx) {
            uint32_t* dst = a.r1 + 2 * (int64_t)(R.ch_off + o);
            dst[0] = ~enc_ord(mn);
            dst[1] = enc_ord(mx);
        };
        auto none = [](int) -> float { return 1.0f; };
        if (R.r1_mode == 0) {
            // 1/S_A of the input channels of the tile's group, staged in LDS once (the tile's rows share one group of A)
            float* tab = (float*)sh_col;
            const int n_in = small_div(R.row_len1, R.khkw1);
            const float* src = a.invS + R.a_off + small_div(T.r0, R.a_go) * R.a_gi;
            for (int i = threadIdx.x; i < n_in; i += kBlock) tab[i] = src[i];
            __syncthreads();
            if (R.vec1 == 4) lz_rows<4, true>(R.w1, R.row_len1, T.r0, T.nr, tab, R.khkw1, none, emit);
            else lz_rows<1, true>(R.w1, R.row_len1, T.r0, T.nr, tab, R.khkw1, none, emit);
        } else {                                                       // sweep-invariant: the extrema of the pristine rows
            if (R.vec1 == 4) lz_rows<4, false>(R.w1, R.row_len1, T.r0, T.nr, nullptr, 1, none, emit);
            else lz_rows<1, false>(R.w1, R.row_len1, T.r0, T.nr, nullptr, 1, none, emit);
        }
    } else if (T.kind == kLzDw) {
        // depthwise second layer (one input channel per row): raw r2[c] = range over the rows of channel c of fl(w0 * S_B[o]);
        // with one row per channel (r2_mode 2) the row factor moves to the solve launch and the pass runs once
        const float* sb = (R.b_off >= 0 && R.r2_mode == 0) ? a.S + R.b_off : nullptr;
        auto rowfac = [&](int o) -> float { return sb ? sb[o] : 1.0f; };
        auto emit = [&](int o, float mn, float mx) {
            const int ch = R.ch_off + small_div(o, R.go) * R.gi;
            atomicMax(a.r2 + 2 * (int64_t)ch, ~enc_ord(mn));
            atomicMax(a.r2 + 2 * (int64_t)ch + 1, enc_ord(mx));
        };
        if (R.vec2 == 4) lz_rows<4, false>(R.w2, R.row_len2, T.r0, T.nr, nullptr, 1, rowfac, emit);
        else lz_rows<1, false>(R.w2, R.row_len2, T.r0, T.nr, nullptr, 1, rowfac, emit);
    } else {
        if (R.vec2 == 4) lz_cols<4>(R, T, a, sh_col);
        else lz_cols<1>(R, T, a, sh_col);
    }
}

// dfq.py:58-59 per paired channel of the level's relations; S *= s, 1/S *= (1/s as the reference multiplies it, dfq.py:73)
__global__ __launch_bounds__(kBlock) void lz_solve_kernel(const LzRel* __restrict__ rels, const int32_t* __restrict__ lvl_rel,
                                                          const int32_t* __restrict__ lvl_begin, int n_lvl_rels, LzArrays a,
                                                          LeParams p, int sweep) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= lvl_begin[n_lvl_rels]) return;
    int lo = 0, hi = n_lvl_rels - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (lvl_begin[mid] <= j) lo = mid; else hi = mid - 1;
    }
    const LzRel R = rels[lvl_rel[lo]];
    if (sweep >= a.sweeps[R.net]) return;
    const int64_t ch = R.ch_off + (j - lvl_begin[lo]);
    const int c = j - lvl_begin[lo];
    const uint32_t a0 = a.r1[2 * ch], a1 = a.r1[2 * ch + 1], b0 = a.r2[2 * ch], b1 = a.r2[2 * ch + 1];
    const float s_old = a.S[ch], inv_old = a.invS[ch];
    // the raw extrema times the factors that are constant along the reduced dimension, in the order a pass over the
    // current weights would apply them: rows fl(fl(w0 * 1/S_A) * S), columns fl(fl(w0 * S_B) * 1/S)
    float mn1 = slot_min(a0), mx1 = slot_max(a1), mn2 = slot_min(b0), mx2 = slot_max(b1);
    if (R.r1_mode == 2) {                  // first layer depthwise: its single input channel's 1/S_A was not in the raw extrema
        const float fa = a.invS[R.a_off + small_div(c, R.a_go) * R.a_gi];
        mn1 = mn1 * fa; mx1 = mx1 * fa;
    }
    mn1 = mn1 * s_old; mx1 = mx1 * s_old;
    if (R.r2_mode == 2) {                  // second layer depthwise (one row per channel): S_B of that row
        const float fb = a.S[R.b_off + c];
        mn2 = mn2 * fb; mx2 = mx2 * fb;
    }
    mn2 = mn2 * inv_old; mx2 = mx2 * inv_old;
    float s, inv;
    le_solve(range_of(mn1, mx1, p.signed_range), range_of(mn2, mx2, p.signed_range), p, s, inv);
    a.S[ch] = s_old * s;
    a.invS[ch] = inv_old * inv;
    if (R.r2_mode == 0) {                  // the next sweep's column passes merge into a clean slot
        a.r2[2 * ch] = 0u;
        a.r2[2 * ch + 1] = 0u;
    }
}

__global__ void lz_fill_kernel(float* x, int64_t n, float v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = v;
}

}  // namespace dfq

using namespace dfq;

struct dfq_le_lazy_plan {
    int n_rels = 0, n_nets = 0, n_levels = 0;
    int64_t channels = 0, paired_elements = 0, weight_elements = 0, sweep_elements = 0;
    LzRel* d_rels = nullptr;
    LzTile* d_tiles = nullptr;
    int32_t* d_lvl_rel = nullptr;
    int32_t* d_lvl_begin = nullptr;
    int32_t* d_sweeps = nullptr;
    float* d_S = nullptr;            // [2 * channels]: S then 1/S
    uint32_t* d_stats = nullptr;     // [4 * channels]: r1 then r2
    struct Level { int tile_begin, n_tiles, n_every, rel_begin, n_rels, ch_total; };   // tiles [0, n_every) run every sweep, the rest once
    std::vector<Level> levels;
    std::vector<int> lvl_begin_off;  // offset of each level's prefix array inside d_lvl_begin
    std::vector<int32_t> h_sweeps;   // staging copy of the caller's sweep counts (outlives the asynchronous upload)
    dfq_rebuild_plan* rebuild = nullptr;
};

extern "C" {

void dfq_le_lazy_plan_destroy(dfq_le_lazy_plan* p) {
    if (!p) return;
    dfq::dev_quiesce();                                  // nothing in flight may still use the blocks released below
    if (p->d_rels) dfq::dev_free(p->d_rels);
    if (p->d_tiles) dfq::dev_free(p->d_tiles);
    if (p->d_lvl_rel) dfq::dev_free(p->d_lvl_rel);
    if (p->d_lvl_begin) dfq::dev_free(p->d_lvl_begin);
    if (p->d_sweeps) dfq::dev_free(p->d_sweeps);
    if (p->d_S) dfq::dev_free(p->d_S);
    if (p->d_stats) dfq::dev_free(p->d_stats);
    if (p->rebuild) dfq_rebuild_plan_destroy(p->rebuild);
    delete p;
}

int dfq_le_lazy_plan_create(const dfq_layer* layers, int32_t n_layers, const int32_t* layer_net, int32_t n_nets,
                            const dfq_relation* relations, int32_t n_relations, dfq_le_lazy_plan** out_plan) {
    if (!layers || n_layers <= 0 || !relations || n_relations <= 0 || n_nets <= 0 || !out_plan)
        return fail_arg("dfq_le_lazy_plan_create: bad argument");
    auto net_of = [&](int l) { return layer_net ? layer_net[l] : 0; };
    std::vector<int> as_first(n_layers, -1), as_second(n_layers, -1);
    for (int r = 0; r < n_relations; ++r) {
        const dfq_relation& rr = relations[r];
        if (rr.first < 0 || rr.first >= n_layers || rr.second < 0 || rr.second >= n_layers || rr.first == rr.second)
            return fail_arg("dfq_le_lazy_plan_create: relation %d: bad layer indices", r);
        if (!rr.scale_cum) return fail_arg("dfq_le_lazy_plan_create: relation %d: scale_cum is required", r);
        if (net_of(rr.first) != net_of(rr.second)) return fail_arg("dfq_le_lazy_plan_create: relation %d pairs layers of two networks", r);
        if (as_first[rr.first] >= 0) return fail_arg("dfq_le_lazy_plan_create: layer %d is first in one relation only", rr.first);
        if (as_second[rr.second] >= 0) return fail_arg("dfq_le_lazy_plan_create: layer %d is second in one relation only", rr.second);
        as_first[rr.first] = r; as_second[rr.second] = r;
        const dfq_layer& A = layers[rr.first];
        const dfq_layer& B = layers[rr.second];
        if (!A.weight || !B.weight || A.out_ch <= 0 || B.out_ch <= 0 || A.in_per_group <= 0 || B.in_per_group <= 0 || A.khkw <= 0 || B.khkw <= 0)
            return fail_arg("dfq_le_lazy_plan_create: relation %d: bad layer", r);
        const int G = (A.out_ch != B.in_per_group) ? (A.out_ch / B.in_per_group) : 1;
        if (G < 1 || G * B.in_per_group != A.out_ch || B.out_ch % G != 0)
            return fail_arg("dfq_le_lazy_plan_create: relation %d: unsupported pairing O1=%d I2/g=%d O2=%d", r, A.out_ch, B.in_per_group, B.out_ch);
        if ((int64_t)A.in_per_group * A.khkw >= (1 << 20) || (int64_t)B.in_per_group * B.khkw >= (1 << 20) || A.out_ch >= (1 << 20) || B.out_ch >= (1 << 20))
            return fail_arg("dfq_le_lazy_plan_create: relation %d: layer dimensions must be below 2^20", r);
    }
    // the list order must rescale a shared layer as a second layer before it is rescaled as a first layer (like the eager plan)
    for (int l = 0; l < n_layers; ++l)
        if (as_first[l] >= 0 && as_second[l] >= 0 && as_second[l] > as_first[l])
            return fail_arg("dfq_le_lazy_plan_create: layer %d: unsupported relation order", l);
    dfq_le_lazy_plan* p = new dfq_le_lazy_plan();
    p->n_rels = n_relations; p->n_nets = n_nets;
    // levels: relations sharing a layer keep their list order
    std::vector<int> level(n_relations, 0), last_level(n_layers, -1);
    int n_levels = 0;
    for (int r = 0; r < n_relations; ++r) {
        const int lv = std::max(last_level[relations[r].first], last_level[relations[r].second]) + 1;
        level[r] = lv; last_level[relations[r].first] = lv; last_level[relations[r].second] = lv;
        n_levels = std::max(n_levels, lv + 1);
    }
    p->n_levels = n_levels;
    std::vector<LzRel> h(n_relations);
    int64_t ch = 0;
    for (int r = 0; r < n_relations; ++r) { h[r].ch_off = (int32_t)ch; ch += (layers[relations[r].first].out_ch + 3) & ~3; }
    p->channels = ch;
    for (int r = 0; r < n_relations; ++r) {
        const dfq_relation& rr = relations[r];
        const dfq_layer& A = layers[rr.first];
        const dfq_layer& B = layers[rr.second];
        LzRel& d = h[r];
        d.w1 = A.weight; d.w2 = B.weight;
        d.o1 = A.out_ch; d.row_len1 = A.in_per_group * A.khkw; d.khkw1 = A.khkw;
        d.o2 = B.out_ch; d.i2g = B.in_per_group; d.khkw2 = B.khkw; d.row_len2 = B.in_per_group * B.khkw;
        const int G = (d.o1 != d.i2g) ? (d.o1 / d.i2g) : 1;
        d.gi = d.o1 / G; d.go = d.o2 / G;
        const int ra = as_second[rr.first], rb = as_first[rr.second];
        d.a_off = ra >= 0 ? h[ra].ch_off : -1;
        d.a_go = ra >= 0 ? h[ra].go : 1; d.a_gi = ra >= 0 ? h[ra].gi : 0;
        d.b_off = rb >= 0 ? h[rb].ch_off : -1;
        d.net = net_of(rr.first);
        // sweep-invariant passes (see the header): rows of a chain start or of a depthwise first layer; columns of a chain end or
        // of a depthwise second layer with one row per channel
        d.r1_mode = (d.a_off < 0) ? 1 : (d.row_len1 == d.khkw1 ? 2 : 0);
        d.r2_mode = (d.b_off < 0) ? 1 : ((d.i2g == 1 && d.go == 1) ? 2 : 0);
        d.vec1 = (d.row_len1 % 4 == 0 && ((uintptr_t)A.weight & 15u) == 0) ? 4 : 1;
        d.vec2 = (d.row_len2 % 4 == 0 && ((uintptr_t)B.weight & 15u) == 0) ? 4 : 1;
        p->paired_elements += (int64_t)d.o1 * d.row_len1 + (int64_t)d.o2 * d.row_len2;
    }
    // geometry of A was filled in list order: a relation's A precedes it (checked above), except through ch_off which is complete
    for (int r = 0; r < n_relations; ++r) {
        const int ra = as_second[relations[r].first];
        if (ra >= 0) { h[r].a_go = h[ra].go; h[r].a_gi = h[ra].gi; }
    }
    // tiles, level after level
    std::vector<LzTile> tiles;
    std::vector<int32_t> lvl_rel, lvl_begin;
    for (int lv = 0; lv < n_levels; ++lv) {
        dfq_le_lazy_plan::Level L;
        L.tile_begin = (int)tiles.size(); L.rel_begin = (int)lvl_rel.size();
        p->lvl_begin_off.push_back((int)lvl_begin.size());
        int chs = 0;
        for (int r = 0; r < n_relations; ++r) {
            if (level[r] != lv) continue;
            const LzRel& d = h[r];
            lvl_rel.push_back(r);
            lvl_begin.push_back(chs);
            chs += d.o1;
            // row pass over the first layer: complete rows; with a column-factor table (A present, several input channels per
            // row) the rows of a tile stay inside one group of A
            {
                int tr = std::max(1, kLzTileElems / std::max(1, d.row_len1));
                tr = std::min(tr, d.o1);
                const bool table = d.r1_mode == 0;
                const int span = table ? std::min(d.a_go, d.o1) : d.o1;
                if (table && d.row_len1 / d.khkw1 > 2 * kLzColTab)
                    return (dfq_le_lazy_plan_destroy(p), fail_arg("dfq_le_lazy_plan_create: relation %d: %d input channels per row > %d", r, d.row_len1 / d.khkw1, 2 * kLzColTab));
                for (int g0 = 0; g0 < d.o1; g0 += span)
                    for (int r0 = g0; r0 < std::min(g0 + span, d.o1); r0 += tr)
                        tiles.push_back(LzTile{r, kLzRow, r0, std::min(tr, std::min(g0 + span, d.o1) - r0), 0, d.row_len1, d.r1_mode != 0, 0});
            }
            if (d.i2g == 1) {            // depthwise second layer: row style
                int tr = std::max(1, kLzTileElems / std::max(1, d.row_len2));
                tr = std::min(tr, d.o2);
                for (int r0 = 0; r0 < d.o2; r0 += tr) tiles.push_back(LzTile{r, kLzDw, r0, std::min(tr, d.o2 - r0), 0, d.row_len2, d.r2_mode != 0, 0});
            } else {
                // tall tiles: up to 256 rows, as wide as kLzTileElems allows (>= 16 vector positions, <= one per thread)
                const int groups = d.o2 / d.go;
                const int tr_want = std::min(d.go, 256);
                int tc_max = d.vec2 * 16;
                while (tc_max < kBlock * d.vec2 && tc_max * 2 * tr_want <= kLzTileElems) tc_max *= 2;
                for (int c0 = 0; c0 < d.row_len2; c0 += tc_max) {
                    const int nc = std::min(tc_max, d.row_len2 - c0);
                    int tr = std::max(1, kLzTileElems / nc);
                    tr = std::min(tr, d.go);
                    for (int g = 0; g < groups; ++g)
                        for (int r0 = 0; r0 < d.go; r0 += tr)
                            tiles.push_back(LzTile{r, kLzCol, g * d.go + r0, std::min(tr, d.go - r0), c0, nc, d.r2_mode != 0, 0});
                }
            }
        }
        lvl_begin.push_back(chs);
        // the tiles that run every sweep first, the sweep-invariant ones behind them (sweep 0 launches both)
        std::stable_partition(tiles.begin() + L.tile_begin, tiles.end(), [](const LzTile& t) { return t.once == 0; });
        L.n_tiles = (int)tiles.size() - L.tile_begin; L.n_rels = (int)lvl_rel.size() - L.rel_begin; L.ch_total = chs;
        L.n_every = 0;
        for (int t = L.tile_begin; t < (int)tiles.size(); ++t) {
            if (tiles[t].once) continue;
            L.n_every += 1;
            p->sweep_elements += (int64_t)tiles[t].nr * tiles[t].nc;
        }
        p->levels.push_back(L);
    }
    // materialisation: every paired tensor once, from the final factors
    std::vector<dfq_rebuild_item> items;
    hipError_t e;
    auto fail_alloc = [&](hipError_t err) { dfq_le_lazy_plan_destroy(p); return fail_hip(err, "lazy le plan allocation", __FILE__, __LINE__); };
    if ((e = dfq::dev_malloc((void**)&p->d_S, sizeof(float) * 2 * (size_t)ch)) != hipSuccess) return fail_alloc(e);
    if ((e = dfq::dev_malloc((void**)&p->d_stats, sizeof(uint32_t) * 4 * (size_t)ch)) != hipSuccess) return fail_alloc(e);
    float* dS = p->d_S;
    float* dInv = p->d_S + ch;
    for (int l = 0; l < n_layers; ++l) {
        const int rb = as_first[l], ra = as_second[l];
        if (rb < 0 && ra < 0) continue;
        const dfq_layer& L = layers[l];
        dfq_rebuild_item it;
        it.src = L.weight; it.dst = L.weight;
        it.s_out = rb >= 0 ? dS + h[rb].ch_off : nullptr;
        it.s_in = ra >= 0 ? dInv + h[ra].ch_off : nullptr;
        it.rows = L.out_ch; it.cols = L.in_per_group; it.khkw = L.khkw;
        it.groups = ra >= 0 ? L.out_ch / h[ra].go : 1;
        it.in_reciprocal = 1; it.reserved = 0;
        items.push_back(it);
        p->weight_elements += (int64_t)L.out_ch * L.in_per_group * L.khkw;
        if (rb >= 0) {
            const dfq_relation& rr = relations[rb];
            float* vecs[4] = {L.bias, rr.bn_weight, rr.bn_bias, rr.scale_cum};
            for (float* v : vecs) {
                if (!v) continue;
                dfq_rebuild_item vi;
                vi.src = v; vi.dst = v; vi.s_out = dS + h[rb].ch_off; vi.s_in = nullptr;
                vi.rows = L.out_ch; vi.cols = 1; vi.khkw = 1; vi.groups = 1; vi.in_reciprocal = 0; vi.reserved = 0;
                items.push_back(vi);
            }
        }
    }
    int rc = dfq_rebuild_plan_create(items.data(), (int32_t)items.size(), &p->rebuild);
    if (rc) { dfq_le_lazy_plan_destroy(p); return rc; }
    if ((e = dfq::dev_malloc((void**)&p->d_rels, sizeof(LzRel) * n_relations)) != hipSuccess) return fail_alloc(e);
    if ((e = dfq::dev_malloc((void**)&p->d_tiles, sizeof(LzTile) * std::max<size_t>(1, tiles.size()))) != hipSuccess) return fail_alloc(e);
    if ((e = dfq::dev_malloc((void**)&p->d_lvl_rel, sizeof(int32_t) * std::max<size_t>(1, lvl_rel.size()))) != hipSuccess) return fail_alloc(e);
    if ((e = dfq::dev_malloc((void**)&p->d_lvl_begin, sizeof(int32_t) * std::max<size_t>(1, lvl_begin.size()))) != hipSuccess) return fail_alloc(e);
    if ((e = dfq::dev_malloc((void**)&p->d_sweeps, sizeof(int32_t) * n_nets)) != hipSuccess) return fail_alloc(e);
    if ((e = hipMemcpy(p->d_rels, h.data(), sizeof(LzRel) * n_relations, hipMemcpyHostToDevice)) != hipSuccess) return fail_alloc(e);
    if ((e = hipMemcpy(p->d_tiles, tiles.data(), sizeof(LzTile) * tiles.size(), hipMemcpyHostToDevice)) != hipSuccess) return fail_alloc(e);
    if ((e = hipMemcpy(p->d_lvl_rel, lvl_rel.data(), sizeof(int32_t) * lvl_rel.size(), hipMemcpyHostToDevice)) != hipSuccess) return fail_alloc(e);
    if ((e = hipMemcpy(p->d_lvl_begin, lvl_begin.data(), sizeof(int32_t) * lvl_begin.size(), hipMemcpyHostToDevice)) != hipSuccess) return fail_alloc(e);
    if ((e = hipDeviceSynchronize()) != hipSuccess) return fail_alloc(e);
    *out_plan = p;
    return DFQ_OK;
}

int32_t dfq_le_lazy_plan_levels(const dfq_le_lazy_plan* p) { return p ? p->n_levels : 0; }
int64_t dfq_le_lazy_plan_paired_elements(const dfq_le_lazy_plan* p) { return p ? p->paired_elements : 0; }
int64_t dfq_le_lazy_plan_weight_elements(const dfq_le_lazy_plan* p) { return p ? p->weight_elements : 0; }
int64_t dfq_le_lazy_plan_sweep_elements(const dfq_le_lazy_plan* p) { return p ? p->sweep_elements : 0; }

int dfq_le_lazy_run(dfq_le_lazy_plan* p, const dfq_le_config* cfg, const int32_t* sweeps_per_net, void* stream) {
    if (!p || !cfg || !sweeps_per_net) return fail_arg("dfq_le_lazy_run: bad argument");
    hipStream_t st = as_stream(stream);
    int max_sweeps = 0;
    for (int n = 0; n < p->n_nets; ++n) {
        if (sweeps_per_net[n] < 0) return fail_arg("dfq_le_lazy_run: network %d: the sweep count must be given (>= 0)", n);
        max_sweeps = std::max(max_sweeps, sweeps_per_net[n]);
    }
    p->h_sweeps.assign(sweeps_per_net, sweeps_per_net + p->n_nets);
    DFQ_HIP_TRY(hipMemcpyAsync(p->d_sweeps, p->h_sweeps.data(), sizeof(int32_t) * p->n_nets, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lz_fill_kernel, dim3(std::min<int64_t>(1024, (2 * p->channels + 255) / 256)), dim3(256), 0, st, p->d_S, 2 * p->channels, 1.0f);
    DFQ_CHECK_LAUNCH();
    DFQ_HIP_TRY(hipMemsetAsync(p->d_stats, 0, sizeof(uint32_t) * 4 * (size_t)p->channels, st));
    LzArrays a;
    a.S = p->d_S; a.invS = p->d_S + p->channels; a.r1 = p->d_stats; a.r2 = p->d_stats + 2 * p->channels; a.sweeps = p->d_sweeps;
    const LeParams q = make_params(cfg);
    for (int k = 0; k < max_sweeps; ++k) {
        for (size_t lv = 0; lv < p->levels.size(); ++lv) {
            const auto& L = p->levels[lv];
            const int n_launch = (k == 0) ? L.n_tiles : L.n_every;
            if (n_launch > 0) {
                hipLaunchKernelGGL(lz_stats_kernel, dim3(n_launch), dim3(kBlock), 0, st, (const LzRel*)p->d_rels,
                                   (const LzTile*)(p->d_tiles + L.tile_begin), a, k);
                DFQ_CHECK_LAUNCH();
            }
            if (L.ch_total > 0) {
                hipLaunchKernelGGL(lz_solve_kernel, dim3((L.ch_total + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const LzRel*)p->d_rels,
                                   (const int32_t*)(p->d_lvl_rel + L.rel_begin), (const int32_t*)(p->d_lvl_begin + p->lvl_begin_off[lv]),
                                   L.n_rels, a, q, k);
                DFQ_CHECK_LAUNCH();
            }
        }
    }
    return dfq_rebuild_plan_run(p->rebuild, stream);
}

}  // extern "C"
