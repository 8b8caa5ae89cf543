// Clipped activation ranges from distilled data: the histogram of a quantiser's input, and the percentile / MSE-optimal range
// read off it.  The two rules of the reference (the analytic range and the running mean of per-sample extrema,
// utils/quantize.py:103-107) are min / max rules; with data in hand a calibrator can trade clipping error against rounding
// error, which is what matters below 8 bits and on the heavy-tailed inputs of add / cat nodes.
//
// 1. ah_piece_kernel (dfq_act_hist_accumulate): x is cut into flat pieces, one workgroup each, as cs_piece_kernel /
//    bt_stream_kernel cut theirs; a lane issues kHistInFlight 16-byte loads back to back (a round: 4096 floats), one round ahead
//    of the counting.  The workgroup keeps a uint32 histogram of bins + 3 slots in LDS (4096 bins: 16 KB) and flushes it ONCE,
//    with 64-bit integer atomics onto `counts`, and only the slots it touched.  A piece is 1 ... 32 rounds, as many as leave
//    about 1024 workgroups: every workgroup adds up to 8 B per touched slot to the SAME bins + 3 words, and that flush is what a
//    large tensor pays for (measured on [64, 96, 112, 112], 2048 bins: pieces of 4 / 8 / 16 rounds 126 / 90 / 77 us, about
//    14 ns per workgroup), while a small tensor wants many short pieces (a round is ~2.5 us of latency for a workgroup on its
//    own: [64, 1000] in pieces of 4 / 8 / 16 rounds 14 / 23 / 41 us).  Counts are integers: the result depends neither on the
//    order of the additions nor on the piece size, no floating-point atomic anywhere.
//    In front of the LDS every lane keeps ONE candidate bin with a private count: an element of the candidate's bin costs a
//    register increment, any other element goes to the LDS at once.  Per 16-byte vector the candidate's vote moves by +2 for
//    a hit and -1 for a miss (capped); below zero the candidate is flushed and a bin of that vector takes its place.  A
//    post-ReLU activation is half exact zeros: without this half of all LDS atomics of a wave hit one address and serialise;
//    with it the zero bin becomes the candidate after a few vectors and stays (any bin that holds more than a third of the
//    data does).  No cross-lane traffic.
// 2. ah_select_kernel (dfq_hist_clip_range): one workgroup per histogram.  Percentile: the prefix and suffix sums, a segment
//    of consecutive bins per thread.  MSE: a thread takes whole candidates (k = t, t + 256, ...) and sums a candidate's error
//    over the bins IN BIN ORDER in float64 (every lane reads the same LDS word: a broadcast), so the error of a candidate
//    does not depend on the launch; the smallest k wins a tie.
#include "dfq_common.hpp"

namespace dfq {

constexpr int kHistMaxBins = 4096;
constexpr int kHistInFlight = 4;                                   // 16-byte loads a lane issues before it uses the first
constexpr int kHistRound = kBlock * 4 * kHistInFlight;             // floats a workgroup reads per round: 4096
constexpr int kHistGroups = 1024;                                  // workgroups aimed at: a piece is as many rounds as that takes,
constexpr int kHistMaxRounds = 32;                                 // ... from 1 (4096 floats) to 32 (131072 floats)
constexpr int kVoteCap = 16;

struct AhRule {
    float lo, hi, inv, fbins;
    int bins;
    bool degenerate;
};

// include/dfq_hip.h: the slot of one element, in float32 with no contraction
__device__ __forceinline__ int ah_slot(float x, const AhRule& r) {
    if (x != x) return r.bins + 2;
    if (r.degenerate) return x < r.lo ? r.bins : (x > r.hi ? r.bins + 1 : 0);
    const float d = x - r.lo;
    const float t = d * r.inv;
    if (t < 0.0f) return r.bins;
    if (t >= r.fbins) return x <= r.hi ? r.bins - 1 : r.bins + 1;
    return t > 0.0f ? (int)t : 0;                            // (t is NaN only for inv = +inf and x == lo: bin 0)
}

struct AhLane {
    int cand, vote;
    uint32_t held;
};

// the four elements of one 16-byte vector: hits of the lane's candidate are counted in a register, every other element goes to
// the LDS at once; the vote moves by +2 per hit and -1 per miss, and below zero the candidate is flushed and a bin of this vector
// takes its place (its elements are in the LDS already).  Branch-free up to the predicated atomics: the kernel is bound by
// vector instructions per element, not by the read, as soon as this costs a branch per element
__device__ __forceinline__ void ah_count4(uint32_t* hist, AhLane& s, int s0, int s1, int s2, int s3) {
    const bool h0 = s0 == s.cand, h1 = s1 == s.cand, h2 = s2 == s.cand, h3 = s3 == s.cand;
    const int hits = (int)h0 + (int)h1 + (int)h2 + (int)h3;
    s.held += (uint32_t)hits;
    if (!h0) atomicAdd(&hist[s0], 1u);
    if (!h1) atomicAdd(&hist[s1], 1u);
    if (!h2) atomicAdd(&hist[s2], 1u);
    if (!h3) atomicAdd(&hist[s3], 1u);
    s.vote += 3 * hits - 4;
    s.vote = s.vote > kVoteCap ? kVoteCap : s.vote;
    if (s.vote < 0) {
        if (s.held) atomicAdd(&hist[s.cand], s.held);
        s.cand = h3 ? s2 : s3;
        s.held = 0;
        s.vote = 0;
    }
}

__global__ __launch_bounds__(kBlock) void ah_piece_kernel(const float* x_, int64_t n, const float* range2, int bins, int rounds,
                                                          unsigned long long* counts) {
    __shared__ uint32_t hist[kHistMaxBins + 3];
    const int t = threadIdx.x;
    const int slots = bins + 3;
    for (int i = t; i < slots; i += kBlock) hist[i] = 0u;
    AhRule r;
    r.lo = range2[0];
    r.hi = range2[1];
    r.bins = bins;
    r.fbins = (float)bins;
    const float w = r.hi - r.lo;
    r.degenerate = !(w > 0.0f && w < INFINITY);
    r.inv = r.fbins / w;
    const int piece = rounds * kHistRound;
    const int64_t start = (int64_t)blockIdx.x * piece;
    const int count = (int)(n - start < piece ? n - start : piece);
    const int nv = count >> 2;
    const gfloat* x = (const gfloat*)x_ + start;
    __syncthreads();

    AhLane s;
    s.cand = -1;
    s.vote = 0;
    s.held = 0u;
    // the loads of a round back to back, a lane past the piece's end reading the last vector again (cs_piece_kernel); the loads
    // of round r + 1 are issued before round r is counted, so a workgroup on its own does not wait a memory latency per round
    fvec4 cur[kHistInFlight], nxt[kHistInFlight];
    if (nv > 0) {
#pragma unroll
        for (int j = 0; j < kHistInFlight; ++j) {
            const int v = j * kBlock + t;
            cur[j] = *(const gfvec4*)(x + 4 * (v < nv ? v : nv - 1));
        }
    }
#pragma unroll 1
    for (int round = 0; round < rounds; ++round) {
        const int v0 = round * (kBlock * kHistInFlight);
        if (v0 >= nv) break;                                 // (workgroup-uniform, as `more` is)
        const int v1 = v0 + kBlock * kHistInFlight;
        const bool more = round + 1 < rounds && v1 < nv;
        if (more) {
#pragma unroll
            for (int j = 0; j < kHistInFlight; ++j) {
                const int v = v1 + j * kBlock + t;
                nxt[j] = *(const gfvec4*)(x + 4 * (v < nv ? v : nv - 1));
            }
        }
#pragma unroll
        for (int j = 0; j < kHistInFlight; ++j) {
            if (v0 + j * kBlock + t < nv) {
                ah_count4(hist, s, ah_slot(cur[j][0], r), ah_slot(cur[j][1], r), ah_slot(cur[j][2], r), ah_slot(cur[j][3], r));
            }
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < kHistInFlight; ++j) cur[j] = nxt[j];
        }
    }
    const int tail = (nv << 2) + t;                          // x may end in up to three single floats
    if (tail < count) atomicAdd(&hist[ah_slot(x[tail], r)], 1u);
    if (s.held) atomicAdd(&hist[s.cand], s.held);
    __syncthreads();
    for (int i = t; i < slots; i += kBlock) {
        const uint32_t c = hist[i];
        if (c) atomicAdd(&counts[i], (unsigned long long)c);
    }
}

// ---- the range from the histogram ------------------------------------------------------------------------------------------
struct AsArgs {
    const unsigned long long* counts;     // [n_hist][bins + 3]
    const float* range2;                  // [n_hist][2]
    const int32_t* num_bits;              // [n_hist]
    float* out2;                          // [n_hist][2]
    double param;
    int bins, method, candidates;
};

__device__ __forceinline__ float ah_edge(double lo, double hi, int b, int bins) {
    if (b <= 0) return (float)lo;
    if (b >= bins) return (float)hi;
    return (float)(lo + (double)b * (hi - lo) / (double)bins);
}

__device__ __forceinline__ float ah_rep(double lo, double hi, int b, int bins) {
    if (b <= 0) return (float)lo;
    if (b >= bins - 1) return (float)hi;
    return (float)(lo + ((double)b + 0.5) * (hi - lo) / (double)bins);
}

// sum_b n_b (fq(rep(b); l, h, bits) - rep(b))^2 in bin order: dfq_fake_quant's asymmetric float64-scale recipe
__device__ __forceinline__ double ah_err(const unsigned long long* nb, const float* rep, int bins, float l, float h, int bits) {
    const QParams p = qparams_double((double)l, (double)h, bits, 0);
    double e = 0.0;
    for (int b = 0; b < bins; ++b) {
        float code;
        const float v = rep[b];
        const double d = (double)fake_quant_one(v, p, &code) - (double)v;
        e += __longlong_as_double((long long)nb[b]) * (d * d);       // (the counts were converted in place, once)
    }
    return e;
}

// the candidate of least error over k < C, the smallest k on a tie; every thread returns it.  UPPER: (lo, edge(bins - k)),
// else (edge(k), h_fixed)
template <bool UPPER>
__device__ __forceinline__ int ah_search(const unsigned long long* nb, const float* rep, double lo, double hi, int bins, int C, int bits,
                                         float fixed, double* best_err, int* best_k) {
    const int t = threadIdx.x;
    double e_min = INFINITY;
    int k_min = 0x7fffffff;
    for (int k = t; k < C; k += kBlock) {
        const float l = UPPER ? fixed : ah_edge(lo, hi, k, bins);
        const float h = UPPER ? ah_edge(lo, hi, bins - k, bins) : fixed;
        const double e = ah_err(nb, rep, bins, l, h, bits);
        if (e < e_min || k_min == 0x7fffffff) { e_min = e; k_min = k; }      // (rising k: a later equal error does not replace)
    }
    __syncthreads();                                         // (best_* may still be read from the search before)
    best_err[t] = e_min;
    best_k[t] = k_min;
    __syncthreads();
    double e = best_err[0];
    int k = best_k[0];                                       // (thread 0 always has a candidate: C >= 1)
    for (int i = 1; i < kBlock; ++i) {
        const int ki = best_k[i];
        if (ki == 0x7fffffff) continue;
        const double ei = best_err[i];
        if (ei < e || (ei == e && ki < k)) { e = ei; k = ki; }
    }
    return k;
}

__global__ __launch_bounds__(kBlock) void ah_select_kernel(AsArgs a) {
    __shared__ unsigned long long nb[kHistMaxBins];
    __shared__ float rep[kHistMaxBins];
    __shared__ unsigned long long seg[kBlock];
    __shared__ double best_err[kBlock];
    __shared__ int best_k[kBlock];
    __shared__ unsigned int found[2];
    const int t = threadIdx.x;
    const int bins = a.bins;
    const unsigned long long* cnt = a.counts + (int64_t)blockIdx.x * (bins + 3);
    const float lo_f = a.range2[2 * blockIdx.x], hi_f = a.range2[2 * blockIdx.x + 1];
    const int bits = a.num_bits[blockIdx.x];
    float* out = a.out2 + 2 * blockIdx.x;
    const double lo = (double)lo_f, hi = (double)hi_f;
    const float w = hi_f - lo_f;
    const bool degenerate = !(w > 0.0f && w < INFINITY);

    for (int b = t; b < bins; b += kBlock) {
        unsigned long long c = cnt[b];
        if (b == 0) c += cnt[bins];                          // below
        if (b == bins - 1) c += cnt[bins + 1];               // above (NaN, slot bins + 2, is ignored)
        nb[b] = c;
        rep[b] = ah_rep(lo, hi, b, bins);
    }
    if (t < 2) found[t] = t == 0 ? (unsigned)bins : 0u;
    __syncthreads();
    // a segment of consecutive bins per thread
    const int per = (bins + kBlock - 1) / kBlock;
    const int b0 = t * per < bins ? t * per : bins;
    const int b1 = b0 + per < bins ? b0 + per : bins;
    unsigned long long mine = 0;
    for (int b = b0; b < b1; ++b) mine += nb[b];
    seg[t] = mine;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (int i = 0; i < kBlock; ++i) {
        if (i == t) before = total;
        total += seg[i];
    }
    // (uniform from here: every thread holds the same total)
    if (degenerate || total == 0 || bits < 2 || bits > 16) {
        if (t == 0) { out[0] = lo_f; out[1] = hi_f; }
        return;
    }
    if (a.method == 0) {
        double kd = ceil(a.param * (double)total);
        if (!(kd >= 1.0)) kd = 1.0;
        if (kd > (double)total) kd = (double)total;
        unsigned long long k = (unsigned long long)kd;
        if (k > total) k = total;                            // ((double)total may have rounded up)
        // first bin whose inclusive prefix sum reaches k; last bin whose inclusive suffix sum does
        unsigned long long run = before;
        for (int b = b0; b < b1; ++b) {
            run += nb[b];
            if (run >= k) { atomicMin(&found[0], (unsigned)b); break; }
        }
        run = total - before - mine;                         // what lies behind the segment
        for (int b = b1 - 1; b >= b0; --b) {
            run += nb[b];
            if (run >= k) { atomicMax(&found[1], (unsigned)b); break; }
        }
        __syncthreads();
        if (t == 0) {
            out[0] = ah_edge(lo, hi, (int)found[1], bins);
            out[1] = ah_edge(lo, hi, (int)found[0] + 1, bins);
        }
        return;
    }
    __syncthreads();                                         // (the prefix sums above read nb as integers)
    for (int b = t; b < bins; b += kBlock) nb[b] = (unsigned long long)__double_as_longlong((double)nb[b]);
    __syncthreads();
    const int k_h = ah_search<true>(nb, rep, lo, hi, bins, a.candidates, bits, lo_f, best_err, best_k);
    const float h = ah_edge(lo, hi, bins - k_h, bins);
    const int k_l = ah_search<false>(nb, rep, lo, hi, bins, a.candidates, bits, h, best_err, best_k);
    if (t == 0) {
        out[0] = ah_edge(lo, hi, k_l, bins);
        out[1] = h;
    }
}

}  // namespace dfq

using namespace dfq;

extern "C" {

int dfq_act_hist_accumulate(const float* x, int64_t n, const float* range2, int32_t bins, unsigned long long* counts, void* stream) {
    const char* me = "dfq_act_hist_accumulate";
    if ((!x && n != 0) || !range2 || !counts) return fail_arg("%s: null %s", me, !x ? "x" : !range2 ? "range2" : "counts");
    if (bins < 2 || bins > kHistMaxBins) return fail_arg("%s: %d bins (2 ... %d)", me, (int)bins, kHistMaxBins);
    if (n < 0) return fail_arg("%s: n = %lld", me, (long long)n);
    if ((uintptr_t)x % 16 != 0) return fail_arg("%s: x is not 16-byte aligned (the caller copies such a view)", me);
    if ((uintptr_t)range2 % 4 != 0 || (uintptr_t)counts % 8 != 0)
        return fail_arg("%s: %s", me, (uintptr_t)range2 % 4 ? "range2 is not 4-byte aligned" : "counts is not 8-byte aligned");
    // rounds per piece: as many as leave about kHistGroups workgroups (the counts do not depend on it: they are integers)
    const int64_t aim = (int64_t)kHistRound * kHistGroups;
    int64_t rounds = (n + aim - 1) / aim;
    rounds = rounds < 1 ? 1 : rounds > kHistMaxRounds ? kHistMaxRounds : rounds;
    const int64_t piece = rounds * kHistRound;
    const int64_t pieces = (n + piece - 1) / piece;
    if (pieces > 0x7fffffff) return fail_arg("%s: n = %lld is more than 2^31 - 1 pieces of %lld floats", me, (long long)n, (long long)piece);
    if (n == 0) return DFQ_OK;
    hipLaunchKernelGGL(ah_piece_kernel, dim3((unsigned)pieces), dim3(kBlock), 0, as_stream(stream), x, n, range2, (int)bins, (int)rounds,
                       counts);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

int dfq_hist_clip_range(const unsigned long long* counts, const float* range2, int32_t n_hist, int32_t bins, const int32_t* num_bits,
                        int32_t method, double param, int32_t candidates, float* out2, void* stream) {
    const char* me = "dfq_hist_clip_range";
    if (!counts || !range2 || !num_bits || !out2)
        return fail_arg("%s: null %s", me, !counts ? "counts" : !range2 ? "range2" : !num_bits ? "num_bits" : "out2");
    if (n_hist < 0) return fail_arg("%s: %d histograms", me, (int)n_hist);
    if (bins < 2 || bins > kHistMaxBins) return fail_arg("%s: %d bins (2 ... %d)", me, (int)bins, kHistMaxBins);
    if (method != 0 && method != 1) return fail_arg("%s: method %d (0: percentile, 1: mse)", me, (int)method);
    if (method == 0 && !(param > 0.5 && param <= 1.0)) return fail_arg("%s: a percentile of %g (0.5 < p <= 1)", me, param);
    if (method == 1 && (candidates < 1 || candidates > bins / 2))
        return fail_arg("%s: %d candidates (1 ... bins / 2 = %d)", me, (int)candidates, (int)bins / 2);
    if ((uintptr_t)counts % 8 != 0 || (uintptr_t)range2 % 4 != 0 || (uintptr_t)num_bits % 4 != 0 || (uintptr_t)out2 % 4 != 0)
        return fail_arg("%s: a misaligned pointer (counts: 8 bytes, the others: 4)", me);
    if (n_hist == 0) return DFQ_OK;
    AsArgs a;
    a.counts = counts;
    a.range2 = range2;
    a.num_bits = num_bits;
    a.out2 = out2;
    a.param = param;
    a.bins = bins;
    a.method = method;
    a.candidates = candidates;
    hipLaunchKernelGGL(ah_select_kernel, dim3((unsigned)n_hist), dim3(kBlock), 0, as_stream(stream), a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
