// Analytic activation ranges of a whole batch of networks of one architecture (extension: set_quant_minmax,
// utils/layer_transform.py:347-609, main_cls.py:188, for every network of an arena.NetworkBatch at once).  The plan holds
// the program the host compiled from ONE walk over network 0's graph (find_prev_bn, :299-344, the branch grouping of
// :476-580) and one byte offset per network, like dfq_batch_quant_plan and dfq_batch_absorb_plan.
//
// This is latency-bound work on channel vectors of at most a few thousand floats: the design goal is the launch count and
// zero host round trips, not bandwidth.  One launch, two with case (d), neither with a wait inside:
//   1. act_source_kernel (only when the program has sources, case d, :451-466): a BatchNorm proxy vector pushed through a
//      conv / linear layer without BatchNorm of its own.  One wave per output row, lane-strided, the kernel taps summed in
//      float32, the products accumulated in float64, wave_sum's butterfly: bn_through_layer_kernel's order (dfq_act.hip).
//      The vectors go to a block [n_nets][source stride] the plan owns.
//   2. act_range_kernel, one workgroup of kBlock threads per (network, result).  A thread owns channels i, i + kBlock, ...
//      and carries a channel's (mean, var) through ALL moment steps of the result in registers (a branch of any depth needs
//      no scratch memory and no second launch), then folds its channels with nan_min / nan_max in rising i; block_minmax
//      folds the workgroup.  That is the partition and the order of bn_ranges_kernel / moment_range_kernel, so the fold gives
//      the same bit pattern whatever NaNs the vectors hold.  The scalar combination across sources, which the
//      single-network path does on Python floats (min, max, +=, /=) before fill_() rounds them into a float32 buffer, is
//      done in float64 by every thread alike and rounded to float32 once, at the store.
// Results are written with ordinary vector stores; the tables are uploaded in create, run copies nothing.
#include <math.h>

#include <vector>

#include "dfq_act_shared.hpp"
#include "dfq_batch_shared.hpp"

namespace dfq {

constexpr int kActWaves = kBlock / kWave;

struct ActStepDev {
    const float* fw;              // network 0; with `sourced`: floats into a network's source block
    const float* fb;
    int64_t src_w, src_b;         // offsets into a network's source block (sourced steps)
    int32_t opcode, channels, relu_mode, operand;
    int32_t sourced;
    float lo, hi;
};

struct ActResultDev {
    int32_t begin, end;           // steps
};

struct ActSourceDev {
    const float* w;               // network 0
    const float* bias;            // may be null
    const float* vin;
    int64_t out_off;              // floats into a network's source block
    int32_t out_ch, ipg, khkw, groups;
    int32_t block_begin;          // first workgroup (within one network)
};

struct ActArgs {
    const ActResultDev* results;
    const ActStepDev* steps;
    const ActSourceDev* sources;
    const int32_t* block_source;  // source of every workgroup of network 0 (launch 1)
    const int64_t* delta;         // bases[n] - bases[0], bytes
    float* src_block;             // [n_nets][src_stride]
    float* out;                   // [n_nets][out_stride]
    int64_t src_stride, out_stride;
    float n_sigma, eps;
    int32_t n_results, n_nets, src_blocks_pn;
};

__device__ __forceinline__ const float* act_at(const float* p, int64_t delta) { return (const float*)((const char*)p + delta); }

// launch 1: v_out[o] = sum_i (sum_k W[o, i, k]) * v_in[group(o) * I/g + i] + bias[o] for every source of every network
__global__ __launch_bounds__(kBlock) void act_source_kernel(ActArgs a) {
    const int net = (int)blockIdx.x / a.src_blocks_pn;
    const int lb = (int)blockIdx.x - net * a.src_blocks_pn;
    const ActSourceDev S = a.sources[a.block_source[lb]];
    const int o = (lb - S.block_begin) * kActWaves + (int)threadIdx.x / kWave;
    if (o >= S.out_ch) return;
    const int lane = threadIdx.x % kWave;
    const int64_t d = a.delta[net];
    const int g = o / (S.out_ch / S.groups);
    const float* row = act_at(S.w, d) + (int64_t)o * S.ipg * S.khkw;
    const float* vin = act_at(S.vin, d) + (int64_t)g * S.ipg;
    double acc = 0.0;
    for (int i = lane; i < S.ipg; i += kWave) {
        float ws = 0.0f;
        for (int k = 0; k < S.khkw; ++k) ws = ws + row[(int64_t)i * S.khkw + k];     // layer_weight.view(O, I, -1).sum(-1)
        acc += (double)ws * (double)vin[i];
    }
    acc = wave_sum(acc);
    if (lane == 0) a.src_block[(int64_t)net * a.src_stride + S.out_off + o] = (float)acc + (S.bias ? act_at(S.bias, d)[o] : 0.0f);
}

// the two vectors of a step in network `net`
__device__ __forceinline__ void act_vectors(const ActArgs& a, const ActStepDev& S, int net, int64_t d, const float*& fw, const float*& fb) {
    if (S.sourced) {
        const float* blk = a.src_block + (int64_t)net * a.src_stride;
        fw = blk + S.src_w;
        fb = blk + S.src_b;
    } else {
        fw = act_at(S.fw, d);
        fb = act_at(S.fb, d);
    }
}

// launch 2: one workgroup per (network, result)
__global__ __launch_bounds__(kBlock) void act_range_kernel(ActArgs a) {
    __shared__ float sh[2 * kActWaves];
    const int net = (int)blockIdx.x / a.n_results;
    const int q = (int)blockIdx.x - net * a.n_results;
    const ActResultDev R = a.results[q];
    const int64_t d = a.delta[net];
    double vmin = 0.0, vmax = 0.0;
    for (int s = R.begin; s < R.end; ++s) {                  // (block-uniform: every thread walks the same steps)
        const ActStepDev S = a.steps[s];
        if (S.opcode == DFQ_ACT_CONST) {
            vmin = (double)S.lo;
            vmax = (double)S.hi;
        } else if (S.opcode == DFQ_ACT_RANGE_DIV) {
            vmin /= (double)S.operand;
            vmax /= (double)S.operand;
        } else if (S.opcode == DFQ_ACT_MOM) {
            int e = s + 1;
            while (a.steps[e].opcode != DFQ_ACT_MOM_RANGE) ++e;          // create has checked that the group is closed
            float mn = INFINITY, mx = -INFINITY;
            for (int i = threadIdx.x; i < S.channels; i += kBlock) {
                float mean = 0.0f, var = 0.0f;
                for (int t = s; t < e; ++t) {
                    const ActStepDev T = a.steps[t];
                    if (T.opcode == DFQ_ACT_MOM_RELU) {
                        const float sd = sd_of(var, a.eps);
                        float m, v;
                        moments_of(T.relu_mode, sd, mean, m, v);                 // moments_after_add_kernel
                        mean = m;
                        var = v;
                    } else {
                        const float *fw, *fb;
                        act_vectors(a, T, net, d, fw, fb);
                        float m, v;
                        moments_of(T.relu_mode, fw[i], fb[i], m, v);             // relu_moments_kernel
                        if (T.opcode == DFQ_ACT_MOM_ADD) { m = mean + m; v = var + v; }
                        mean = m;
                        var = v;
                    }
                }
                const float nw = a.n_sigma * sd_of(var, a.eps);                 // moment_range_kernel
                mn = nan_min(mean - nw, mn);
                mx = nan_max(mean + nw, mx);
            }
            __syncthreads();                                 // `sh` may still be read from the fold before
            block_minmax(mn, mx, sh);
            vmin = (double)mn;
            vmax = (double)mx;
            s = e;
        } else {                                             // RANGE, RANGE_CAT, RANGE_ONE: bn_ranges_kernel
            const float *fw, *fb;
            act_vectors(a, S, net, d, fw, fb);
            float mn = INFINITY, mx = -INFINITY;
            for (int i = threadIdx.x; i < S.channels; i += kBlock) {
                const float nw = a.n_sigma * fw[i];
                mn = nan_min(fb[i] - nw, mn);
                mx = nan_max(fb[i] + nw, mx);
            }
            __syncthreads();
            block_minmax(mn, mx, sh);
            if (S.relu_mode >= 1) mn = (mn > 0.0f) ? mn : 0.0f;     // Python max(0., v): NaN -> 0
            if (S.relu_mode == 2) mx = (mx < 6.0f) ? mx : 6.0f;     // Python min(6., v): NaN -> 6
            const double lo = (double)mn, hi = (double)mx;
            if (S.opcode == DFQ_ACT_RANGE) {
                vmin = lo;
                vmax = hi;
            } else if (S.opcode == DFQ_ACT_RANGE_CAT) {
                vmin = (lo < vmin) ? lo : vmin;              // Python min(value_min, lo): the first unless the second is smaller
                vmax = (hi > vmax) ? hi : vmax;              // Python max(value_max, hi)
            } else {
                vmin += (lo > 0.0) ? lo : 0.0;               // value_min += max(0., lo)
                vmax += hi;
            }
        }
    }
    if (threadIdx.x == 0) {
        float* o = a.out + (int64_t)net * a.out_stride + 2 * q;
        o[0] = (float)vmin;
        o[1] = (float)vmax;
    }
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_act_plan {
    DevSlab mem;
    ActArgs args{};
    int source_blocks = 0, range_blocks = 0;
};

extern "C" {

int32_t dfq_batch_act_plan_launches(const dfq_batch_act_plan* p) { return p ? (p->source_blocks > 0) + (p->range_blocks > 0) : 0; }

void dfq_batch_act_plan_destroy(dfq_batch_act_plan* p) { batch_plan_destroy(p); }

int dfq_batch_act_plan_create(const dfq_batch_act_result* results, int32_t n_results, const dfq_batch_act_step* steps, int32_t n_steps,
                              const dfq_batch_act_source* sources, int32_t n_sources, const void* const* bases, int32_t n_nets,
                              float n_sigma, float eps, float* out, int64_t out_stride, dfq_batch_act_plan** out_plan) {
    const char* me = "dfq_batch_act_plan_create";
    if (!out_plan) return fail_arg("%s: no place for the plan", me);
    if (!results || n_results <= 0 || !steps || n_steps <= 0) return fail_arg("%s: the result or the step table is null or empty", me);
    if (n_sources < 0 || (n_sources > 0 && !sources)) return fail_arg("%s: the source table is null or its count negative", me);
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    if (!isfinite(n_sigma) || !isfinite(eps)) return fail_arg("%s: n_sigma or eps is not finite", me);
    if (!out || out_stride < 2 * (int64_t)n_results) return fail_arg("%s: no block for the ranges, or a stride below 2 * n_results", me);
    if ((int64_t)n_results * n_nets > 0x7fffffff) return fail_arg("%s: too much work for one launch", me);

    // case (d) sources: where each lands in a network's block, and the workgroups of launch 1
    std::vector<ActSourceDev> srcs((size_t)n_sources);
    std::vector<int32_t> block_source;
    int64_t src_stride = 0, src_blocks = 0;
    for (int i = 0; i < n_sources; ++i) {
        const dfq_batch_act_source& s = sources[i];
        if (!s.weight || !s.vector || s.out_ch <= 0 || s.in_per_group <= 0 || s.khkw <= 0 || s.groups <= 0 || s.out_ch % s.groups != 0)
            return fail_arg("%s: source %d: null tensor or unsupported geometry", me, i);
        ActSourceDev& D = srcs[i];
        D.w = s.weight; D.bias = s.bias; D.vin = s.vector;
        D.out_ch = s.out_ch; D.ipg = s.in_per_group; D.khkw = s.khkw; D.groups = s.groups;
        D.out_off = src_stride;
        src_stride += (int64_t)((s.out_ch + 63) / 64) * 64;
        const int64_t k = (s.out_ch + kActWaves - 1) / kActWaves;
        D.block_begin = (int32_t)src_blocks;
        block_source.insert(block_source.end(), (size_t)k, (int32_t)i);
        src_blocks += k;
    }
    if (src_blocks * n_nets > 0x7fffffff || src_stride > 0x7fffffff / n_nets) return fail_arg("%s: too much work for one launch", me);

    std::vector<ActStepDev> dsteps((size_t)n_steps);
    for (int i = 0; i < n_steps; ++i) {
        const dfq_batch_act_step& s = steps[i];
        ActStepDev& D = dsteps[i];
        D.fw = s.fake_weight; D.fb = s.fake_bias;
        D.opcode = s.opcode; D.channels = s.channels; D.relu_mode = s.relu_mode; D.operand = s.operand;
        D.lo = s.lo; D.hi = s.hi;
        D.src_w = D.src_b = 0;
        D.sourced = 0;
        if (s.opcode < DFQ_ACT_CONST || s.opcode > DFQ_ACT_MOM_RANGE) return fail_arg("%s: step %d: unknown opcode %d", me, i, (int)s.opcode);
        const bool reads = s.opcode == DFQ_ACT_RANGE || s.opcode == DFQ_ACT_RANGE_CAT || s.opcode == DFQ_ACT_RANGE_ONE ||
                           s.opcode == DFQ_ACT_MOM || s.opcode == DFQ_ACT_MOM_ADD;
        if ((reads || s.opcode == DFQ_ACT_MOM_RELU) && (s.relu_mode < 0 || s.relu_mode > 2))
            return fail_arg("%s: step %d: ReLU mode %d", me, i, (int)s.relu_mode);
        if (s.opcode == DFQ_ACT_MOM_RELU && s.relu_mode == 0) return fail_arg("%s: step %d: a ReLU step without ReLU", me, i);
        if (s.opcode == DFQ_ACT_RANGE_DIV && s.operand <= 0) return fail_arg("%s: step %d: divisor %d", me, i, (int)s.operand);
        if (!reads) continue;
        if (s.channels <= 0) return fail_arg("%s: step %d: no channels", me, i);
        if (s.source_weight >= 0 || s.source_bias >= 0) {
            if (s.source_weight < 0 || s.source_weight >= n_sources || s.source_bias < 0 || s.source_bias >= n_sources)
                return fail_arg("%s: step %d: source index out of range", me, i);
            if (srcs[s.source_weight].out_ch != s.channels || srcs[s.source_bias].out_ch != s.channels)
                return fail_arg("%s: step %d: its sources do not have %d channels", me, i, (int)s.channels);
            D.sourced = 1;
            D.src_w = srcs[s.source_weight].out_off;
            D.src_b = srcs[s.source_bias].out_off;
            D.fw = D.fb = nullptr;
        } else if (!s.fake_weight || !s.fake_bias) {
            return fail_arg("%s: step %d: null vector", me, i);
        }
    }
    std::vector<ActResultDev> dres((size_t)n_results);
    for (int r = 0; r < n_results; ++r) {
        const int b = results[r].step_begin, c = results[r].step_count;
        if (b < 0 || c <= 0 || b > n_steps - c) return fail_arg("%s: result %d: steps outside the table", me, r);
        dres[r].begin = b;
        dres[r].end = b + c;
        const int first = steps[b].opcode;
        bool ok = true;
        if (first == DFQ_ACT_CONST) {
            ok = c == 1;
        } else if (first == DFQ_ACT_RANGE) {
            for (int i = b + 1; i < b + c; ++i)
                ok = ok && (steps[i].opcode == DFQ_ACT_RANGE_CAT || steps[i].opcode == DFQ_ACT_RANGE_ONE || steps[i].opcode == DFQ_ACT_RANGE_DIV);
        } else if (first == DFQ_ACT_MOM) {
            ok = c >= 2 && steps[b + c - 1].opcode == DFQ_ACT_MOM_RANGE;
            for (int i = b + 1; i < b + c - 1; ++i) {
                ok = ok && (steps[i].opcode == DFQ_ACT_MOM_ADD || steps[i].opcode == DFQ_ACT_MOM_RELU);
                if (steps[i].opcode == DFQ_ACT_MOM_ADD && steps[i].channels != steps[b].channels)
                    return fail_arg("%s: result %d: the sources of an add have %d and %d channels", me, r, (int)steps[b].channels, (int)steps[i].channels);
            }
        } else {
            ok = false;
        }
        if (!ok) return fail_arg("%s: result %d: its steps are not CONST, RANGE [CAT | ONE | DIV]... or MOM [ADD | RELU]... MOM_RANGE", me, r);
    }

    dfq_batch_act_plan* p = new dfq_batch_act_plan();
    ActArgs& a = p->args;
    a.out = out;
    a.out_stride = out_stride;
    a.src_stride = src_stride;
    a.n_sigma = n_sigma;
    a.eps = eps;
    a.n_results = n_results;
    a.n_nets = n_nets;
    a.src_blocks_pn = (int32_t)src_blocks;
    p->range_blocks = n_results * n_nets;
    p->source_blocks = (int)(src_blocks * n_nets);
    BatchUpload up{p->mem};
    a.results = up.put(dres);
    a.steps = up.put(dsteps);
    a.sources = up.put(srcs);
    a.block_source = up.put(block_source);
    a.delta = up.put(batch_delta(bases, n_nets));
    a.src_block = (float*)up.raw(nullptr, sizeof(float) * (size_t)src_stride * n_nets);
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch activation-range plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_act_plan_run(dfq_batch_act_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_act_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    const ActArgs& a = p->args;
    if (p->source_blocks > 0) {
        hipLaunchKernelGGL(act_source_kernel, dim3(p->source_blocks), dim3(kBlock), 0, st, a);
        DFQ_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(act_range_kernel, dim3(p->range_blocks), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
