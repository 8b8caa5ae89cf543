// Per-output-channel weight quantisation of a whole network (or batch) in ONE launch (extension: the per-channel counterpart of
// layer_transform.py:71-89 quantize_targ_layer, whose per-tensor recipe is dfq_quant_plan's two launches).  Every segment is a
// [rows, row_len] matrix; row r is fake-quantised in place with the reference's UniformQuantize recipe (utils/quantize.py:23-76,
// Python-float min/max: qparams_double + fake_quant_one) and its own (min, max) -- what dfq_fake_quant_rows does for one tensor.
// A per-tensor segment (a bias) is a segment of one row.  One wave owns a row: it finds the row's min and max, writes the pair if
// asked, then quantises the row (the second read hits the cache) and writes the integer codes if asked.
#include <vector>

#include "dfq_range.hpp"

namespace dfq {

struct RowSegDev {
    float* data;
    int32_t* codes;
    float* ranges;
    int64_t row_len;
    int32_t num_bits, symmetric;
    int32_t row_begin, pad;      // first global row of the segment
};

__global__ __launch_bounds__(kBlock) void row_seg_quant_kernel(const RowSegDev* __restrict__ segs, const int32_t* __restrict__ row_begin,
                                                               int n_segs, int total_rows) {
    const int r = (int)blockIdx.x * (kBlock / kWave) + (int)threadIdx.x / kWave;
    if (r >= total_rows) return;                       // (wave-uniform)
    const int lane = threadIdx.x % kWave;
    const RowSegDev sg = segs[find_segment(row_begin, n_segs, r)];
    const int64_t o = r - sg.row_begin;
    float* x = sg.data + o * sg.row_len;
    float mn, mx;
    wave_row_range(x, sg.row_len, mn, mx);
    if (sg.ranges && lane == 0) { sg.ranges[2 * o + 0] = mn; sg.ranges[2 * o + 1] = mx; }
    const QParams p = qparams_double((double)mn, (double)mx, sg.num_bits, sg.symmetric);
    for (int64_t i = lane; i < sg.row_len; i += kWave) {
        float code;
        x[i] = fake_quant_one(x[i], p, &code);
        if (sg.codes) sg.codes[o * sg.row_len + i] = (int32_t)code;
    }
}

}  // namespace dfq

using namespace dfq;

struct dfq_row_quant_plan {
    int n_segs = 0;
    int total_rows = 0;
    RowSegDev* d_segs = nullptr;
    int32_t* d_row_begin = nullptr;
};

extern "C" {

void dfq_row_quant_plan_destroy(dfq_row_quant_plan* p) {
    if (!p) return;
    dfq::dev_quiesce();                                  // nothing in flight may still use the blocks released below
    if (p->d_segs) dfq::dev_free(p->d_segs);
    if (p->d_row_begin) dfq::dev_free(p->d_row_begin);
    delete p;
}

int dfq_row_quant_plan_create(const dfq_row_segment* segs, int32_t n_segs, dfq_row_quant_plan** out_plan) {
    if (!segs || n_segs <= 0 || !out_plan) return fail_arg("dfq_row_quant_plan_create: bad argument");
    std::vector<RowSegDev> h(n_segs);
    std::vector<int32_t> rb(n_segs);
    int64_t rows = 0;
    for (int i = 0; i < n_segs; ++i) {
        const dfq_row_segment& s = segs[i];
        if (!s.data || s.rows <= 0 || s.row_len <= 0) return fail_arg("dfq_row_quant_plan_create: segment %d is empty", i);
        if (s.num_bits < 2 || s.num_bits > 16) return fail_arg("dfq_row_quant_plan_create: segment %d: num_bits %d outside [2, 16]", i, (int)s.num_bits);
        h[i].data = s.data; h[i].codes = s.codes; h[i].ranges = s.ranges; h[i].row_len = s.row_len;
        h[i].num_bits = s.num_bits; h[i].symmetric = s.symmetric ? 1 : 0;
        h[i].row_begin = (int32_t)rows; h[i].pad = 0;
        rb[i] = (int32_t)rows;
        rows += s.rows;
        if (rows > 0x7fffffff - kBlock) return fail_arg("dfq_row_quant_plan_create: too many rows");
    }
    dfq_row_quant_plan* p = new dfq_row_quant_plan();
    p->n_segs = n_segs;
    p->total_rows = (int)rows;
    hipError_t e;
    if ((e = dfq::dev_malloc((void**)&p->d_segs, sizeof(RowSegDev) * n_segs)) != hipSuccess ||
        (e = dfq::dev_malloc((void**)&p->d_row_begin, sizeof(int32_t) * n_segs)) != hipSuccess ||
        (e = hipMemcpy(p->d_segs, h.data(), sizeof(RowSegDev) * n_segs, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(p->d_row_begin, rb.data(), sizeof(int32_t) * n_segs, hipMemcpyHostToDevice)) != hipSuccess) {
        dfq_row_quant_plan_destroy(p);
        return fail_hip(e, "row quant plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_row_quant_plan_run(dfq_row_quant_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_row_quant_plan_run: null plan");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(row_seg_quant_kernel, dim3((p->total_rows + kBlock / kWave - 1) / (kBlock / kWave)), dim3(kBlock), 0, st,
                       (const RowSegDev*)p->d_segs, (const int32_t*)p->d_row_begin, p->n_segs, p->total_rows);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
