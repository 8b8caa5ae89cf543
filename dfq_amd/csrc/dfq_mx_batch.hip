// MX block-scaled FP4 / FP6 / FP8 weights (extension; the OCP Microscaling formats of gfx950's block-scaled MFMA).  The
// DEFINITION is in include/dfq_hip.h ("MX block-scaled"); tests/test_batch_mx.py restates it in numpy.
//
// Half a wave takes a block of 32 elements, a lane an element: the block's largest magnitude is an unsigned max of the
// bit patterns over the 32 lanes (five register-file exchanges, no LDS), the block error S(e) the five-level tree of
// xor_lane_add the definition names.  A workgroup takes kMxGroupBlocks consecutive blocks of ONE tensor of one network, eight
// blocks at a time; blocks past the tensor's end and elements past a row's end run along as +0.0 and store nothing, so every
// exchange is reached by whole waves.  The format table and the conversion of one element are dfq_mx.hpp's, shared with the
// lane-per-block kernel of dfq_mx_axis.hip.
//   errors    every candidate format from one read; a workgroup's sum over its blocks goes to a partial sum of the plan, a
//             second launch adds a tensor's partial sums in a fixed order (no floating-point atomic)
//   quantise  the weight, the code byte and the scale byte; the width is the table's or one scalar load per workgroup
//   decode    a lane per element, no exchange at all
#include <vector>

#include "dfq_batch_shared.hpp"
#include "dfq_mx.hpp"

namespace dfq {

constexpr int kMxPerPass = kBlock / kMxBlock;                  // blocks a workgroup takes at a time
constexpr int kMxPasses = 8;
constexpr int kMxGroupBlocks = kMxPerPass * kMxPasses;         // blocks of one tensor a workgroup takes
constexpr int kMxMaxF = 3;

typedef DFQ_GLOBAL_AS uint8_t mx_guint8;
typedef DFQ_GLOBAL_AS double mx_gdouble;
typedef DFQ_GLOBAL_AS int32_t mx_gint32;

struct MxTensorDev {              // addresses in network 0
    const float* x;
    float* y;
    int64_t code_off, scale_off;  // into one network's row, -1 = none
    int32_t rows, len, bpr, n_blocks;
    int32_t item_begin, items;    // the tensor's workgroups within one network
    int32_t num_bits, width_index;      // decode: the tensor's own width, or 0 and its place in a row of the widths
};

struct MxArgs {
    MxTensorDev one;              // the tensor of a single call (tensors == null)
    const MxTensorDev* tensors;
    const int32_t* item_tensor;   // tensor of every workgroup of network 0
    const int64_t* delta;         // bases[n] - bases[0], bytes (null: one network)
    double* errors;               // [n_nets, n_tensors, nf]
    double* partial;              // [n_nets, items_pn, nf], the plan's own
    double* block_err;            // dfq_mx_rows: S of every block
    uint8_t* codes;
    uint8_t* scales;
    int64_t code_stride, scale_stride;
    int32_t items_pn, n_tensors;
    int32_t nf, search;
    int32_t widths[kMxMaxF], fmt[kMxMaxF];
    int32_t qfmt;                 // the format QUANTISE works at without device widths
};

struct MxWidths {                 // dfq_batch_squant_plan_set_widths' shape
    const int32_t* widths;        // [n_nets, stride]
    const int32_t* index;         // [n_tensors]
    int32_t* status;              // [n_nets]
    int64_t stride;
};

// ---- the 32 lanes of a block ---------------------------------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ uint32_t mx_xor_umax(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t p;
    if (M == 1) p = dpp_move<0xB1, 0xf>(v, v);
    else if (M == 2) p = dpp_move<0x4E, 0xf>(v, v);
    else if (M == 4) p = dpp_move<0x114, 0xA>(dpp_move<0x104, 0x5>(v, v), v);
    else if (M == 8) p = dpp_move<0x118, 0xC>(dpp_move<0x108, 0x3>(v, v), v);
    else {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);     // the own word and the partner's, in either order
        return r[0] > r[1] ? r[0] : r[1];
    }
    return v > p ? v : p;
#else
    const uint32_t p = __shfl_xor(v, M);
    return v > p ? v : p;
#endif
}
__device__ __forceinline__ uint32_t mx_block_umax(uint32_t v) {
    v = mx_xor_umax<1>(v); v = mx_xor_umax<2>(v); v = mx_xor_umax<4>(v); v = mx_xor_umax<8>(v);
    return mx_xor_umax<16>(v);
}
// the definition's tree: level m pairs index i with i xor m (both lanes of a pair add the same two numbers)
__device__ __forceinline__ double mx_block_sum(double v) {
    xor_lane_add<1>(v); xor_lane_add<2>(v); xor_lane_add<4>(v); xor_lane_add<8>(v); xor_lane_add<16>(v);
    return v;
}

// ---- an element and its block (the conversion itself: dfq_mx.hpp) ---------------------------------------------------------------
__device__ __forceinline__ MxElem mx_elem(float w) {
    MxElem L = mx_split(w);
    const uint32_t amax = mx_block_umax(__float_as_uint(w) & 0x7fffffffu);       // (the patterns of non-negative floats are ordered as the values, NaN on top)
    L.E = (int32_t)(amax >> 23) - 127;
    L.bad = amax >= 0x7f800000u;
    return L;
}

// The block's shared exponent at format f and its S(e) (NaN for a block that is not finite).  Reached by whole waves.
__device__ __forceinline__ int mx_exponent(const MxElem& L, const MxFmt& f, int search, double& S) {
    const int e0 = L.E - f.emax > -127 ? L.E - f.emax : -127;
    int e = e0;
    S = mx_block_sum(mx_sq_error(mx_value_bits(mx_encode(L, e0, f), e0, f) | L.sign, L.w));
    if (search) {                                      // (uniform over the launch)
        const double S1 = mx_block_sum(mx_sq_error(mx_value_bits(mx_encode(L, e0 + 1, f), e0 + 1, f) | L.sign, L.w));
        if (S1 < S) { e = e0 + 1; S = S1; }            // (a tie, and a NaN on either side, keep e0)
    }
    if (L.bad) S = __builtin_nan("");
    return e;
}

// where lane `threadIdx.x % 32` of the half wave that takes block b of T stands: its element's index in the tensor, or -1
__device__ __forceinline__ int64_t mx_element(const MxTensorDev& T, int b) {
    if (b >= T.n_blocks) return -1;
    const int r = b / T.bpr, j = b - r * T.bpr;
    const int col = j * kMxBlock + (int)(threadIdx.x % kMxBlock);
    return col < T.len ? (int64_t)r * T.len + col : -1;
}

// ---- ERRORS -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mx_errors_kernel(MxArgs a) {
    __shared__ double sh[kBlock / kWave];
    const int net = (int)blockIdx.x / a.items_pn;
    const int item = (int)blockIdx.x - net * a.items_pn;
    const MxTensorDev T = a.tensors[a.item_tensor[item]];
    const gfloat* x = (const gfloat*)(const float*)((const char*)T.x + a.delta[net]);
    const int b0 = (item - T.item_begin) * kMxGroupBlocks + (int)threadIdx.x / kMxBlock;
    double acc[kMxMaxF] = {0.0, 0.0, 0.0};
    for (int pass = 0; pass < kMxPasses; ++pass) {
        const int64_t at = mx_element(T, b0 + pass * kMxPerPass);
        const MxElem L = mx_elem(at >= 0 ? x[at] : 0.0f);
#pragma unroll
        for (int f = 0; f < kMxMaxF; ++f) {
            if (f < a.nf) {
                double S;
                mx_exponent(L, mx_fmt(a.fmt[f]), a.search, S);
                acc[f] += S;                           // (the same in the 32 lanes of the block)
            }
        }
    }
#pragma unroll
    for (int f = 0; f < kMxMaxF; ++f) {
        if (f < a.nf) {
            const double v = block_sum(threadIdx.x % kMxBlock == 0 ? acc[f] : 0.0, sh);
            if (threadIdx.x == 0) ((mx_gdouble*)a.partial)[((int64_t)net * a.items_pn + item) * a.nf + f] = v;
        }
    }
}

// a workgroup per (network, tensor): thread t adds the partial sums t, t + kBlock, ... of the tensor, then the fixed block sum
__global__ __launch_bounds__(kBlock) void mx_errors_finish_kernel(MxArgs a) {
    __shared__ double sh[kBlock / kWave];
    const int net = (int)blockIdx.x / a.n_tensors;
    const int ti = (int)blockIdx.x - net * a.n_tensors;
    const MxTensorDev T = a.tensors[ti];
    const mx_gdouble* part = (const mx_gdouble*)a.partial + ((int64_t)net * a.items_pn + T.item_begin) * a.nf;
#pragma unroll
    for (int f = 0; f < kMxMaxF; ++f) {
        if (f < a.nf) {
            double v = 0.0;
            for (int i = (int)threadIdx.x; i < T.items; i += kBlock) v += part[(int64_t)i * a.nf + f];
            v = block_sum(v, sh);
            if (threadIdx.x == 0) ((mx_gdouble*)a.errors)[((int64_t)net * a.n_tensors + ti) * a.nf + f] = v;
        }
    }
}

// ---- QUANTISE ---------------------------------------------------------------------------------------------------------------------
template <bool kDeviceWidths>
__device__ __forceinline__ void mx_quant_item(const MxArgs& a, const MxWidths& wd) {
    const int net = (int)blockIdx.x / a.items_pn;
    const int item = (int)blockIdx.x - net * a.items_pn;
    int fmt = a.qfmt;
    if constexpr (kDeviceWidths) {                     // (a plan's launch: the tensors are a table)
        const int bits = __builtin_amdgcn_readfirstlane(wd.widths[(int64_t)net * wd.stride + wd.index[a.item_tensor[item]]]);
        fmt = -1;
#pragma unroll
        for (int f = 0; f < kMxMaxF; ++f)
            if (f < a.nf && a.widths[f] == bits) fmt = a.fmt[f];
        if (fmt < 0) {                                 // no candidate: the whole workgroup, before any exchange
            if (threadIdx.x == 0) ((mx_gint32*)wd.status)[net] = 2;
            return;
        }
    }
    const MxTensorDev T = a.tensors ? a.tensors[a.item_tensor[item]] : a.one;
    const MxFmt F = mx_fmt(fmt);
    const int64_t dbytes = a.delta ? a.delta[net] : 0;
    const gfloat* x = (const gfloat*)(const float*)((const char*)T.x + dbytes);
    gfloat* y = T.y ? (gfloat*)(float*)((char*)T.y + dbytes) : nullptr;
    mx_guint8* codes = T.code_off >= 0 ? (mx_guint8*)a.codes + (int64_t)net * a.code_stride + T.code_off : nullptr;
    mx_guint8* scales = T.scale_off >= 0 ? (mx_guint8*)a.scales + (int64_t)net * a.scale_stride + T.scale_off : nullptr;
    const int b0 = (item - T.item_begin) * kMxGroupBlocks + (int)threadIdx.x / kMxBlock;
    for (int pass = 0; pass < kMxPasses; ++pass) {
        const int b = b0 + pass * kMxPerPass;
        const int64_t at = mx_element(T, b);
        const MxElem L = mx_elem(at >= 0 ? x[at] : 0.0f);
        double S;
        const int e = mx_exponent(L, F, a.search, S);
        const uint32_t k = L.bad ? 0u : mx_encode(L, e, F);
        if (at >= 0) {
            if (y) y[at] = __uint_as_float(L.bad ? kMxQuietNan : (mx_value_bits(k, e, F) | L.sign));
            if (codes) codes[at] = (uint8_t)(L.bad ? 0u : (k | (L.sign >> (32 - F.bits))));
        }
        if (threadIdx.x % kMxBlock == 0 && b < T.n_blocks) {
            if (scales) scales[b] = (uint8_t)(L.bad ? 255 : e + 127);
            if (a.block_err) ((mx_gdouble*)a.block_err)[b] = S;
        }
    }
}

__global__ __launch_bounds__(kBlock) void mx_quant_kernel(MxArgs a) { mx_quant_item<false>(a, MxWidths{}); }
__global__ __launch_bounds__(kBlock) void mx_quant_widths_kernel(MxArgs a, MxWidths wd) { mx_quant_item<true>(a, wd); }

// ---- decode ------------------------------------------------------------------------------------------------------------------------
struct MxDecodeArgs {
    const MxTensorDev* tensors;
    const int32_t* item_tensor;
    const int64_t* delta;
    const uint8_t* codes;
    const uint8_t* scales;
    const int32_t* widths;        // [n_nets, width_stride], or null
    const int32_t* gate;          // [n_nets], or null: a network whose word is not 0 is left as it is
    int32_t* status;
    int64_t code_stride, scale_stride, width_stride;
    int32_t items_pn, format6, format8;
};

__global__ __launch_bounds__(kBlock) void mx_decode_kernel(MxDecodeArgs a) {
    const int net = (int)blockIdx.x / a.items_pn;
    const int item = (int)blockIdx.x - net * a.items_pn;
    if (a.gate && __builtin_amdgcn_readfirstlane(a.gate[net]) != 0) return;       // (the launch in front skipped this network)
    const MxTensorDev T = a.tensors[a.item_tensor[item]];
    int bits = T.num_bits;
    if (bits == 0) bits = __builtin_amdgcn_readfirstlane(a.widths[(int64_t)net * a.width_stride + T.width_index]);
    if (bits != 4 && bits != 6 && bits != 8) {
        if (threadIdx.x == 0) ((mx_gint32*)a.status)[net] = 2;
        return;
    }
    const MxFmt F = mx_fmt(bits == 4 ? DFQ_MX_E2M1 : (bits == 6 ? a.format6 : a.format8));
    gfloat* y = (gfloat*)(float*)((char*)T.y + a.delta[net]);
    const mx_guint8* codes = (const mx_guint8*)a.codes + (int64_t)net * a.code_stride + T.code_off;
    const mx_guint8* scales = (const mx_guint8*)a.scales + (int64_t)net * a.scale_stride + T.scale_off;
    const int b0 = (item - T.item_begin) * kMxGroupBlocks + (int)threadIdx.x / kMxBlock;
#pragma unroll
    for (int pass = 0; pass < kMxPasses; ++pass) {
        const int b = b0 + pass * kMxPerPass;
        const int64_t at = mx_element(T, b);
        if (at < 0) continue;
        const uint32_t c = codes[at], s = scales[b];
        const uint32_t sign = ((c >> (F.bits - 1)) & 1u) << 31;
        const uint32_t k = c & ((1u << (F.bits - 1)) - 1u);
        y[at] = __uint_as_float(s == 255u ? kMxQuietNan : (mx_value_bits(k, (int)s - 127, F) | sign));
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
inline bool mx_format_fits(int32_t format6, int32_t format8) {
    return (format6 == DFQ_MX_E2M3 || format6 == DFQ_MX_E3M2) && (format8 == DFQ_MX_E4M3 || format8 == DFQ_MX_E5M2);
}

// the geometry of one tensor into d, its workgroups behind those of `item_tensor`; DFQ_OK or the argument error
inline int mx_add_tensor(const char* me, int i, const float* data, int64_t rows, int64_t row_len, int64_t code_off, int64_t scale_off,
                         int64_t code_stride, int64_t scale_stride, std::vector<int32_t>& item_tensor, MxTensorDev& d) {
    if (!data) return fail_arg("%s: tensor %d: null weight", me, i);
    if ((uintptr_t)data % 4 != 0) return fail_arg("%s: tensor %d: the weight is not 4-byte aligned", me, i);
    if (rows <= 0 || row_len <= 0) return fail_arg("%s: tensor %d is empty (rows %lld, row_len %lld)", me, i, (long long)rows, (long long)row_len);
    if (row_len > 0x7fffffffll) return fail_arg("%s: tensor %d: row_len %lld above 2^31 - 1", me, i, (long long)row_len);
    const int64_t bpr = (row_len + kMxBlock - 1) / kMxBlock;
    if (rows > kMxMost / bpr) return fail_arg("%s: tensor %d: more than 2^29 blocks", me, i);
    const int64_t n_blocks = rows * bpr, numel = rows * row_len;
    if (code_off < -1 || scale_off < -1) return fail_arg("%s: tensor %d: negative offset", me, i);
    if (code_off >= 0 && code_off > code_stride - numel) return fail_arg("%s: tensor %d: codes overflow the code stride", me, i);
    if (scale_off >= 0 && scale_off > scale_stride - n_blocks) return fail_arg("%s: tensor %d: scales overflow the scale stride", me, i);
    const int64_t items = (n_blocks + kMxGroupBlocks - 1) / kMxGroupBlocks;
    if (items > kMxMost - (int64_t)item_tensor.size()) return fail_arg("%s: too much work for one launch", me);
    d = MxTensorDev{};
    d.x = data; d.y = const_cast<float*>(data);
    d.code_off = code_off; d.scale_off = scale_off;
    d.rows = (int32_t)rows; d.len = (int32_t)row_len; d.bpr = (int32_t)bpr; d.n_blocks = (int32_t)n_blocks;
    d.item_begin = (int32_t)item_tensor.size(); d.items = (int32_t)items;
    item_tensor.insert(item_tensor.end(), (size_t)items, i);
    return DFQ_OK;
}

inline int mx_check_nets(const char* me, const void* const* bases, int32_t n_nets, int64_t items_pn) {
    if (const int rc = batch_check_bases(me, bases, n_nets)) return rc;
    for (int n = 1; n < n_nets; ++n)
        if (((uintptr_t)bases[n] - (uintptr_t)bases[0]) % 16 != 0) return fail_arg("%s: network %d is not 16-byte aligned to network 0", me, n);
    if (items_pn * n_nets > kMxMost) return fail_arg("%s: too much work for one launch", me);
    return DFQ_OK;
}

}  // namespace dfq

using namespace dfq;

struct dfq_batch_mx_plan {
    DevSlab mem;
    MxArgs args{};
    MxWidths widths{};            // widths.widths null: the configuration's num_bits (set_widths)
    int32_t n_nets = 0, n_tensors = 0, apply = 0;
    int launches = 0;
};

struct dfq_batch_mx_decode_plan {
    DevSlab mem;
    MxDecodeArgs args{};
    int32_t n_nets = 0;
    bool device_widths = false;
};

namespace {

int mx_run_errors(const dfq_batch_mx_plan* p, hipStream_t st) {
    const MxArgs& a = p->args;
    hipLaunchKernelGGL(mx_errors_kernel, dim3(a.items_pn * p->n_nets), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    hipLaunchKernelGGL(mx_errors_finish_kernel, dim3(p->n_tensors * p->n_nets), dim3(kBlock), 0, st, a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

int mx_run_quantise(const dfq_batch_mx_plan* p, hipStream_t st) {
    const MxArgs& a = p->args;
    const dim3 grid(a.items_pn * p->n_nets);
    if (p->widths.widths) {
        DFQ_HIP_TRY(hipMemsetAsync(p->widths.status, 0, sizeof(int32_t) * (size_t)p->n_nets, st));
        hipLaunchKernelGGL(mx_quant_widths_kernel, grid, dim3(kBlock), 0, st, a, p->widths);
    } else {
        hipLaunchKernelGGL(mx_quant_kernel, grid, dim3(kBlock), 0, st, a);
    }
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // namespace

extern "C" {

int dfq_mx_rows(const float* x, float* y, int64_t rows, int64_t row_len, int32_t format, int32_t search, uint8_t* codes, uint8_t* scales,
                double* err, void* stream) {
    const char* me = "dfq_mx_rows";
    if (format < DFQ_MX_E2M1 || format > DFQ_MX_E5M2) return fail_arg("%s: unknown format %d", me, (int)format);
    MxArgs a{};
    std::vector<int32_t> item_tensor;
    const int64_t big = (int64_t)1 << 62;
    if (const int rc = mx_add_tensor(me, 0, x, rows, row_len, codes ? 0 : -1, scales ? 0 : -1, big, big, item_tensor, a.one)) return rc;
    a.one.y = y;
    a.codes = codes;
    a.scales = scales;
    a.block_err = err;
    a.items_pn = a.one.items;
    a.n_tensors = 1;
    a.search = search ? 1 : 0;
    a.qfmt = format;
    hipLaunchKernelGGL(mx_quant_kernel, dim3(a.items_pn), dim3(kBlock), 0, as_stream(stream), a);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

int32_t dfq_batch_mx_plan_launches(const dfq_batch_mx_plan* p) { return p ? p->launches : 0; }

void dfq_batch_mx_plan_destroy(dfq_batch_mx_plan* p) { batch_plan_destroy(p); }

int dfq_batch_mx_plan_create(const dfq_batch_mx_tensor* tensors, int32_t n_tensors, const dfq_batch_mx_config* config,
                             const void* const* bases, int32_t n_nets, double* errors, uint8_t* codes, int64_t code_stride,
                             uint8_t* scales, int64_t scale_stride, dfq_batch_mx_plan** out_plan) {
    const char* me = "dfq_batch_mx_plan_create";
    if (!tensors || n_tensors <= 0 || !out_plan) return fail_arg("%s: no tensors", me);
    if (!config) return fail_arg("%s: null configuration", me);
    const dfq_batch_mx_config& c = *config;
    if (c.n_widths < 1 || c.n_widths > kMxMaxF) return fail_arg("%s: %d widths (1 to %d)", me, (int)c.n_widths, kMxMaxF);
    for (int f = 0; f < c.n_widths; ++f) {
        const int32_t w = c.widths[f];
        if ((w != 4 && w != 6 && w != 8) || (f > 0 && w <= c.widths[f - 1]))
            return fail_arg("%s: the widths are no rising subset of (4, 6, 8)", me);
    }
    if (!mx_format_fits(c.format6, c.format8))
        return fail_arg("%s: format6 %d / format8 %d do not match their widths", me, (int)c.format6, (int)c.format8);
    const auto format_of = [&](int32_t w) { return w == 4 ? DFQ_MX_E2M1 : (w == 6 ? c.format6 : c.format8); };
    bool candidate = false;
    for (int f = 0; f < c.n_widths; ++f) candidate |= c.widths[f] == c.num_bits;
    if (c.apply && !candidate) return fail_arg("%s: num_bits %d is none of the widths", me, (int)c.num_bits);
    if (!errors) return fail_arg("%s: null errors block", me);
    if (code_stride < 0 || scale_stride < 0) return fail_arg("%s: negative stride", me);
    std::vector<MxTensorDev> table;
    std::vector<int32_t> item_tensor;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_mx_tensor& t = tensors[i];
        if (t.code_offset >= 0 && !codes) return fail_arg("%s: tensor %d writes codes, but the code block is null", me, i);
        if (t.scale_offset >= 0 && !scales) return fail_arg("%s: tensor %d writes scales, but the scale block is null", me, i);
        MxTensorDev d;
        if (const int rc = mx_add_tensor(me, i, t.data, t.rows, t.row_len, t.code_offset, t.scale_offset, code_stride, scale_stride, item_tensor, d))
            return rc;
        table.push_back(d);
    }
    if (const int rc = mx_check_nets(me, bases, n_nets, (int64_t)item_tensor.size())) return rc;

    dfq_batch_mx_plan* p = new dfq_batch_mx_plan();
    MxArgs& a = p->args;
    a.errors = errors;
    a.codes = codes;
    a.scales = scales;
    a.code_stride = code_stride; a.scale_stride = scale_stride;
    a.items_pn = (int32_t)item_tensor.size();
    a.n_tensors = n_tensors;
    a.nf = c.n_widths;
    a.search = c.search ? 1 : 0;
    for (int f = 0; f < c.n_widths; ++f) { a.widths[f] = c.widths[f]; a.fmt[f] = format_of(c.widths[f]); }
    a.qfmt = candidate ? format_of(c.num_bits) : a.fmt[0];
    p->n_nets = n_nets;
    p->n_tensors = n_tensors;
    p->apply = c.apply ? 1 : 0;
    p->launches = 2 + p->apply;
    BatchUpload up{p->mem};
    a.tensors = up.put(table);
    a.item_tensor = up.put(item_tensor);
    a.delta = up.put(batch_delta(bases, n_nets));
    a.partial = (double*)up.raw(nullptr, sizeof(double) * (size_t)a.items_pn * (size_t)n_nets * (size_t)a.nf);
    p->widths.index = (const int32_t*)up.raw(nullptr, sizeof(int32_t) * (size_t)n_tensors);      // (filled by set_widths)
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch mx plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_mx_plan_run_stages(dfq_batch_mx_plan* p, int32_t stages, void* stream) {
    const char* me = "dfq_batch_mx_plan_run_stages";
    if (!p) return fail_arg("%s: null plan", me);
    if (stages == 0 || (stages & ~(DFQ_MX_ERRORS | DFQ_MX_QUANTISE))) return fail_arg("%s: stages %d", me, (int)stages);
    if (stages & DFQ_MX_ERRORS)
        if (const int rc = mx_run_errors(p, as_stream(stream))) return rc;
    if (stages & DFQ_MX_QUANTISE)
        if (const int rc = mx_run_quantise(p, as_stream(stream))) return rc;
    return DFQ_OK;
}

int dfq_batch_mx_plan_run(dfq_batch_mx_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_mx_plan_run: null plan");
    return dfq_batch_mx_plan_run_stages(p, DFQ_MX_ERRORS | (p->apply ? DFQ_MX_QUANTISE : 0), stream);
}

int dfq_batch_mx_plan_set_widths(dfq_batch_mx_plan* p, const int32_t* widths, int64_t width_stride, const int32_t* width_index,
                                 int32_t* status) {
    const char* me = "dfq_batch_mx_plan_set_widths";
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

int32_t dfq_batch_mx_decode_plan_launches(const dfq_batch_mx_decode_plan* p) { return p ? 1 : 0; }

void dfq_batch_mx_decode_plan_destroy(dfq_batch_mx_decode_plan* p) { batch_plan_destroy(p); }

int dfq_batch_mx_decode_plan_create(const dfq_batch_mx_decode_tensor* tensors, int32_t n_tensors, const void* const* bases,
                                    int32_t n_nets, const uint8_t* codes, int64_t code_stride, const uint8_t* scales,
                                    int64_t scale_stride, const int32_t* widths, int64_t width_stride, int32_t format6,
                                    int32_t format8, const int32_t* gate, int32_t* status, dfq_batch_mx_decode_plan** out_plan) {
    const char* me = "dfq_batch_mx_decode_plan_create";
    if (!tensors || n_tensors <= 0 || !out_plan) return fail_arg("%s: no tensors", me);
    if (!codes || !scales) return fail_arg("%s: null code or scale block", me);
    if (code_stride < 0 || scale_stride < 0) return fail_arg("%s: negative stride", me);
    if (!mx_format_fits(format6, format8)) return fail_arg("%s: format6 %d / format8 %d do not match their widths", me, (int)format6, (int)format8);
    std::vector<MxTensorDev> table;
    std::vector<int32_t> item_tensor;
    bool device_widths = false;
    for (int i = 0; i < n_tensors; ++i) {
        const dfq_batch_mx_decode_tensor& t = tensors[i];
        if (t.num_bits != 0 && t.num_bits != 4 && t.num_bits != 6 && t.num_bits != 8)
            return fail_arg("%s: tensor %d: num_bits %d is none of 0, 4, 6, 8", me, i, (int)t.num_bits);
        if (t.num_bits == 0) {
            if (!widths || !status) return fail_arg("%s: tensor %d reads its width on the device, but the width or status block is null", me, i);
            if (t.width_index < 0 || t.width_index >= width_stride)
                return fail_arg("%s: tensor %d: width_index %d outside [0, %lld)", me, i, (int)t.width_index, (long long)width_stride);
            device_widths = true;
        }
        if (t.code_offset < 0 || t.scale_offset < 0) return fail_arg("%s: tensor %d: negative offset", me, i);
        MxTensorDev d;
        if (const int rc = mx_add_tensor(me, i, t.data, t.rows, t.row_len, t.code_offset, t.scale_offset, code_stride, scale_stride, item_tensor, d))
            return rc;
        d.num_bits = t.num_bits;
        d.width_index = t.width_index;
        table.push_back(d);
    }
    if (const int rc = mx_check_nets(me, bases, n_nets, (int64_t)item_tensor.size())) return rc;

    dfq_batch_mx_decode_plan* p = new dfq_batch_mx_decode_plan();
    MxDecodeArgs& a = p->args;
    a.codes = codes;
    a.scales = scales;
    a.widths = widths;
    a.gate = gate;
    a.status = status;
    a.code_stride = code_stride; a.scale_stride = scale_stride; a.width_stride = width_stride;
    a.items_pn = (int32_t)item_tensor.size();
    a.format6 = format6; a.format8 = format8;
    p->n_nets = n_nets;
    p->device_widths = device_widths;
    BatchUpload up{p->mem};
    a.tensors = up.put(table);
    a.item_tensor = up.put(item_tensor);
    a.delta = up.put(batch_delta(bases, n_nets));
    if (up.err != hipSuccess) {
        batch_plan_destroy(p);
        return fail_hip(up.err, "batch mx decode plan allocation", __FILE__, __LINE__);
    }
    *out_plan = p;
    return DFQ_OK;
}

int dfq_batch_mx_decode_plan_run(dfq_batch_mx_decode_plan* p, void* stream) {
    if (!p) return fail_arg("dfq_batch_mx_decode_plan_run: null plan");
    const hipStream_t st = as_stream(stream);
    if (p->device_widths) DFQ_HIP_TRY(hipMemsetAsync(p->args.status, 0, sizeof(int32_t) * (size_t)p->n_nets, st));
    hipLaunchKernelGGL(mx_decode_kernel, dim3(p->args.items_pn * p->n_nets), dim3(kBlock), 0, st, p->args);
    DFQ_CHECK_LAUNCH();
    return DFQ_OK;
}

}  // extern "C"
