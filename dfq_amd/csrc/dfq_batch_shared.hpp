// Host side of what the batch plans share (dfq_quant_batch.hip, dfq_absorb_batch.hip, dfq_act_batch.hip): a plan holds the
// tables of network 0 in a DevSlab `mem` and finds network n's tensors bases[n] - bases[0] bytes further on.  Everything here
// has internal linkage (the library exports nothing for it).
#pragma once

#include "dfq_common.hpp"

namespace dfq {
namespace {

// the base addresses of a batch: DFQ_OK, or the argument error under the caller's name
inline int batch_check_bases(const char* me, const void* const* bases, int32_t n_nets) {
    if (!bases || n_nets <= 0) return fail_arg("%s: no networks (n_nets %d)", me, (int)n_nets);
    for (int n = 0; n < n_nets; ++n)
        if (!bases[n]) return fail_arg("%s: base address of network %d is null", me, n);
    return DFQ_OK;
}

// bases[n] - bases[0], bytes
inline std::vector<int64_t> batch_delta(const void* const* bases, int32_t n_nets) {
    std::vector<int64_t> delta(n_nets);
    for (int n = 0; n < n_nets; ++n) delta[n] = (int64_t)((uintptr_t)bases[n] - (uintptr_t)bases[0]);
    return delta;
}

// Host tables into a plan's DevSlab.  The first error is kept in `err` and nothing is tried after it; an empty table stays null.
struct BatchUpload {
    DevSlab& mem;
    hipError_t err = hipSuccess;
    void* raw(const void* h, size_t bytes) {               // h null: the allocation alone
        void* d = nullptr;
        if (err != hipSuccess || bytes == 0) return nullptr;
        if ((err = mem.alloc(&d, bytes)) == hipSuccess && h) err = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
        return d;
    }
    template <typename T>
    const T* put(const std::vector<T>& table) { return (const T*)raw(table.data(), sizeof(T) * table.size()); }
};

template <typename Plan>
void batch_plan_destroy(Plan* p) {
    if (!p) return;
    dev_quiesce();                                         // nothing in flight may still use the blocks released below
    p->mem.release();
    delete p;
}

}  // namespace
}  // namespace dfq
