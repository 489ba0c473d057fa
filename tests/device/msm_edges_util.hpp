// Shared by the two device test harnesses of the Pippenger pipeline, msm_edges.hip (sort, grouping, merge, segments, reduce, finish) and
// msm_slot_edges.hip (extended bases, slot sums and their fix-up kernels): device buffers with slack and a sentinel, the plan as 8 words, and the host
// checks every entry makes BEFORE it launches -- each size and each layout array that decides where a kernel reads or writes is verified against the
// buffers here, so that no input of a test can send a store or a load out of bounds (-1 = refused).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../ripp_amd/csrc/kernels.hpp"
#include "../../ripp_amd/csrc/fq_msm.hpp"
#include "../../ripp_amd/csrc/msm_batch.hpp"

#define MS_SENTINEL 0xA5C3F00Du          // twelve of these words are >= p on both curves: no stored coordinate looks like it
#define MS_SLACK 64                      // elements behind every output array
#define MS_CHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
#define MS_API extern "C" __attribute__((visibility("default")))

namespace msedge {
using namespace ripp;

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    hipError_t put(const void* host, size_t bytes) { const hipError_t e = alloc(bytes); return (e != hipSuccess || bytes == 0) ? e : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice); }
    hipError_t sentinel(size_t words) { const hipError_t e = alloc(words * 4); return (e != hipSuccess || words == 0) ? e : hipMemsetD32(p, (int)MS_SENTINEL, words); }
    hipError_t get(void* host, size_t bytes) const { return bytes ? hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
inline unsigned nblk(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }
inline MsmPlan plan_of(const uint32_t* w) { MsmPlan p; p.c = (int)w[0]; p.nwin = (int)w[1]; p.nb = w[2]; p.n = w[3]; p.ch = w[4]; p.seg = w[5]; p.nreal = w[6]; p.gmin = w[7]; return p; }

constexpr size_t MS_MAX_N = (size_t)1 << 16;          // terms
constexpr size_t MS_MAX_WIN = 4096;                   // (virtual) windows
constexpr size_t MS_MAX_ELEMS = (size_t)1 << 18;      // elements of any one array

// the plan members every kernel relies on; nwin may be a batch's virtual windows
inline bool plan_ok(const MsmPlan& p) {
    return p.c >= 4 && p.c <= 13 && p.nb == (1u << p.c) && p.nwin >= 1 && (size_t)p.nwin <= MS_MAX_WIN && p.n >= 1 && p.n <= MS_MAX_N && p.ch >= 1 && p.ch <= 65536 &&
           p.seg == 4 && p.gmin >= 1 && p.gmin <= 65536 && p.nreal >= 1 && p.nreal <= p.n && p.n % p.nreal == 0 && (p.n / p.nreal == 1 || p.n / p.nreal == 2 || p.n / p.nreal == 4) &&
           (size_t)p.nwin * p.nb <= MS_MAX_ELEMS && (size_t)p.nwin * p.n <= 4 * MS_MAX_ELEMS;
}
// slot_offs is the exclusive scan of ceil(hist / ch) in every window, slots_per_window its total, and every window's slots fit max_slots
inline bool layout_ok(const MsmPlan& p, const uint32_t* hist, const uint32_t* slot_offs, const uint32_t* spw, uint32_t max_slots) {
    if (max_slots == 0 || (size_t)p.nwin * max_slots > MS_MAX_ELEMS) return false;
    for (int w = 0; w < p.nwin; ++w) {
        uint64_t run = 0;
        for (uint32_t d = 0; d < p.nb; ++d) {
            const size_t k = (size_t)w * p.nb + d;
            if (slot_offs[k] != run) return false;
            run += ((uint64_t)hist[k] + p.ch - 1) / p.ch;
            if (run > max_slots) return false;
        }
        if (spw[w] != run) return false;
    }
    return true;
}
// offs is the exclusive scan of hist in every window, every run ends inside the window's row of `sorted`, and every index a slot gathers is a term
inline bool runs_ok(const MsmPlan& p, const uint32_t* hist, const uint32_t* offs, const uint32_t* sorted) {
    for (int w = 0; w < p.nwin; ++w) {
        uint64_t run = 0;
        for (uint32_t d = 0; d < p.nb; ++d) {
            const size_t k = (size_t)w * p.nb + d;
            if (offs[k] != run) return false;
            run += hist[k];
            if (run > p.n) return false;
        }
        for (uint64_t i = 0; i < run; ++i) if (sorted[(size_t)w * p.n + i] >= p.n) return false;
    }
    return true;
}
}  // namespace msedge
