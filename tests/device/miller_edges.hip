// Device test harness for stage 1 of the pairing product -- the three Miller-line kernels k_vm_miller_lines (vm.hpp), k_miller_lines_q (fq_miller.hpp)
// and k_miller_lines (kernels.hpp) -- and for the scalar dense tree k_fp12_tree (kernels.hpp).  It includes the production headers unchanged and
// launches the kernels with the geometry of Engine::enqueue_products / enqueue_stage2 (engine.hip); tests/test_gpu_miller_edges.py feeds it the point
// sets of tests/miller_edges.py and compares every stored line with the textbook formulas in Python integers.
//
// Built twice by tests/device/Makefile: libmiller_edges_381.so and libmiller_edges_377.so (-DRIPP_BLS12_377).  Every launcher takes HOST arrays, copies
// them to the device, runs one kernel, waits and copies the results back; it returns the HIP error code (0 = success, -1 = refused arguments).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../ripp_amd/csrc/vm.hpp"
#include "../../ripp_amd/csrc/fq_miller.hpp"

using namespace ripp;

#define ME_SENTINEL 0xA5C3F00Du          // twelve of these words are >= p on both curves: no stored coefficient looks like it

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    hipError_t put(const void* host, size_t bytes) { const hipError_t e = alloc(bytes); return (e != hipSuccess || bytes == 0) ? e : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice); }
    hipError_t get(void* host, size_t bytes) const { return bytes ? hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
#define ME_CHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
inline unsigned nblk(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }
constexpr uint32_t ME_MAX_M = 4096;
}  // namespace

static_assert(sizeof(G1A) == 96 && sizeof(G2A) == 192 && sizeof(Fp12) == 576, "struct sizes the Python side packs");
static_assert(4 * VM_EPW * VM_LINES_SLOTS * sizeof(VmSlot) <= 65536, "the VM kernel's workspace fits the LDS of one block");

extern "C" {
__attribute__((visibility("default"))) int me_curve() {
#if defined(RIPP_BLS12_377)
    return 377;
#else
    return 381;
#endif
}
__attribute__((visibility("default"))) int me_n_lines() { return N_LINES; }
__attribute__((visibility("default"))) int me_max_share() { return MAX_SHARE; }
__attribute__((visibility("default"))) uint32_t me_sentinel() { return ME_SENTINEL; }
// the SIMD count Engine::init derives the accumulator count of stage 2 from (4 per compute unit of the current device); -1 on a HIP error
__attribute__((visibility("default"))) int me_n_simd() {
    int dev = 0; hipDeviceProp_t pr;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) return -1;
    return pr.multiProcessorCount * 4;
}

// kind: 0 k_vm_miller_lines, 1 k_miller_lines_q, 2 k_miller_lines.  g1: n1 affine points of 24 words, g2: n2 of 48 words (the engine's Montgomery-384
// form, (0, 0) = infinity).  sets: nprod x (offset of the product's P vector in g1, offset of its Q vector in g2), M points each.  Kind 1 groups
// consecutive products over the same Q vector into chains of up to MAX_SHARE, as enqueue_products does; no_share != 0 gives every product its own chain.
// lines_out: the WHOLE buffer, nprod x N_LINES x 18 x stride chunks of 4 words, every word the sentinel before the launch.
__attribute__((visibility("default"))) int me_lines(int kind, const uint32_t* g1, uint32_t n1, const uint32_t* g2, uint32_t n2, const uint32_t* sets, int nprod,
                                                     uint32_t M, size_t stride, int no_share, uint32_t* lines_out) {
    if (kind < 0 || kind > 2 || nprod < 1 || nprod > MAX_PRODUCTS || M == 0 || M > ME_MAX_M || stride < M || stride > 2 * (size_t)ME_MAX_M) return -1;
    for (int p = 0; p < nprod; ++p)
        if ((uint64_t)sets[2 * p] + M > n1 || (uint64_t)sets[2 * p + 1] + M > n2) return -1;             // every vector inside its pool
    DevBuf d1, d2, dl;
    const size_t nrows = (size_t)nprod * N_LINES, words = nrows * LINE_CHUNKS * stride * 4;
    ME_CHK(d1.put(g1, (size_t)n1 * sizeof(G1A))); ME_CHK(d2.put(g2, (size_t)n2 * sizeof(G2A)));
    ME_CHK(dl.alloc(words * 4)); ME_CHK(hipMemsetD32(dl.p, (int)ME_SENTINEL, words));
    PairSets ps{};
    for (int p = 0; p < nprod; ++p) { ps.a[p] = d1.as<G1A>() + sets[2 * p]; ps.b[p] = d2.as<G2A>() + sets[2 * p + 1]; }
    const size_t m = M;
    if (kind == 0)
        hipLaunchKernelGGL(k_vm_miller_lines, dim3(nblk(m, 4 * VM_EPW), nprod), dim3(256), 4 * VM_EPW * VM_LINES_SLOTS * sizeof(VmSlot), 0, ps, (uint32_t)m, dl.as<uint4>(), stride);
    else if (kind == 1) {
        ChainSets cs{}; int ng = 0;
        for (int p = 0; p < nprod; ++p) {
            cs.a[p] = ps.a[p];
            if (!no_share && ng > 0 && ps.b[p] == cs.b[ng - 1] && cs.np[ng - 1] < MAX_SHARE) ++cs.np[ng - 1];
            else { cs.b[ng] = ps.b[p]; cs.first[ng] = (uint8_t)p; cs.np[ng] = 1; ++ng; }
        }
        hipLaunchKernelGGL(k_miller_lines_q, dim3(nblk(m, 256), ng), dim3(256), 0, 0, cs, (uint32_t)m, dl.as<uint4>(), stride);
    } else
        hipLaunchKernelGGL(k_miller_lines, dim3(nblk(m, 256), nprod), dim3(256), 0, 0, ps, (uint32_t)m, dl.as<uint4>(), stride);
    ME_CHK(hipGetLastError()); ME_CHK(hipDeviceSynchronize());
    ME_CHK(dl.get(lines_out, words * 4));
    return 0;
}

// k_fp12_tree with the engine's launch geometry: in = rows x 36 x Tin chunks of 16 bytes, out = rows x 36 x Tout, Tout = ceil(Tin / R), R = 2 or 4
__attribute__((visibility("default"))) int me_fp12_tree(const uint32_t* in, uint32_t Tin, uint32_t* out, uint32_t Tout, int R, uint32_t rows) {
    if (Tin == 0 || Tin > ME_MAX_M || rows == 0 || rows > 1024 || (R != 2 && R != 4) || Tout != (Tin + R - 1) / R) return -1;
    DevBuf din, dout;
    const size_t iw = (size_t)rows * FP12_CHUNKS * Tin * 4, ow = (size_t)rows * FP12_CHUNKS * Tout * 4;
    ME_CHK(din.put(in, iw * 4)); ME_CHK(dout.alloc(ow * 4)); ME_CHK(hipMemsetD32(dout.p, (int)ME_SENTINEL, ow));
    hipLaunchKernelGGL(k_fp12_tree, dim3(nblk(Tout, 64), (unsigned)rows), dim3(64), 0, 0, din.as<uint4>(), Tin, dout.as<uint4>(), Tout, R);
    ME_CHK(hipGetLastError()); ME_CHK(hipDeviceSynchronize());
    ME_CHK(dout.get(out, ow * 4));
    return 0;
}
}  // extern "C"
