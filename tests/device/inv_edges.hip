// Device test harness for the field inversion (bls12_381/fp_inv.hpp: fp_inv_bingcd, fp_inv_kaliski, finv), the Fp2 inverse built on it (tower.hpp), the
// single-point to_affine (curve.hpp) and the batch normalisation k_normalize<F> (kernels.hpp).  It includes the production headers unchanged;
// tests/test_gpu_inv_edges.py feeds it the edge list of tests/inv_edges.py and chains with points at infinity at chosen places and compares every
// result with Python integers.
//
// Built twice by tests/device/Makefile: libinv_edges_381.so and libinv_edges_377.so (-DRIPP_BLS12_377).  Every launcher takes HOST arrays, copies
// them to the device, runs one kernel, waits and copies the results back; it returns the HIP error code (0 = success, -1 = refused arguments).
// All values are the engine's: 12 words per Fp (Montgomery form, radix 2^384), Fp2 = (c0, c1), Jacobian (X, Y, Z), affine (x, y).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../ripp_amd/csrc/kernels.hpp"

using namespace ripp;

// one lane per case.  WHICH 0: fp_inv_bingcd, 1: fp_inv_kaliski (its loop leaves when no lane of the WAVE is live), 2: finv, what the kernels call
template <int WHICH>
__global__ void __launch_bounds__(256) k_ie_fp_inv(const Fp* __restrict__ in, uint32_t n, Fp* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
    const Fp y = in[i];
    out[i] = WHICH == 0 ? fp_inv_bingcd(y) : WHICH == 1 ? fp_inv_kaliski(y) : finv(y);
#endif
}
__global__ void __launch_bounds__(256) k_ie_fp2_inv(const Fp2* __restrict__ in, uint32_t n, Fp2* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
    out[i] = finv(in[i]);
#endif
}
template <class F>
__global__ void __launch_bounds__(256) k_ie_to_affine(const Jac<F>* __restrict__ in, uint32_t n, Affine<F>* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
    out[i] = to_affine(in[i]);
#endif
}

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    hipError_t put(const void* host, size_t bytes) { const hipError_t e = alloc(bytes); return (e != hipSuccess || bytes == 0) ? e : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice); }
    hipError_t get(void* host, size_t bytes) const { return bytes ? hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
#define IE_CHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
constexpr uint32_t IE_MAX_N = 1u << 24;
inline dim3 ie_grid(uint32_t n, uint32_t block) { return dim3((n + block - 1) / block); }
}  // namespace

static_assert(sizeof(Fp) == 48 && sizeof(Fp2) == 96 && sizeof(G1J) == 144 && sizeof(G2J) == 288 && sizeof(G1A) == 96 && sizeof(G2A) == 192, "the layouts the Python side packs");

extern "C" {
__attribute__((visibility("default"))) int ie_curve() {
#if defined(RIPP_BLS12_377)
    return 377;
#else
    return 381;
#endif
}

// in / out: n x 12 words.  which 0 fp_inv_bingcd, 1 fp_inv_kaliski, 2 finv; block 64 or 256
__attribute__((visibility("default"))) int ie_fp_inv(int which, const uint32_t* in, uint32_t n, int block, uint32_t* out) {
    if (which < 0 || which > 2 || n == 0 || n > IE_MAX_N || (block != 64 && block != 256)) return -1;
    DevBuf din, dout;
    const size_t bytes = (size_t)n * sizeof(Fp);
    IE_CHK(din.put(in, bytes)); IE_CHK(dout.alloc(bytes)); IE_CHK(hipMemset(dout.p, 0xA5, bytes));
    const dim3 grid = ie_grid(n, (uint32_t)block), blk((uint32_t)block);
    if (which == 0) hipLaunchKernelGGL(k_ie_fp_inv<0>, grid, blk, 0, 0, din.as<Fp>(), n, dout.as<Fp>());
    else if (which == 1) hipLaunchKernelGGL(k_ie_fp_inv<1>, grid, blk, 0, 0, din.as<Fp>(), n, dout.as<Fp>());
    else hipLaunchKernelGGL(k_ie_fp_inv<2>, grid, blk, 0, 0, din.as<Fp>(), n, dout.as<Fp>());
    IE_CHK(hipGetLastError()); IE_CHK(hipDeviceSynchronize());
    IE_CHK(dout.get(out, bytes));
    return 0;
}

// in / out: n x 24 words: the device finv(Fp2)
__attribute__((visibility("default"))) int ie_fp2_inv(const uint32_t* in, uint32_t n, uint32_t* out) {
    if (n == 0 || n > IE_MAX_N) return -1;
    DevBuf din, dout;
    const size_t bytes = (size_t)n * sizeof(Fp2);
    IE_CHK(din.put(in, bytes)); IE_CHK(dout.alloc(bytes)); IE_CHK(hipMemset(dout.p, 0xA5, bytes));
    hipLaunchKernelGGL(k_ie_fp2_inv, ie_grid(n, 256), dim3(256), 0, 0, din.as<Fp2>(), n, dout.as<Fp2>());
    IE_CHK(hipGetLastError()); IE_CHK(hipDeviceSynchronize());
    IE_CHK(dout.get(out, bytes));
    return 0;
}

// k_normalize<Fp> (g2 = 0) / k_normalize<Fp2> (g2 = 1) with the engine's launch geometry (engine.hip::normalize_dev) and the caller's T lanes:
// in: n Jacobian points, out: n affine points, separate buffers; 1 <= T <= n
__attribute__((visibility("default"))) int ie_normalize(int g2, const uint32_t* in, uint32_t n, uint32_t T, uint32_t* out) {
    if (n == 0 || n > IE_MAX_N || T < 1 || T > n) return -1;
    DevBuf din, dout;
    const size_t ib = (size_t)n * (g2 ? sizeof(G2J) : sizeof(G1J)), ob = (size_t)n * (g2 ? sizeof(G2A) : sizeof(G1A));
    IE_CHK(din.put(in, ib)); IE_CHK(dout.alloc(ob)); IE_CHK(hipMemset(dout.p, 0xA5, ob));
    if (g2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_normalize<Fp2>), ie_grid(T, 256), dim3(256), 0, 0, din.as<G2J>(), n, dout.as<G2A>(), T);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_normalize<Fp>), ie_grid(T, 256), dim3(256), 0, 0, din.as<G1J>(), n, dout.as<G1A>(), T);
    IE_CHK(hipGetLastError()); IE_CHK(hipDeviceSynchronize());
    IE_CHK(dout.get(out, ob));
    return 0;
}

// the device to_affine, one lane per point
__attribute__((visibility("default"))) int ie_to_affine(int g2, const uint32_t* in, uint32_t n, uint32_t* out) {
    if (n == 0 || n > IE_MAX_N) return -1;
    DevBuf din, dout;
    const size_t ib = (size_t)n * (g2 ? sizeof(G2J) : sizeof(G1J)), ob = (size_t)n * (g2 ? sizeof(G2A) : sizeof(G1A));
    IE_CHK(din.put(in, ib)); IE_CHK(dout.alloc(ob)); IE_CHK(hipMemset(dout.p, 0xA5, ob));
    if (g2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ie_to_affine<Fp2>), ie_grid(n, 256), dim3(256), 0, 0, din.as<G2J>(), n, dout.as<G2A>());
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ie_to_affine<Fp>), ie_grid(n, 256), dim3(256), 0, 0, din.as<G1J>(), n, dout.as<G1A>());
    IE_CHK(hipGetLastError()); IE_CHK(hipDeviceSynchronize());
    IE_CHK(dout.get(out, ob));
    return 0;
}
}  // extern "C"
