// Device test harness for the lane-parallel field VM (vm.hpp: vm_run, vm_operand, vm_carry, vm_ld / vm_st, vm_put / vm_get), its compiled-in
// program tables (vm_programs.inc), the VmCurve<F> wrappers of msm.hpp and k_vm_fp12_tree.  It includes the production headers unchanged;
// tests/test_gpu_vm_edges.py feeds it tables and workspaces that tests/vm_model.py has checked against the interpreter's contract and compares
// every result bit for bit with that model.
//
// Built twice by tests/device/Makefile: libvm_edges_381.so and libvm_edges_377.so (-DRIPP_BLS12_377).  Every launcher takes HOST arrays, copies
// them to the device, runs one kernel, waits and copies the results back; it returns the HIP error code (0 = success, -1 = refused arguments).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../ripp_amd/csrc/vm.hpp"
#include "../../ripp_amd/csrc/msm.hpp"

using namespace ripp;

#define VE_GUARD_WORD(e, g, w) (0xC0DE0000u ^ ((uint32_t)(e) << 8) ^ ((uint32_t)(g) << 4) ^ (uint32_t)(w))

// ---- a table given at run time ---------------------------------------------------------------------------------------------------------------
// Launch shape of the engine's VM kernels: blockDim = 64 * waves, 4 groups of 16 lanes per wave, one element per group, the element's workspace
// at lds + e * (nslots + guard).  in: n x nslots x 14 limbs; out: n x nslots x 14 limbs (the final workspace through vm_ld, no fq_canon);
// gout: n x guard x 16 words (the slots behind the workspace, raw).
// FILL 0: the workspace is written (and read back) by all 16 lanes of the group, slot s by lane s mod 16, as k_vm_miller_lines and k_vm_fp12_tree
// write their inputs; FILL 1: by lane 0 alone, with the vm_run call outside any loop, as k_vm_scale_g1 calls its first doubling.
template <int FILL>
__global__ void __launch_bounds__(256) k_ve_run(const unsigned char* __restrict__ kind, const VmOp* __restrict__ ops, int nlayers, int nslots, int guard,
                                                 const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out, uint32_t* __restrict__ gout) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vm_smem[];
#if defined(__HIP_DEVICE_COMPILE__)
    VmSlot* const lds = reinterpret_cast<VmSlot*>(vm_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane & (VM_G - 1), grp = lane / VM_G;
    const uint32_t e = (blockIdx.x * (blockDim.x >> 6) + wave) * VM_EPW + grp;
    VmSlot* const ws = lds + (size_t)(wave * VM_EPW + grp) * (nslots + guard);
    const bool active = e < n;
    const int step = FILL == 0 ? VM_G : 1;
    if (FILL == 0 || lg == 0) {
        for (int s = (FILL == 0 ? lg : 0); s < nslots; s += step) {
            VmVal v;
            for (int i = 0; i < fq28::NL; ++i) v.l[i] = active ? in[((size_t)e * nslots + s) * 14 + i] : 0u;      // idle groups run on zeros
            vm_st(ws, s, v);
        }
        for (int g = (FILL == 0 ? lg : 0); g < guard; g += step)
            for (int w = 0; w < 16; ++w) ws[nslots + g].l[w] = VE_GUARD_WORD(e & 0xFFu, g, w);
    }
    vm_run(ws, kind, ops, nlayers, lg);
    if (active && (FILL == 0 || lg == 0)) {
        for (int s = (FILL == 0 ? lg : 0); s < nslots; s += step) {
            const VmVal v = vm_ld(ws, s);
            for (int i = 0; i < fq28::NL; ++i) out[((size_t)e * nslots + s) * 14 + i] = v.l[i];
        }
        for (int g = (FILL == 0 ? lg : 0); g < guard; g += step)
            for (int w = 0; w < 16; ++w) gout[((size_t)e * guard + g) * 16 + w] = ws[nslots + g].l[w];
    }
#endif
}

// ---- the compiled-in production tables -------------------------------------------------------------------------------------------------------------
#define VE_PROGS(X) X(0, fp12_mul_g16) X(1, g1_cadd_g16) X(2, g1_hdbl_g16) X(3, g2_cadd_g16) X(4, g2_hdbl_g16) X(5, line_add_g16) X(6, line_double_g16)
// hdr: nlayers, nslots, number of inputs, number of outputs; kind: nlayers bytes; ops: 16 nlayers records; io: the _in then the _out slot numbers
__global__ void k_ve_export(int prog, int* hdr, unsigned char* kind, VmOp* ops, unsigned char* io) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    namespace vp = vmprog;
#define X(ID, T)                                                                                                       \
    if (prog == ID) {                                                                                                  \
        const int ni = (int)sizeof(vp::T##_in), no = (int)sizeof(vp::T##_out);                                         \
        hdr[0] = vp::T##_nlayers; hdr[1] = vp::T##_nslots; hdr[2] = ni; hdr[3] = no;                                   \
        for (int i = 0; i < vp::T##_nlayers; ++i) kind[i] = vp::T##_kind[i];                                           \
        for (int i = 0; i < vp::T##_nlayers * VM_G; ++i) ops[i] = vp::T##_ops[i];                                      \
        for (int i = 0; i < ni; ++i) io[i] = vp::T##_in[i];                                                            \
        for (int i = 0; i < no; ++i) io[ni + i] = vp::T##_out[i];                                                      \
    }
    VE_PROGS(X)
#undef X
#endif
}

// ---- VmCurve<F>: put -> a list of dbl_ / add_ steps -> get, on engine-format values ------------------------------------------------------------
// in: per element T = (X, Y, Z) then Q = (X, Y, Z), NF x 12 words per coordinate; steps: 0 = dbl_, 1 = add_ of Q (the addend slots are rewritten
// before every addition, as every caller does: the programs use them as scratch); out: T, canonical.  Lane 0 of the group writes and reads.
template <class F>
__global__ void __launch_bounds__(256) k_ve_curve(const uint32_t* __restrict__ in, const unsigned char* __restrict__ steps, int nsteps, uint32_t n, uint32_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vm_smem[];
#if defined(__HIP_DEVICE_COMPILE__)
    using C = VmCurve<F>;
    constexpr int CW = 12 * C::NF;
    VmSlot* const lds = reinterpret_cast<VmSlot*>(vm_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane & (VM_G - 1), grp = lane / VM_G;
    const uint32_t e = (blockIdx.x * 4 + wave) * VM_EPW + grp;
    VmSlot* const ws = lds + (size_t)(wave * VM_EPW + grp) * C::SLOTS;
    const bool active = e < n;
    F t[3], q[3];
    t[0] = F::zero(); t[1] = F::one(); t[2] = F::zero(); q[0] = F::zero(); q[1] = F::one(); q[2] = F::zero();      // idle groups: the identity
    if (active && lg == 0) {
        for (int k = 0; k < 3; ++k) {
            uint32_t* tw = reinterpret_cast<uint32_t*>(&t[k]); uint32_t* qw = reinterpret_cast<uint32_t*>(&q[k]);
            for (int w = 0; w < CW; ++w) { tw[w] = in[((size_t)e * 6 + k) * CW + w]; qw[w] = in[((size_t)e * 6 + 3 + k) * CW + w]; }
        }
    }
    if (lg == 0) {
        for (int s = 0; s < C::SLOTS; ++s) vm_st(ws, s, fq_zero());            // a defined workspace: the model starts from zeros as well
        C::put(ws, C::SX, t[0]); C::put(ws, C::SY, t[1]); C::put(ws, C::SZ, t[2]);
    }
#pragma unroll 1
    for (int k = 0; k < nsteps; ++k) {
        if (steps[k] == 0) C::dbl_(ws, lg);
        else {
            if (lg == 0) { C::put(ws, C::QX, q[0]); C::put(ws, C::QY, q[1]); C::put(ws, C::QZ, q[2]); }
            C::add_(ws, lg);
        }
    }
    if (active && lg == 0) {
        const F r[3] = {C::get(ws, C::SX), C::get(ws, C::SY), C::get(ws, C::SZ)};
        for (int k = 0; k < 3; ++k) {
            const uint32_t* rw = reinterpret_cast<const uint32_t*>(&r[k]);
            for (int w = 0; w < CW; ++w) out[((size_t)e * 3 + k) * CW + w] = rw[w];
        }
    }
#endif
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    hipError_t put(const void* host, size_t bytes) { const hipError_t e = alloc(bytes); return (e != hipSuccess || bytes == 0) ? e : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice); }
    hipError_t get(void* host, size_t bytes) const { return bytes ? hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
#define VE_CHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
constexpr size_t VE_LDS_MAX = 65536;             // what every engine launch stays within
}  // namespace

static_assert(sizeof(VmOp) == 36 && sizeof(VmSlot) == 64, "record sizes the Python side packs");

extern "C" {
__attribute__((visibility("default"))) int ve_curve() {
#if defined(RIPP_BLS12_377)
    return 377;
#else
    return 381;
#endif
}
__attribute__((visibility("default"))) int ve_curve_slots(int g2) { return g2 ? VmCurve<Fp2>::SLOTS : VmCurve<Fp>::SLOTS; }
__attribute__((visibility("default"))) int ve_f12_slots() { return VM_F12_SLOTS; }

// kind: nlayers bytes; ops: 16 nlayers records of 36 bytes; in / out: n x nslots x 14; gout: n x guard x 16; fill 0 / 1; waves per block 1..4
__attribute__((visibility("default"))) int ve_run_table(const unsigned char* kind, const unsigned char* ops, int nlayers, int nslots, int guard, int fill, int waves,
                                                         const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* gout) {
    if (nlayers < 0 || nslots < 2 || nslots > 255 || guard < 0 || guard > 16 || (fill != 0 && fill != 1) || waves < 1 || waves > 4 || n == 0) return -1;
    const size_t lds = (size_t)waves * VM_EPW * (size_t)(nslots + guard) * sizeof(VmSlot);
    if (lds > VE_LDS_MAX) return -1;
    for (int i = 0; i < nlayers * VM_G; ++i) {          // every slot index of the table inside the workspace
        const unsigned char* o = ops + (size_t)i * sizeof(VmOp);
        if (o[0] >= nslots) return -1;
        for (int t = 0; t < 16; ++t) if (o[4 + t] >= nslots) return -1;
    }
    DevBuf dk, dops, din, dout, dg;
    const size_t wsw = (size_t)n * nslots * 14, gw = (size_t)n * guard * 16;
    VE_CHK(dk.put(kind, (size_t)nlayers)); VE_CHK(dops.put(ops, (size_t)nlayers * VM_G * sizeof(VmOp))); VE_CHK(din.put(in, wsw * 4));
    VE_CHK(dout.alloc(wsw * 4)); VE_CHK(hipMemset(dout.p, 0xA5, wsw * 4)); VE_CHK(dg.alloc(gw * 4)); VE_CHK(hipMemset(dg.p, 0xA5, gw ? gw * 4 : 16));
    const dim3 grid((n + waves * VM_EPW - 1) / (waves * VM_EPW)), block(64 * waves);
    if (fill == 0) hipLaunchKernelGGL(k_ve_run<0>, grid, block, lds, 0, dk.as<unsigned char>(), dops.as<VmOp>(), nlayers, nslots, guard, din.as<uint32_t>(), n, dout.as<uint32_t>(), dg.as<uint32_t>());
    else hipLaunchKernelGGL(k_ve_run<1>, grid, block, lds, 0, dk.as<unsigned char>(), dops.as<VmOp>(), nlayers, nslots, guard, din.as<uint32_t>(), n, dout.as<uint32_t>(), dg.as<uint32_t>());
    VE_CHK(hipGetLastError()); VE_CHK(hipDeviceSynchronize());
    VE_CHK(dout.get(out, wsw * 4)); VE_CHK(dg.get(gout, gw * 4));
    return 0;
}
// the word the kernel writes at word w of guard slot g behind element e
__attribute__((visibility("default"))) uint32_t ve_guard_word(uint32_t e, int g, int w) { return VE_GUARD_WORD(e & 0xFFu, g, w); }

// prog: 0 fp12_mul, 1 g1_cadd, 2 g1_hdbl, 3 g2_cadd, 4 g2_hdbl, 5 line_add, 6 line_double.  hdr: 4 ints; kind: >= 64 bytes; ops: >= 64 x 16 records; io: >= 64 bytes
__attribute__((visibility("default"))) int ve_export(int prog, int* hdr, unsigned char* kind, unsigned char* ops, unsigned char* io) {
    if (prog < 0 || prog > 6) return -1;
    int nl = 0, ni = 0, no = 0;
    namespace vp = vmprog;
#define X(ID, T) if (prog == ID) { nl = vp::T##_nlayers; ni = (int)sizeof(vp::T##_in); no = (int)sizeof(vp::T##_out); }
    VE_PROGS(X)
#undef X
    if (nl > 64 || ni + no > 64) return -1;
    DevBuf dh, dk, dops, dio;
    VE_CHK(dh.alloc(16)); VE_CHK(dk.alloc(64)); VE_CHK(dops.alloc((size_t)64 * VM_G * sizeof(VmOp))); VE_CHK(dio.alloc(64));
    hipLaunchKernelGGL(k_ve_export, dim3(1), dim3(64), 0, 0, prog, dh.as<int>(), dk.as<unsigned char>(), dops.as<VmOp>(), dio.as<unsigned char>());
    VE_CHK(hipGetLastError()); VE_CHK(hipDeviceSynchronize());
    VE_CHK(dh.get(hdr, 16)); VE_CHK(dk.get(kind, (size_t)nl)); VE_CHK(dops.get(ops, (size_t)nl * VM_G * sizeof(VmOp))); VE_CHK(dio.get(io, (size_t)(ni + no)));
    return 0;
}

// in: n x 6 x (12 NF) words, steps: nsteps bytes, out: n x 3 x (12 NF) words
__attribute__((visibility("default"))) int ve_curve_seq(int g2, const uint32_t* in, const unsigned char* steps, int nsteps, uint32_t n, uint32_t* out) {
    if (n == 0 || nsteps < 0) return -1;
    for (int k = 0; k < nsteps; ++k) if (steps[k] > 1) return -1;
    const size_t cw = g2 ? 24 : 12;
    DevBuf din, ds, dout;
    VE_CHK(din.put(in, (size_t)n * 6 * cw * 4)); VE_CHK(ds.put(steps, (size_t)nsteps)); VE_CHK(dout.alloc((size_t)n * 3 * cw * 4)); VE_CHK(hipMemset(dout.p, 0xA5, (size_t)n * 3 * cw * 4));
    const dim3 grid((n + 4 * VM_EPW - 1) / (4 * VM_EPW)), block(256);
    if (g2) hipLaunchKernelGGL(k_ve_curve<Fp2>, grid, block, 4 * VM_EPW * VmCurve<Fp2>::SLOTS * sizeof(VmSlot), 0, din.as<uint32_t>(), ds.as<unsigned char>(), nsteps, n, dout.as<uint32_t>());
    else hipLaunchKernelGGL(k_ve_curve<Fp>, grid, block, 4 * VM_EPW * VmCurve<Fp>::SLOTS * sizeof(VmSlot), 0, din.as<uint32_t>(), ds.as<unsigned char>(), nsteps, n, dout.as<uint32_t>());
    VE_CHK(hipGetLastError()); VE_CHK(hipDeviceSynchronize());
    VE_CHK(dout.get(out, (size_t)n * 3 * cw * 4));
    return 0;
}

// k_vm_fp12_tree with the engine's launch geometry (engine.hip): in = rows x 36 x Tin chunks of 16 bytes, out = rows x 36 x Tout
__attribute__((visibility("default"))) int ve_fp12_tree(const uint32_t* in, uint32_t Tin, uint32_t* out, uint32_t Tout, uint32_t rows) {
    if (Tin == 0 || rows == 0 || Tout != (Tin + 1) / 2) return -1;
    DevBuf din, dout;
    const size_t iw = (size_t)rows * FP12_CHUNKS * Tin * 4, ow = (size_t)rows * FP12_CHUNKS * Tout * 4;
    VE_CHK(din.put(in, iw * 4)); VE_CHK(dout.alloc(ow * 4)); VE_CHK(hipMemset(dout.p, 0xA5, ow * 4));
    hipLaunchKernelGGL(k_vm_fp12_tree, dim3((Tout + 2 * VM_EPW - 1) / (2 * VM_EPW), rows), dim3(128), 2 * VM_EPW * VM_F12_SLOTS * sizeof(VmSlot), 0,
                       din.as<uint4>(), Tin, dout.as<uint4>(), Tout);
    VE_CHK(hipGetLastError()); VE_CHK(hipDeviceSynchronize());
    VE_CHK(dout.get(out, ow * 4));
    return 0;
}
}  // extern "C"
