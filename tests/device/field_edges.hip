// Device test harness for the carry-free field arithmetic (fq28.hpp), its group law (fq_curve.hpp, fq_curve2.hpp) and stage 2 of the pairing
// product (fq_line_products.hpp, fq_line_products_k.hpp).  It includes the production headers unchanged and runs their primitives at fixed type
// instantiations, one lane per test case, over arrays of raw limbs; tests/test_gpu_field_edges.py feeds it values at the bounds each type admits
// (tests/field_edges.py builds them) and checks the results against Python integers.
//
// Built twice by tests/device/Makefile: libfield_edges_381.so and libfield_edges_377.so (-DRIPP_BLS12_377).  Every launcher takes HOST arrays,
// copies them to the device, runs one kernel, waits and copies the results back; it returns the HIP error code (0 = success).
//
// The instantiation tables below (FE_*_LIST) are mirrored in tests/field_edges.py; the fe_*_bounds exports let the GPU test check the two agree.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <initializer_list>
#include "../../ripp_amd/csrc/fq28.hpp"
#include "../../ripp_amd/csrc/fq_curve.hpp"
#include "../../ripp_amd/csrc/fq_curve2.hpp"
#include "../../ripp_amd/csrc/fq_line_products.hpp"
#include "../../ripp_amd/csrc/fq_line_products_k.hpp"

using namespace ripp;

#define FE_L28 ((uint64_t)1 << 28)
#define FE_LWIDE (((uint64_t)1 << 32) - 16)            // the widest limb bound fq_norm accepts

// ---- instantiation tables: (id, limb bound, value bound) of every operand --------------------------------------------------------------------
// tests/field_edges.py names the engine call site each entry mirrors: an engine type that widens needs its entry widened here and there.
// fq_reduce / fq_norm: the code does not depend on the bounds (they are static checks only); each engine bound still gets its own instantiation
#define FE_REDUCE_LIST(X)                                                                                                             \
    X(0, FE_L28, 4) X(1, FE_L28, 8) X(2, FE_L28, 19) X(3, FE_L28, 36) X(4, FE_L28, 256) X(5, ((uint64_t)1 << 29), 258)                 \
    X(6, FE_L28, 7) X(7, FE_L28, 11) X(8, FE_L28, 14) X(9, FE_L28, 44) X(10, FE_LWIDE, 2500)
// fq_sub / fq_neg: the bias K = (V2 + 1) p depends on the subtrahend's type (L2, V2); the minuend is 0 of type Fq<1, 1>
#define FE_SUB_LIST(X)                                                                                                                \
    X(0, FE_L28, 2) X(1, FE_L28, 4) X(2, FE_L28, 8) X(3, FE_L28, 11) X(4, FE_L28, 16) X(5, FE_L28, 19) X(6, FE_L28, 36)               \
    X(7, FE_L28, 256) X(8, 8 * (FE_L28 - 1) + 1, 16) X(9, ((uint64_t)1 << 29) - 1, 38) X(10, 5 * (FE_L28 - 1) + 1, 20)                 \
    X(11, 4 * (FE_L28 - 1) + 1, 8) X(12, 5 * (((uint64_t)1 << 29) - 2) + 1, 40) X(13, 14 * FE_L28 - 13, 1000)
// fq_mul (L1, V1) x (L2, V2)
#define FE_MUL_LIST(X)                                                                                                                \
    X(0, FE_L28, 2, FE_L28, 2) X(1, FE_L28, 256, FE_L28, 2) X(2, ((uint64_t)1 << 29), 258, FE_L28, 8)                                 \
    X(3, 4 * (FE_L28 - 1) + 1, 8, FE_L28, 39) X(4, 3 * (FE_L28 - 1) + 1, 6, 3 * FE_L28 - 1, 53) X(5, FE_L28, 19, FE_L28, 8)             \
    X(6, FE_L28, 36, 4 * (FE_L28 - 1) + 1, 8) X(7, 4 * (FE_L28 - 1) + 1, 8, 4 * (FE_L28 - 1) + 1, 8) X(8, FE_L28, 1250, FE_L28, 2)
// fq_sqr (L1, V1): the doubled limbs must fit 32 bits
#define FE_SQR_LIST(X)                                                                                                                \
    X(0, FE_L28, 2) X(1, FE_L28, 36) X(2, ((uint64_t)1 << 29) - 1, 38) X(3, 3 * (FE_L28 - 1) + 1, 6) X(4, FE_L28, 44)                 \
    X(5, ((uint64_t)1 << 29) - 1, 47) X(6, FE_L28, 50) X(7, 4 * (FE_L28 - 1) + 1, 8)
// fq_dot<2> and fq_dot<4>: every a[t] of type (L1, V1), every b[t] of type (L2, V2)
#define FE_DOT2_LIST(X) X(0, 3 * FE_L28, 44, FE_L28, 14) X(1, ((uint64_t)1 << 29) - 1, 8, ((uint64_t)1 << 29) - 1, 8) X(2, FE_L28, 625, FE_L28, 2)
#define FE_DOT4_LIST(X) X(0, 3 * FE_L28, 22, FE_L28, 14) X(1, FE_L28, 312, FE_L28, 2)
// fq_mul_sub(a, b, c, d) = a b - c d: (La, Va) (Lb, Vb) (Lc, Vc) (Ld, Vd)
#define FE_MULSUB_LIST(X) X(0, FE_L28, 44, FE_L28, 14, ((uint64_t)1 << 29) - 1, 38, FE_L28, 2) X(1, FE_L28, 2, FE_L28, 2, FE_L28, 2, FE_L28, 2)
// Fp2 products (both parts of an operand of the same type)
#if defined(RIPP_BLS12_377)
#define FE_F2MUL_LIST(X)                                                                                                              \
    X(0, FE_L28, 2, FE_L28, 2) X(1, 4 * (FE_L28 - 1) + 1, 8, FE_L28, 2) X(2, FE_L28, 4, 4 * (FE_L28 - 1) + 1, 8)                      \
    X(3, FE_L28, 4, FE_L28, 14) X(4, 8 * (FE_L28 - 1) + 1, 16, FE_L28, 2)
#define FE_F2SQR_LIST(X) X(0, FE_L28, 2) X(1, FE_L28, 4) X(2, FE_L28, 6) X(3, FE_L28, 12)
#else
#define FE_F2MUL_LIST(X)                                                                                                              \
    X(0, FE_L28, 2, FE_L28, 2) X(1, FE_L28, 256, FE_L28, 2) X(2, ((uint64_t)1 << 29), 258, FE_L28, 2) X(3, FE_L28, 14, 4 * (FE_L28 - 1) + 1, 8) \
    X(4, FE_L28, 11, 4 * (FE_L28 - 1) + 1, 8) X(5, FE_L28, 6, FE_L28, 19) X(6, FE_L28, 7, FE_L28, 8)
#define FE_F2SQR_LIST(X) X(0, FE_L28, 2) X(1, FE_L28, 11) X(2, FE_L28, 7) X(3, FE_L28, 13) X(4, FE_L28, 22) X(5, FE_L28, 20) X(6, FE_L28, 8)
#define FE_F2MULSUB_LIST(X) X(0, FE_L28, 20, FE_L28, 14, ((uint64_t)1 << 29) - 1, 4, FE_L28, 7)
#endif
// f2_mul_fq (Fp2 operand (L1, V1), Fp operand (L2, V2))
#define FE_F2MULFQ_LIST(X) X(0, FE_L28, 2, FE_L28, 2) X(1, FE_L28, 4, FE_L28, 256) X(2, 3 * (FE_L28 - 1) + 1, 6, FE_L28, 4)

#define FE_COUNT(...) +1
#define FE_N(LIST) (0 LIST(FE_COUNT))

// ---- device helpers ---------------------------------------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
template <class T> __device__ __forceinline__ T fe_ld(const uint32_t* s) { T v; for (int i = 0; i < fq28::NL; ++i) v.l[i] = s[i]; return v; }
template <class T> __device__ __forceinline__ void fe_st(uint32_t* d, const T& v) { for (int i = 0; i < fq28::NL; ++i) d[i] = v.l[i]; }
template <class T> __device__ __forceinline__ T fe_ld2(const uint32_t* s) { T v; v.c0 = fe_ld<decltype(v.c0)>(s); v.c1 = fe_ld<decltype(v.c1)>(s + fq28::NL); return v; }
template <class T> __device__ __forceinline__ void fe_st2(uint32_t* d, const T& v) { fe_st(d, v.c0); fe_st(d + fq28::NL, v.c1); }
#endif
#define FE_LANE const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;

// out[14]: fq_reduce(a); flag: fq_is_zero of the result
template <uint64_t LM, int VB> __global__ void k_reduce(const uint32_t* in, uint32_t* out, uint32_t* flag, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    const Fqn r = fq_reduce(fe_ld<Fq<LM, VB>>(in + (size_t)i * 14));
    fe_st(out + (size_t)i * 14, r);
    flag[i] = fq_is_zero(r) ? 1u : 0u;
#endif
}
template <uint64_t LM, int VB> __global__ void k_norm(const uint32_t* in, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    fe_st(out + (size_t)i * 14, fq_norm(fe_ld<Fq<LM, VB>>(in + (size_t)i * 14)));
#endif
}
// out[0..13]: fq_neg(b); out[14..27]: fq_sub(0 as Fqn, b); out[28..55]: f2_sub(0, (b, b))
template <uint64_t L2, int V2> __global__ void k_sub(const uint32_t* in, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    using T = Fq<L2, V2>;
    const T b = fe_ld<T>(in + (size_t)i * 14);
    uint32_t* o = out + (size_t)i * 56;
    fe_st(o, fq_neg(b));
    fe_st(o + 14, fq_sub(fq_zero(), b));
    fe_st2(o + 28, f2_sub(Fq2n{fq_zero(), fq_zero()}, Fq2T<L2, V2>{b, b}));
#endif
}
// flag: fq_is_zero of a reduced value as given; out: fq_canon of it
__global__ void k_canon(const uint32_t* in, uint32_t* out, uint32_t* flag, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    const Fqn a = fe_ld<Fqn>(in + (size_t)i * 14);
    fe_st(out + (size_t)i * 14, fq_canon(a));
    flag[i] = fq_is_zero(a) ? 1u : 0u;
#endif
}
template <uint64_t L1, int V1, uint64_t L2, int V2> __global__ void k_mul(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    fe_st(out + (size_t)i * 14, fq_mul(fe_ld<Fq<L1, V1>>(a + (size_t)i * 14), fe_ld<Fq<L2, V2>>(b + (size_t)i * 14)));
#endif
}
template <uint64_t L1, int V1> __global__ void k_sqr(const uint32_t* a, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    fe_st(out + (size_t)i * 14, fq_sqr(fe_ld<Fq<L1, V1>>(a + (size_t)i * 14)));
#endif
}
template <int NT, uint64_t L1, int V1, uint64_t L2, int V2> __global__ void k_dot(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    Fq<L1, V1> aa[NT]; Fq<L2, V2> bb[NT];
    for (int t = 0; t < NT; ++t) { aa[t] = fe_ld<Fq<L1, V1>>(a + ((size_t)i * NT + t) * 14); bb[t] = fe_ld<Fq<L2, V2>>(b + ((size_t)i * NT + t) * 14); }
    fe_st(out + (size_t)i * 14, fq_dot<NT>(aa, bb));
#endif
}
// in: a, b, c, d (14 limbs each, per case)
template <uint64_t LA, int VA, uint64_t LB, int VB_, uint64_t LC, int VC, uint64_t LD, int VD> __global__ void k_mul_sub(const uint32_t* in, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t* s = in + (size_t)i * 56;
    fe_st(out + (size_t)i * 14, fq_mul_sub(fe_ld<Fq<LA, VA>>(s), fe_ld<Fq<LB, VB_>>(s + 14), fe_ld<Fq<LC, VC>>(s + 28), fe_ld<Fq<LD, VD>>(s + 42)));
#endif
}
// f2_muld(a, b): a, b as (c0, c1), 28 limbs each
template <uint64_t L1, int V1, uint64_t L2, int V2> __global__ void k_f2mul(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    fe_st2(out + (size_t)i * 28, f2_muld(fe_ld2<Fq2T<L1, V1>>(a + (size_t)i * 28), fe_ld2<Fq2T<L2, V2>>(b + (size_t)i * 28)));
#endif
}
// out[0..27]: f2_sqrd(a); out[28..41]: fq_mul_beta(a.c0) (the raw lazy limbs)
template <uint64_t L1, int V1> __global__ void k_f2sqr(const uint32_t* a, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    const Fq2T<L1, V1> x = fe_ld2<Fq2T<L1, V1>>(a + (size_t)i * 28);
    fe_st2(out + (size_t)i * 42, f2_sqrd(x));
    fe_st(out + (size_t)i * 42 + 28, fq_mul_beta(x.c0));
#endif
}
#if !defined(RIPP_BLS12_377)
template <uint64_t LA, int VA, uint64_t LB, int VB_, uint64_t LC, int VC, uint64_t LD, int VD> __global__ void k_f2mulsub(const uint32_t* in, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t* s = in + (size_t)i * 112;
    fe_st2(out + (size_t)i * 28, f2_muld_sub(fe_ld2<Fq2T<LA, VA>>(s), fe_ld2<Fq2T<LB, VB_>>(s + 28), fe_ld2<Fq2T<LC, VC>>(s + 56), fe_ld2<Fq2T<LD, VD>>(s + 84)));
#endif
}
#endif
template <uint64_t L1, int V1, uint64_t L2, int V2> __global__ void k_f2mulfq(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    fe_st2(out + (size_t)i * 28, f2_mul_fq(fe_ld2<Fq2T<L1, V1>>(a + (size_t)i * 28), fe_ld<Fq<L2, V2>>(b + (size_t)i * 14)));
#endif
}
// storage conversions of 12 words x (per case, 122 words out):
//   [0, 14) fq_unpack(x)   [14, 26) fq_pack(fq_unpack(x))   [26, 40) fq_unpack_shl8(x)   [40, 54) fq_from_fp(x)   [54, 68) fq_from_fp_fast(x)
//   [68, 80) fq_to_fp(fq_from_fp(x))   [80, 94) fq_tab(x)   [94, 122) f2_tab((x, x))
__global__ void k_storage(const uint32_t* in, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    Fp x; for (int k = 0; k < 12; ++k) x.l[k] = in[(size_t)i * 12 + k];
    uint32_t* o = out + (size_t)i * 122;
    const Fqn u = fq_unpack(x.l);
    fe_st(o, u);
    { uint32_t w[12]; fq_pack(u, w); for (int k = 0; k < 12; ++k) o[14 + k] = w[k]; }
    fe_st(o + 26, fq_unpack_shl8(x.l));
    const Fqn f = fq_from_fp(x);
    fe_st(o + 40, f);
    fe_st(o + 54, fq_from_fp_fast(x));
    { const Fp t = fq_to_fp(f); for (int k = 0; k < 12; ++k) o[68 + k] = t.l[k]; }
    fe_st(o + 80, fq_tab(x));
    fe_st2(o + 94, f2_tab(Fp2{x, x}));
#endif
}
// out[0..11]: fq_to_fp(a) for a reduced value a (< 2p, normalised limbs)
__global__ void k_to_fp(const uint32_t* in, uint32_t* out, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    const Fp t = fq_to_fp(fe_ld<Fqn>(in + (size_t)i * 14));
    for (int k = 0; k < 12; ++k) out[(size_t)i * 12 + k] = t.l[k];
#endif
}

// ---- group law: per case X, Y, Z (the slot types) then x2, y2 of the affine operand; out: X, Y, Z; flag: the `special` result of an addition
// MODE 0: doubling; 1: mixed addition with a reduced affine operand (Fqn); 2: mixed addition with table operands (FqTab, FqTabY; G2: BLS12-381 only)
template <int MODE> __global__ void k_g1(const uint32_t* in, uint32_t* out, uint32_t* flag, uint32_t n) {
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t* s = in + (size_t)i * 70;
    JacQ p; p.x = fe_ld<JX>(s); p.y = fe_ld<JY>(s + 14); p.z = fe_ld<JZ>(s + 28);
    bool sp = false;
    if constexpr (MODE == 0) jdbl_q(p);
    else if constexpr (MODE == 1) sp = jmadd_q(p, fe_ld<Fqn>(s + 42), fe_ld<Fqn>(s + 56));
    else sp = jmadd_q(p, fe_ld<FqTab>(s + 42), fe_ld<FqTabY>(s + 56));
    uint32_t* o = out + (size_t)i * 42;
    fe_st(o, p.x); fe_st(o + 14, p.y); fe_st(o + 28, p.z);
    flag[i] = sp ? 1u : 0u;
#endif
}
template <int MODE> __global__ void __launch_bounds__(64) k_g2(const uint32_t* in, uint32_t* out, uint32_t* flag, uint32_t n) {
    __shared__ uint4 park_[7 * 64];
    FE_LANE
#if defined(__HIP_DEVICE_COMPILE__)
    uint4* park = park_ + threadIdx.x;
    const uint32_t* s = in + (size_t)i * 140;
    JacQ2 p; p.x = fe_ld2<Fq2X>(s); p.y = fe_ld2<Fq2Y>(s + 28); p.z = fe_ld2<Fq2Z>(s + 56);
    bool sp = false;
    if constexpr (MODE == 0) jdbl2_q(p);
    else if constexpr (MODE == 1) sp = jmadd2_q(p, [&]() { return fe_ld2<Fq2n>(s + 84); }, [&]() { return fe_ld2<Fq2n>(s + 112); }, park);
#if !defined(RIPP_BLS12_377)
    else sp = jmadd2_q(p, [&]() { return fe_ld2<Fq2T<FQ_LN, 256>>(s + 84); }, [&]() { return fe_ld2<Fq2T<FqTabY::LMAX, 258>>(s + 112); }, park);
#endif
    uint32_t* o = out + (size_t)i * 84;
    fe_st2(o, p.x); fe_st2(o + 28, p.y); fe_st2(o + 56, p.z);
    flag[i] = sp ? 1u : 0u;
#endif
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
#define FE_CHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
// one kernel over n lanes: `ins` host arrays of the given sizes in, `outs` out (uint32 words)
struct Io { const void* host; size_t words; };
struct Oo { void* host; size_t words; };
template <class LAUNCH> int run(uint32_t n, std::initializer_list<Io> ins, std::initializer_list<Oo> outs, LAUNCH launch) {
    DevBuf din[4], dout[3];
    const uint32_t* dpi[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t* dpo[3] = {nullptr, nullptr, nullptr};
    int k = 0;
    for (const Io& io : ins) { FE_CHK(din[k].alloc(io.words * 4)); FE_CHK(hipMemcpy(din[k].p, io.host, io.words * 4, hipMemcpyHostToDevice)); dpi[k] = din[k].as<uint32_t>(); ++k; }
    k = 0;
    for (const Oo& oo : outs) { FE_CHK(dout[k].alloc(oo.words * 4)); FE_CHK(hipMemset(dout[k].p, 0xA5, oo.words * 4)); dpo[k] = dout[k].as<uint32_t>(); ++k; }
    if (n > 0) { launch(dpi, dpo); FE_CHK(hipGetLastError()); }
    FE_CHK(hipDeviceSynchronize());
    k = 0;
    for (const Oo& oo : outs) { FE_CHK(hipMemcpy(oo.host, dout[k].p, oo.words * 4, hipMemcpyDeviceToHost)); ++k; }
    return 0;
}
inline dim3 blocks(uint32_t n, uint32_t bs) { return dim3((n + bs - 1) / bs); }
}  // namespace

extern "C" {
__attribute__((visibility("default"))) int fe_curve() {
#if defined(RIPP_BLS12_377)
    return 377;
#else
    return 381;
#endif
}

// table exports: kind 0 reduce, 1 norm (same list), 2 sub, 3 mul, 4 sqr, 5 dot2, 6 dot4, 7 mul_sub, 8 f2mul, 9 f2sqr, 10 f2mulsub, 11 f2mulfq.
// fe_count(kind): entries; fe_bounds(kind, id, lv): up to four (limb bound, value bound) pairs of operands into lv[0..7]
#define FE_CNT(LIST) FE_N(LIST)
__attribute__((visibility("default"))) int fe_count(int kind) {
    switch (kind) {
        case 0: case 1: return FE_CNT(FE_REDUCE_LIST);
        case 2: return FE_CNT(FE_SUB_LIST);
        case 3: return FE_CNT(FE_MUL_LIST);
        case 4: return FE_CNT(FE_SQR_LIST);
        case 5: return FE_CNT(FE_DOT2_LIST);
        case 6: return FE_CNT(FE_DOT4_LIST);
        case 7: return FE_CNT(FE_MULSUB_LIST);
        case 8: return FE_CNT(FE_F2MUL_LIST);
        case 9: return FE_CNT(FE_F2SQR_LIST);
#if !defined(RIPP_BLS12_377)
        case 10: return FE_CNT(FE_F2MULSUB_LIST);
#else
        case 10: return 0;
#endif
        case 11: return FE_CNT(FE_F2MULFQ_LIST);
    }
    return -1;
}
__attribute__((visibility("default"))) int fe_bounds(int kind, int id, uint64_t* lv) {
    for (int k = 0; k < 8; ++k) lv[k] = 0;
#define B1(ID, L, V) if (id == ID) { lv[0] = L; lv[1] = V; return 0; }
#define B2(ID, L1, V1, L2, V2) if (id == ID) { lv[0] = L1; lv[1] = V1; lv[2] = L2; lv[3] = V2; return 0; }
#define B4(ID, L1, V1, L2, V2, L3, V3, L4, V4) if (id == ID) { lv[0] = L1; lv[1] = V1; lv[2] = L2; lv[3] = V2; lv[4] = L3; lv[5] = V3; lv[6] = L4; lv[7] = V4; return 0; }
    switch (kind) {
        case 0: case 1: FE_REDUCE_LIST(B1) break;
        case 2: FE_SUB_LIST(B1) break;
        case 3: FE_MUL_LIST(B2) break;
        case 4: FE_SQR_LIST(B1) break;
        case 5: FE_DOT2_LIST(B2) break;
        case 6: FE_DOT4_LIST(B2) break;
        case 7: FE_MULSUB_LIST(B4) break;
        case 8: FE_F2MUL_LIST(B2) break;
        case 9: FE_F2SQR_LIST(B1) break;
#if !defined(RIPP_BLS12_377)
        case 10: FE_F2MULSUB_LIST(B4) break;
#endif
        case 11: FE_F2MULFQ_LIST(B2) break;
    }
#undef B1
#undef B2
#undef B4
    return -1;
}

// in: n x 14, out: n x 14, flag: n
__attribute__((visibility("default"))) int fe_reduce(int id, const uint32_t* in, uint32_t* out, uint32_t* flag, uint32_t n) {
    return run(n, {{in, (size_t)n * 14}}, {{out, (size_t)n * 14}, {flag, n}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, L, V) if (id == ID) hipLaunchKernelGGL((k_reduce<L, V>), blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], dout[1], n);
        FE_REDUCE_LIST(X)
#undef X
    });
}
__attribute__((visibility("default"))) int fe_norm(int id, const uint32_t* in, uint32_t* out, uint32_t n) {
    return run(n, {{in, (size_t)n * 14}}, {{out, (size_t)n * 14}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, L, V) if (id == ID) hipLaunchKernelGGL((k_norm<L, V>), blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], n);
        FE_REDUCE_LIST(X)
#undef X
    });
}
// out: n x 56 (fq_neg, fq_sub from an Fqn zero, f2_sub from an Fp2 zero)
__attribute__((visibility("default"))) int fe_sub(int id, const uint32_t* in, uint32_t* out, uint32_t n) {
    return run(n, {{in, (size_t)n * 14}}, {{out, (size_t)n * 56}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, L, V) if (id == ID) hipLaunchKernelGGL((k_sub<L, V>), blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], n);
        FE_SUB_LIST(X)
#undef X
    });
}
__attribute__((visibility("default"))) int fe_canon(const uint32_t* in, uint32_t* out, uint32_t* flag, uint32_t n) {
    return run(n, {{in, (size_t)n * 14}}, {{out, (size_t)n * 14}, {flag, n}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
        hipLaunchKernelGGL(k_canon, blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], dout[1], n);
    });
}
__attribute__((visibility("default"))) int fe_mul(int id, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    return run(n, {{a, (size_t)n * 14}, {b, (size_t)n * 14}}, {{out, (size_t)n * 14}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, L1, V1, L2, V2) if (id == ID) hipLaunchKernelGGL((k_mul<L1, V1, L2, V2>), blocks(n, 64), dim3(64), 0, 0, di[0], di[1], dout[0], n);
        FE_MUL_LIST(X)
#undef X
    });
}
__attribute__((visibility("default"))) int fe_sqr(int id, const uint32_t* a, uint32_t* out, uint32_t n) {
    return run(n, {{a, (size_t)n * 14}}, {{out, (size_t)n * 14}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, L, V) if (id == ID) hipLaunchKernelGGL((k_sqr<L, V>), blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], n);
        FE_SQR_LIST(X)
#undef X
    });
}
// a, b: n x NT x 14
__attribute__((visibility("default"))) int fe_dot(int nt, int id, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    if (nt != 2 && nt != 4) return -1;
    return run(n, {{a, (size_t)n * nt * 14}, {b, (size_t)n * nt * 14}}, {{out, (size_t)n * 14}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, L1, V1, L2, V2) if (nt == 2 && id == ID) hipLaunchKernelGGL((k_dot<2, L1, V1, L2, V2>), blocks(n, 64), dim3(64), 0, 0, di[0], di[1], dout[0], n);
        FE_DOT2_LIST(X)
#undef X
#define X(ID, L1, V1, L2, V2) if (nt == 4 && id == ID) hipLaunchKernelGGL((k_dot<4, L1, V1, L2, V2>), blocks(n, 64), dim3(64), 0, 0, di[0], di[1], dout[0], n);
        FE_DOT4_LIST(X)
#undef X
    });
}
// in: n x (a, b, c, d) x 14
__attribute__((visibility("default"))) int fe_mul_sub(int id, const uint32_t* in, uint32_t* out, uint32_t n) {
    return run(n, {{in, (size_t)n * 56}}, {{out, (size_t)n * 14}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, LA, VA, LB, VB, LC, VC, LD, VD) if (id == ID) hipLaunchKernelGGL((k_mul_sub<LA, VA, LB, VB, LC, VC, LD, VD>), blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], n);
        FE_MULSUB_LIST(X)
#undef X
    });
}
__attribute__((visibility("default"))) int fe_f2mul(int id, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    return run(n, {{a, (size_t)n * 28}, {b, (size_t)n * 28}}, {{out, (size_t)n * 28}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, L1, V1, L2, V2) if (id == ID) hipLaunchKernelGGL((k_f2mul<L1, V1, L2, V2>), blocks(n, 64), dim3(64), 0, 0, di[0], di[1], dout[0], n);
        FE_F2MUL_LIST(X)
#undef X
    });
}
// out: n x 42 (f2_sqrd: 28, fq_mul_beta of c0: 14)
__attribute__((visibility("default"))) int fe_f2sqr(int id, const uint32_t* a, uint32_t* out, uint32_t n) {
    return run(n, {{a, (size_t)n * 28}}, {{out, (size_t)n * 42}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, L, V) if (id == ID) hipLaunchKernelGGL((k_f2sqr<L, V>), blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], n);
        FE_F2SQR_LIST(X)
#undef X
    });
}
// in: n x (a, b, c, d) x 28
__attribute__((visibility("default"))) int fe_f2mulsub(int id, const uint32_t* in, uint32_t* out, uint32_t n) {
#if defined(RIPP_BLS12_377)
    (void)id; (void)in; (void)out; (void)n; return -1;
#else
    return run(n, {{in, (size_t)n * 112}}, {{out, (size_t)n * 28}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, LA, VA, LB, VB, LC, VC, LD, VD) if (id == ID) hipLaunchKernelGGL((k_f2mulsub<LA, VA, LB, VB, LC, VC, LD, VD>), blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], n);
        FE_F2MULSUB_LIST(X)
#undef X
    });
#endif
}
__attribute__((visibility("default"))) int fe_f2mulfq(int id, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
    return run(n, {{a, (size_t)n * 28}, {b, (size_t)n * 14}}, {{out, (size_t)n * 28}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
#define X(ID, L1, V1, L2, V2) if (id == ID) hipLaunchKernelGGL((k_f2mulfq<L1, V1, L2, V2>), blocks(n, 64), dim3(64), 0, 0, di[0], di[1], dout[0], n);
        FE_F2MULFQ_LIST(X)
#undef X
    });
}
// in: n x 12 words, out: n x 122
__attribute__((visibility("default"))) int fe_storage(const uint32_t* in, uint32_t* out, uint32_t n) {
    return run(n, {{in, (size_t)n * 12}}, {{out, (size_t)n * 122}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
        hipLaunchKernelGGL(k_storage, blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], n);
    });
}
__attribute__((visibility("default"))) int fe_to_fp(const uint32_t* in, uint32_t* out, uint32_t n) {
    return run(n, {{in, (size_t)n * 14}}, {{out, (size_t)n * 12}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
        hipLaunchKernelGGL(k_to_fp, blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], n);
    });
}
// G1: in n x 70, out n x 42;  G2: in n x 140, out n x 84;  flag: n
__attribute__((visibility("default"))) int fe_g1(int mode, const uint32_t* in, uint32_t* out, uint32_t* flag, uint32_t n) {
    if (mode < 0 || mode > 2) return -1;
    return run(n, {{in, (size_t)n * 70}}, {{out, (size_t)n * 42}, {flag, n}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
        if (mode == 0) hipLaunchKernelGGL(k_g1<0>, blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], dout[1], n);
        else if (mode == 1) hipLaunchKernelGGL(k_g1<1>, blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], dout[1], n);
        else hipLaunchKernelGGL(k_g1<2>, blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], dout[1], n);
    });
}
__attribute__((visibility("default"))) int fe_g2(int mode, const uint32_t* in, uint32_t* out, uint32_t* flag, uint32_t n) {
#if defined(RIPP_BLS12_377)
    if (mode < 0 || mode > 1) return -1;
#else
    if (mode < 0 || mode > 2) return -1;
#endif
    return run(n, {{in, (size_t)n * 140}}, {{out, (size_t)n * 84}, {flag, n}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
        if (mode == 0) hipLaunchKernelGGL(k_g2<0>, blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], dout[1], n);
        else if (mode == 1) hipLaunchKernelGGL(k_g2<1>, blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], dout[1], n);
#if !defined(RIPP_BLS12_377)
        else hipLaunchKernelGGL(k_g2<2>, blocks(n, 64), dim3(64), 0, 0, di[0], dout[0], dout[1], n);
#endif
    });
}
// Stage 2a of the pairing product, launched as the engine launches it (engine.hip enqueue_stage2): lines = rows x 18 x stride chunks of 16 bytes
// (chunk (r 18 + 3 f + c) stride + i: coefficient f = l0.c0, l0.c1, l1.c0, .. of line i, 12 words), partials = rows x 36 x T chunks.
// kara = 1: k_line_products_k (BLS12-381 only), 0: k_line_products_q.
__attribute__((visibility("default"))) int fe_line_products(int kara, const uint32_t* lines, size_t stride, uint32_t M, uint32_t T, uint32_t rows, uint32_t* partials) {
    if (T == 0 || rows == 0 || stride < M) return -1;
#if defined(RIPP_BLS12_377)
    if (kara) return -1;
#endif
    const size_t lw = (size_t)rows * 18 * stride * 4, pw = (size_t)rows * 36 * T * 4;
    return run(1, {{lines, lw}}, {{partials, pw}}, [&](const uint32_t* const* di, uint32_t* const* dout) {
        const uint4* l = reinterpret_cast<const uint4*>(di[0]); uint4* p = reinterpret_cast<uint4*>(dout[0]);
#if !defined(RIPP_BLS12_377)
        if (kara) { hipLaunchKernelGGL(k_line_products_k, dim3((T + LK_GROUPS_PER_WAVE - 1) / LK_GROUPS_PER_WAVE, rows), dim3(64), 0, 0, l, stride, M, p, T); return; }
#endif
        hipLaunchKernelGGL(k_line_products_q, dim3((T + LP_GROUPS_PER_WAVE - 1) / LP_GROUPS_PER_WAVE, rows), dim3(64), 0, 0, l, stride, M, p, T);
    });
}
}  // extern "C"
