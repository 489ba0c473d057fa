// Device test harness for the 32-bit Montgomery form Mont<P> (bls12_381/fp.hpp: Fr with 8 limbs, Fp with 12) and the Fr kernels built on it: the Barrett
// division msm_divmod and the five digit passes that copy it (msm.hpp, msm_batch.hpp, tpc.hpp, gipa_mexp.hpp, tipa_scalar.hpp), the KZG quotient scan with
// its production launch sequence (msm_batch.hpp kzg_quotient_launch), k_pc_partial_eval, k_fr_dot / k_fr_dot2 and k_fold_fr / k_fold_fr2.  It includes the
// production headers unchanged; tests/test_gpu_fr_edges.py feeds it the cases of tests/fr_edges.py and compares every result with Python integers.
//
// Built twice by tests/device/Makefile: libfr_edges_381.so and libfr_edges_377.so (-DRIPP_BLS12_377).  Every launcher takes HOST arrays, copies them to the
// device, runs one kernel (or the scan's three), waits and copies the results back; it returns the HIP error code (0 = success, -1 = refused arguments: every
// size that decides where a kernel writes is checked against the buffers here, before the launch).  Outputs are prefilled with the byte 0xA5 (digits: 0xFF)
// and are longer than what the kernel may write, so that the caller sees a store that went astray.
// All values are the engine's: 8 words per Fr, 12 per Fp, little-endian; Montgomery form unless stated.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../ripp_amd/csrc/kernels.hpp"
#include "../../ripp_amd/csrc/msm_batch.hpp"
#include "../../ripp_amd/csrc/tpc.hpp"
#include "../../ripp_amd/csrc/gipa_mexp.hpp"
#include "../../ripp_amd/csrc/tipa_scalar.hpp"

using namespace ripp;

enum { FE_MUL = 0, FE_SQR, FE_ADD, FE_SUB, FE_NEG, FE_FROM_MONT, FE_TO_MONT, FE_MUL2_ADD, FE_MUL_CIOS, FE_NOPS };

// one lane per case; on the device mul / sqr / from_mont / to_mont / mul2_add are the column-accumulator forms, mul_cios the portable one
template <class P, int OP>
__global__ void __launch_bounds__(256) k_fe_mont(const Mont<P>* __restrict__ a, const Mont<P>* __restrict__ b, const Mont<P>* __restrict__ c, const Mont<P>* __restrict__ d,
                                                 uint32_t n, Mont<P>* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
    Mont<P> r;
    if constexpr (OP == FE_MUL) r = mul(a[i], b[i]);
    else if constexpr (OP == FE_SQR) r = sqr(a[i]);
    else if constexpr (OP == FE_ADD) r = add(a[i], b[i]);
    else if constexpr (OP == FE_SUB) r = sub(a[i], b[i]);
    else if constexpr (OP == FE_NEG) r = neg(a[i]);
    else if constexpr (OP == FE_FROM_MONT) r = from_mont(a[i]);
    else if constexpr (OP == FE_TO_MONT) r = to_mont(a[i]);
    else if constexpr (OP == FE_MUL2_ADD) r = mul2_add(a[i], b[i], c[i], d[i]);
    else r = mul_cios(a[i], b[i]);
    out[i] = r;
#endif
}

// k: canonical scalars.  q / rem: what msm_divmod<4, 5> leaves (8 and 5 words)
__global__ void __launch_bounds__(256) k_fe_divmod_lambda(const Fr* __restrict__ k, uint32_t n, uint32_t* __restrict__ q, uint32_t* __restrict__ rem) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr v = k[i];
    const uint32_t lam[8] = RIPP_GLV_LAMBDA;
    const uint32_t lam_mu[5] = RIPP_GLV_LAMBDA_MU;
    uint32_t r[5];
    msm_divmod<4, 5>(v.l, lam, lam_mu, r);
    for (int t = 0; t < 8; ++t) q[(size_t)i * 8 + t] = v.l[t];
    for (int t = 0; t < 5; ++t) rem[(size_t)i * 5 + t] = r[t];
}
// the chain of k_msm_digits' GLS branch: q / rem of step j at [i][j] (8 and 3 words)
__global__ void __launch_bounds__(256) k_fe_divmod_x(const Fr* __restrict__ k, uint32_t n, uint32_t* __restrict__ q, uint32_t* __restrict__ rem) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr v = k[i];
    const uint32_t u[2] = RIPP_X_ABS_LIMBS;
    const uint32_t u_mu[7] = RIPP_X_ABS_MU;
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
        uint32_t r[3];
        msm_divmod<2, 7>(v.l, u, u_mu, r);
        for (int t = 0; t < 8; ++t) q[((size_t)i * 3 + j) * 8 + t] = v.l[t];
        for (int t = 0; t < 3; ++t) rem[((size_t)i * 3 + j) * 3 + t] = r[t];
    }
}

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    hipError_t fill(size_t bytes, int byte) { const hipError_t e = alloc(bytes); return (e != hipSuccess || bytes == 0) ? e : hipMemset(p, byte, bytes); }
    hipError_t put(const void* host, size_t bytes) { const hipError_t e = alloc(bytes); return (e != hipSuccess || bytes == 0) ? e : hipMemcpy(p, host, bytes, hipMemcpyHostToDevice); }
    hipError_t get(void* host, size_t bytes) const { return bytes ? hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
#define FE_CHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
#define FE_API extern "C" __attribute__((visibility("default")))
constexpr size_t FE_MAX_N = (size_t)1 << 20;
inline dim3 fe_grid(size_t n, uint32_t block) { return dim3((unsigned)((n + block - 1) / block)); }
inline Fr fe_fr(const uint32_t* w) { Fr r; for (int i = 0; i < 8; ++i) r.l[i] = w[i]; return r; }
inline MsmPlan fe_plan_of(const uint32_t* w) { MsmPlan p; p.c = (int)w[0]; p.nwin = (int)w[1]; p.nb = w[2]; p.n = w[3]; p.ch = w[4]; p.seg = w[5]; p.nreal = w[6]; p.gmin = w[7]; return p; }

template <class P, int OP>
int fe_mont_run(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t n, uint32_t* out) {
    using F = Mont<P>;
    DevBuf da, db, dc, dd, dout;
    const size_t bytes = (size_t)n * sizeof(F);
    FE_CHK(da.put(a, bytes)); FE_CHK(db.put(b, bytes)); FE_CHK(dc.put(c, bytes)); FE_CHK(dd.put(d, bytes)); FE_CHK(dout.fill(bytes, 0xA5));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fe_mont<P, OP>), fe_grid(n, 256), dim3(256), 0, 0, da.as<F>(), db.as<F>(), dc.as<F>(), dd.as<F>(), n, dout.as<F>());
    FE_CHK(hipGetLastError()); FE_CHK(hipDeviceSynchronize());
    FE_CHK(dout.get(out, bytes));
    return 0;
}
template <class P>
int fe_mont_op(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t n, uint32_t* out) {
    switch (op) {
    case FE_MUL: return fe_mont_run<P, FE_MUL>(a, b, c, d, n, out);
    case FE_SQR: return fe_mont_run<P, FE_SQR>(a, b, c, d, n, out);
    case FE_ADD: return fe_mont_run<P, FE_ADD>(a, b, c, d, n, out);
    case FE_SUB: return fe_mont_run<P, FE_SUB>(a, b, c, d, n, out);
    case FE_NEG: return fe_mont_run<P, FE_NEG>(a, b, c, d, n, out);
    case FE_FROM_MONT: return fe_mont_run<P, FE_FROM_MONT>(a, b, c, d, n, out);
    case FE_TO_MONT: return fe_mont_run<P, FE_TO_MONT>(a, b, c, d, n, out);
    case FE_MUL_CIOS: return fe_mont_run<P, FE_MUL_CIOS>(a, b, c, d, n, out);
    default: return -1;
    }
}
}  // namespace

static_assert(sizeof(Fr) == 32 && sizeof(Fp) == 48 && sizeof(MsmPlan) == 32, "the layouts the Python side packs");

FE_API int fe_curve() {
#if defined(RIPP_BLS12_377)
    return 377;
#else
    return 381;
#endif
}

// field 0: Fr (n x 8 words), 1: Fp (n x 12 words).  op: the FE_ list above; a, b, c, d all hold n values (the operation reads those it needs).
// FE_MUL2_ADD is the form of Fp only.
FE_API int fe_mont(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t n, uint32_t* out) {
    if (field < 0 || field > 1 || op < 0 || op >= FE_NOPS || n == 0 || n > FE_MAX_N || !a || !b || !c || !d || !out) return -1;
    if (op == FE_MUL2_ADD) return field == 1 ? fe_mont_run<FpParams, FE_MUL2_ADD>(a, b, c, d, n, out) : -1;
    return field ? fe_mont_op<FpParams>(op, a, b, c, d, n, out) : fe_mont_op<FrParams>(op, a, b, c, d, n, out);
}

// k: n canonical scalars (8 words).  by_x = 0: msm_divmod<4, 5> by lambda, q n x 8 words, rem n x 5.  by_x = 1: three msm_divmod<2, 7> by |x| in a chain, q n x 3 x 8, rem n x 3 x 3
FE_API int fe_divmod(int by_x, const uint32_t* k, uint32_t n, uint32_t* q, uint32_t* rem) {
    if (by_x < 0 || by_x > 1 || n == 0 || n > FE_MAX_N) return -1;
    DevBuf dk, dq, dr;
    const size_t qb = (size_t)n * (by_x ? 24 : 8) * 4, rb = (size_t)n * (by_x ? 9 : 5) * 4;
    FE_CHK(dk.put(k, (size_t)n * sizeof(Fr))); FE_CHK(dq.fill(qb, 0xA5)); FE_CHK(dr.fill(rb, 0xA5));
    if (by_x) hipLaunchKernelGGL(k_fe_divmod_x, fe_grid(n, 256), dim3(256), 0, 0, dk.as<Fr>(), n, dq.as<uint32_t>(), dr.as<uint32_t>());
    else hipLaunchKernelGGL(k_fe_divmod_lambda, fe_grid(n, 256), dim3(256), 0, 0, dk.as<Fr>(), n, dq.as<uint32_t>(), dr.as<uint32_t>());
    FE_CHK(hipGetLastError()); FE_CHK(hipDeviceSynchronize());
    FE_CHK(dq.get(q, qb)); FE_CHK(dr.get(rem, rb));
    return 0;
}

// msm_plan (rows = 0) / msm_plan_batch (rows >= 1) on the host with MsmTune{c, ch, gmin}: out = c, nwin, nb, n, ch, seg, nreal, gmin
FE_API int fe_plan(size_t nreal, int split, size_t rows, int c, uint32_t ch, uint32_t gmin, uint32_t* out) {
    if (nreal == 0 || nreal > FE_MAX_N || (split != 1 && split != 2 && split != 4) || (c != 0 && (c < 4 || c > 13)) || rows > 64) return -1;
    MsmTune t; t.c = c; t.ch = ch; t.gmin = gmin;
    const MsmPlan p = rows ? msm_plan_batch(nreal, split, rows, t) : msm_plan(nreal, split, t);
    out[0] = (uint32_t)p.c; out[1] = (uint32_t)p.nwin; out[2] = p.nb; out[3] = p.n; out[4] = p.ch; out[5] = p.seg; out[6] = p.nreal; out[7] = p.gmin;
    return 0;
}

// The digit passes.  which 0: k_msm_digits (rows = 1; arg unused; hist: nwin x nb counters, zero before the launch), 1: k_msm_digits_batch (arg = cols, stride),
// 2: k_tpc_digits_cross (arg = h), 3: k_gipa_mexp_digits (arg = len), 4: k_tipa_scalar_digits_cross_g2 (arg = h).  scalars: nscalars x 8 words.
// plan: the eight words of fe_plan.  digits: rows x nwin x n digits and `guard` more behind them, all 0xFFFF before the launch.
FE_API int fe_digits(int which, const uint32_t* scalars, size_t nscalars, uint32_t arg, size_t stride, uint32_t rows, const uint32_t* plan, size_t guard, uint16_t* digits, uint32_t* hist) {
    if (which < 0 || which > 4 || !plan || nscalars == 0 || nscalars > FE_MAX_N || guard > FE_MAX_N) return -1;
    const MsmPlan p = fe_plan_of(plan);
    if (p.nreal == 0 || p.nreal > FE_MAX_N || p.c < 4 || p.c > 13 || p.nb != (1u << p.c)) return -1;
    const uint32_t split = p.n / p.nreal;
    if ((size_t)split * p.nreal != p.n || (split != 1 && split != 2 && split != 4)) return -1;
    const int nbits = split == 1 ? 255 : split == 2 ? 128 : 64;
    if (p.nwin != (nbits + p.c - 1) / p.c) return -1;                                // the window loop reads limb (nwin - 1) c / 32 of a 3-, 5- or 8-limb value
    switch (which) {
    case 0: if (rows != 1 || nscalars < p.nreal || !hist) return -1; break;
    case 1: if (split != 2 || rows < 1 || rows > 64 || arg > p.nreal || stride < arg || nscalars < (size_t)(rows - 1) * stride + arg) return -1; break;
    case 2: if (split != 2 || rows != 2 || arg == 0 || p.nreal != 2 * arg || nscalars < 2 * (size_t)arg) return -1; break;
    case 3: if (split != 2 || rows != 4 || arg == 0 || (arg & 1) || p.nreal != 2 * arg || nscalars < arg) return -1; break;
    default: if (split != 4 || rows != 2 || arg == 0 || p.nreal != 2 * arg || nscalars < 2 * (size_t)arg) return -1; break;
    }
    const size_t nd = (size_t)rows * (size_t)p.nwin * p.n, hb = (size_t)p.nwin * p.nb * sizeof(uint32_t);
    DevBuf ds, dd, dh;
    FE_CHK(ds.put(scalars, nscalars * sizeof(Fr))); FE_CHK(dd.fill((nd + guard) * sizeof(uint16_t), 0xFF));
    if (which == 0) FE_CHK(dh.fill(hb, 0));
    const Fr* const s = ds.as<Fr>(); uint16_t* const dg = dd.as<uint16_t>();
    if (which == 0) hipLaunchKernelGGL(k_msm_digits, fe_grid(p.nreal, 256), dim3(256), 0, 0, s, p, dg, dh.as<uint32_t>());
    else if (which == 1) hipLaunchKernelGGL(k_msm_digits_batch, dim3(fe_grid(p.nreal, 256).x, rows), dim3(256), 0, 0, s, arg, stride, p, dg);
    else if (which == 2) hipLaunchKernelGGL(k_tpc_digits_cross, dim3(fe_grid(p.nreal, 256).x, 2), dim3(256), 0, 0, s, arg, p, dg);
    else if (which == 3) hipLaunchKernelGGL(k_gipa_mexp_digits, fe_grid(arg, 256), dim3(256), 0, 0, s, arg, p, dg);
    else hipLaunchKernelGGL(k_tipa_scalar_digits_cross_g2, dim3(fe_grid(p.nreal, 256).x, 2), dim3(256), 0, 0, s, arg, p, dg);
    FE_CHK(hipGetLastError()); FE_CHK(hipDeviceSynchronize());
    FE_CHK(dd.get(digits, (nd + guard) * sizeof(uint16_t)));
    if (which == 0) FE_CHK(dh.get(hist, hb));
    return 0;
}

// The KZG scan through kzg_quotient_launch: p = m coefficients, per = 0 (the formula) or the caller's lane share.  h and cin: nchunk + 1 values each, q: m + 2 values
// (the production layout q[0 .. m - 1), q[m - 1] not written, q[m] = p(z), and one slot behind it); what the kernels do not write stays 0xA5.
FE_API int fe_kzg_scan(const uint32_t* p, size_t m, const uint32_t* z, size_t per, uint32_t* h, uint32_t* cin, uint32_t* q) {
    if (m == 0 || m > FE_MAX_N) return -1;
    const size_t nchunk = (m + KZG_CHUNK - 1) / KZG_CHUNK;
    if (per && (per * KZG_SCAN_LANES < nchunk || per > FE_MAX_N)) return -1;
    DevBuf dp, dh, dc, dq;
    FE_CHK(dp.put(p, m * sizeof(Fr))); FE_CHK(dh.fill((nchunk + 1) * sizeof(Fr), 0xA5)); FE_CHK(dc.fill((nchunk + 1) * sizeof(Fr), 0xA5)); FE_CHK(dq.fill((m + 2) * sizeof(Fr), 0xA5));
    kzg_quotient_launch((hipStream_t)0, dp.as<Fr>(), m, fe_fr(z), dh.as<Fr>(), dc.as<Fr>(), dq.as<Fr>(), per);
    FE_CHK(hipGetLastError()); FE_CHK(hipDeviceSynchronize());
    FE_CHK(dh.get(h, (nchunk + 1) * sizeof(Fr))); FE_CHK(dc.get(cin, (nchunk + 1) * sizeof(Fr))); FE_CHK(dq.get(q, (m + 2) * sizeof(Fr)));
    return 0;
}

// coef: rows x stride, xp: rows, out: out_len >= ncols values
FE_API int fe_partial_eval(const uint32_t* coef, uint32_t rows, uint32_t cols, size_t stride, const uint32_t* xp, uint32_t ncols, size_t out_len, uint32_t* out) {
    if (rows == 0 || rows > 4096 || cols > stride || stride > FE_MAX_N || cols > ncols || ncols == 0 || ncols > out_len || out_len > FE_MAX_N || (size_t)rows * stride > FE_MAX_N) return -1;
    DevBuf dc, dx, dout;
    FE_CHK(dc.put(coef, (size_t)rows * stride * sizeof(Fr))); FE_CHK(dx.put(xp, (size_t)rows * sizeof(Fr))); FE_CHK(dout.fill(out_len * sizeof(Fr), 0xA5));
    hipLaunchKernelGGL(k_pc_partial_eval, fe_grid(ncols, 256), dim3(256), 0, 0, dc.as<Fr>(), rows, cols, stride, dx.as<Fr>(), ncols, dout.as<Fr>());
    FE_CHK(hipGetLastError()); FE_CHK(hipDeviceSynchronize());
    FE_CHK(dout.get(out, out_len * sizeof(Fr)));
    return 0;
}

// two = 0: k_fr_dot over l, r (n values each), partials: grid + 1 values.  two = 1: k_fr_dot2 with l = m, r = b (2 n values each, n = h), partials: 2 grid + 1 values
FE_API int fe_fr_dot(int two, const uint32_t* l, const uint32_t* r, uint32_t n, uint32_t grid, uint32_t* partials) {
    if (two < 0 || two > 1 || n == 0 || n > FE_MAX_N || grid == 0 || grid > 1024) return -1;
    DevBuf dl, dr, dp;
    const size_t in = (size_t)n * (two ? 2 : 1) * sizeof(Fr), ob = ((size_t)grid * (two ? 2 : 1) + 1) * sizeof(Fr);
    FE_CHK(dl.put(l, in)); FE_CHK(dr.put(r, in)); FE_CHK(dp.fill(ob, 0xA5));
    if (two) hipLaunchKernelGGL(k_fr_dot2, dim3(grid, 2), dim3(256), 0, 0, dl.as<Fr>(), dr.as<Fr>(), n, dp.as<Fr>());
    else hipLaunchKernelGGL(k_fr_dot, dim3(grid), dim3(256), 0, 0, dl.as<Fr>(), dr.as<Fr>(), n, dp.as<Fr>());
    FE_CHK(hipGetLastError()); FE_CHK(hipDeviceSynchronize());
    FE_CHK(dp.get(partials, ob));
    return 0;
}

// k_fold_fr: out[i] = hi[i] s + lo[i], i < half; out: out_len >= half values
FE_API int fe_fold_fr(const uint32_t* hi, const uint32_t* lo, uint32_t half, const uint32_t* s, size_t out_len, uint32_t* out) {
    if (half == 0 || half > FE_MAX_N || out_len < half || out_len > 2 * FE_MAX_N) return -1;
    DevBuf dh, dl, dout;
    FE_CHK(dh.put(hi, (size_t)half * sizeof(Fr))); FE_CHK(dl.put(lo, (size_t)half * sizeof(Fr))); FE_CHK(dout.fill(out_len * sizeof(Fr), 0xA5));
    hipLaunchKernelGGL(k_fold_fr, fe_grid(half, 256), dim3(256), 0, 0, dh.as<Fr>(), dl.as<Fr>(), half, fe_fr(s), dout.as<Fr>());
    FE_CHK(hipGetLastError()); FE_CHK(hipDeviceSynchronize());
    FE_CHK(dout.get(out, out_len * sizeof(Fr)));
    return 0;
}

// k_fold_fr2 with the engine's grid (ceil(h / 256), 2): m, b: 2 h values each; m_out, b_out: out_len >= h values each
FE_API int fe_fold_fr2(const uint32_t* m, const uint32_t* b, uint32_t h, const uint32_t* c, const uint32_t* c_inv, size_t out_len, uint32_t* m_out, uint32_t* b_out) {
    if (h == 0 || h > FE_MAX_N || out_len < h || out_len > 2 * FE_MAX_N) return -1;
    DevBuf dm, db, dmo, dbo;
    FE_CHK(dm.put(m, 2 * (size_t)h * sizeof(Fr))); FE_CHK(db.put(b, 2 * (size_t)h * sizeof(Fr))); FE_CHK(dmo.fill(out_len * sizeof(Fr), 0xA5)); FE_CHK(dbo.fill(out_len * sizeof(Fr), 0xA5));
    hipLaunchKernelGGL(k_fold_fr2, dim3(fe_grid(h, 256).x, 2), dim3(256), 0, 0, dm.as<Fr>(), db.as<Fr>(), h, fe_fr(c), fe_fr(c_inv), dmo.as<Fr>(), dbo.as<Fr>());
    FE_CHK(hipGetLastError()); FE_CHK(hipDeviceSynchronize());
    FE_CHK(dmo.get(m_out, out_len * sizeof(Fr))); FE_CHK(dbo.get(b_out, out_len * sizeof(Fr)));
    return 0;
}
