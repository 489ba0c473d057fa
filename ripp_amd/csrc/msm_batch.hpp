// Batched shared-base G1 multi-scalar multiplication and the Fr kernels of the polynomial commitments
// (ip_proofs/src/applications/poly_commit/mod.rs) on gfx950.
//
//   out[r] = sum_i scalars[r][i] * bases[i],   r < rows          (the x_degree + 1 KZG commitments of BivariatePolynomialCommitment::commit, mod.rs:174-196)
//
// The pipeline of msm.hpp already indexes its windows through gridDim.y and keeps every per-window array at `w * stride`.  A batch is that
// pipeline over the rows * nwin (row, window) pairs: the stages between the digit pass and the Horner finish never look at how many windows a
// scalar has, so they run UNCHANGED with the plan's nwin set to rows * nwin ("virtual windows" v = r * nwin + w).  Term indices are the same in every
// row, so all rows gather from ONE extended base array (fq_msm.hpp k_msm_extend_q).  New here: the digit pass over a scalar matrix and the finish,
// which runs the Horner recurrence of four rows per wave (one per 16-lane group of the field VM) instead of one in total.
//
//   k_msm_digits_batch      lane per (row, base): GLV split, c-bit digits of the row's windows; columns >= cols are zero scalars
//   (msm.hpp / fq_msm.hpp)  hist -> scan -> scatter -> slot sums (+ exceptional-slot fix-up) -> group -> merge -> segments -> reduce, grid.y = rows * nwin
//   k_msm_finish_vm_batch   group per row: T <- W_top; T <- 2^c T + W_w
//
//   k_pc_partial_eval       y_eval[j] = sum_i x^i c[i][j]  (mod.rs:228-234), lane per column
//   k_kzg_chunk_sums / k_kzg_carry_scan / k_kzg_quotient   the quotient of p(X) by (X - z) and p(z) (mod.rs:96-104) as a suffix scan
#pragma once
#include "msm.hpp"

namespace ripp {

// The plan of ONE row with the slot length chosen for the whole launch: the rule of msm_plan ("the shortest chain that still gives every SIMD two
// waves") is about the launch, and the launch holds rows times the additions.  The window width stays the row's own: every (row, window) pair has
// its own 2^c buckets, so the bucket work per term is that of a lone MSM of the row's length.
inline MsmPlan msm_plan_batch(size_t nreal, int split, size_t rows, const MsmTune& tune = MsmTune()) {
    MsmPlan p = msm_plan(nreal, split, tune);
    if (!tune.ch) {
        const size_t adds = (size_t)p.n * (size_t)p.nwin * rows;
        p.ch = 4; while (p.ch < 32 && (size_t)p.ch * 131072 < adds) p.ch *= 2;
        if ((size_t)p.n * rows > ((size_t)1 << 20)) p.ch = 64;
    }
    return p;
}

// p: the plan of one row (p.nwin windows).  Row r writes its digits at digits + r * p.nwin * p.n, i.e. as windows r * nwin .. of the batch.
// scalars: row-major, `stride` elements from one row to the next; columns [cols, p.nreal) count as zero (they sort into no bucket).
__global__ void __launch_bounds__(256) k_msm_digits_batch(const Fr* __restrict__ scalars, uint32_t cols, size_t stride, MsmPlan p, uint16_t* __restrict__ digits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (i >= p.nreal) return;
    uint16_t* const dg = digits + (size_t)r * (size_t)p.nwin * p.n;
    Fr k = Fr::zero();
    if (i < cols) k = from_mont(scalars[(size_t)r * stride + i]);
    const uint32_t lam[8] = RIPP_GLV_LAMBDA;
    const uint32_t lam_mu[5] = RIPP_GLV_LAMBDA_MU;
    uint32_t rem[5];
    msm_divmod<4, 5>(k.l, lam, lam_mu, rem);                                          // k = q * lambda + rem, both < 2^128 (msm.hpp k_msm_digits)
    msm_emit_digits(rem, 5, i, p, dg, nullptr);
    msm_emit_digits(k.l, 8, p.nreal + i, p, dg, nullptr);
}

// block of 64 lanes = 4 rows; win[r * p.nwin + w] is the homogeneous sum of window w of row r (k_msm_vm_reduce ran down to one per virtual window).
// Every group walks the same p.nwin windows and p.c doublings, so the wave stays converged; groups past the last row carry the identity.
template <class F>
__global__ void __launch_bounds__(64) k_msm_finish_vm_batch(MsmPlan p, uint32_t rows, const Jac<F>* __restrict__ win, Jac<F>* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vm_smem[];
    using C = VmCurve<F>;
    const int lane = threadIdx.x, lg = lane & (VM_G - 1), grp = lane / VM_G;
    VmSlot* const ws = reinterpret_cast<VmSlot*>(vm_smem) + (size_t)grp * C::SLOTS;
    const uint32_t r = blockIdx.x * VM_EPW + grp;
    const bool active = r < rows;
    const Jac<F>* const w_r = win + (size_t)(active ? r : 0) * p.nwin;
    if (lg == 0) { vm_zero(ws); vm_put_t<F>(ws, active ? w_r[p.nwin - 1] : msm_id_h<F>()); }
#pragma unroll 1
    for (int w = p.nwin - 2; w >= 0; --w) {
#pragma unroll 1
        for (int k = 0; k < p.c; ++k) C::dbl_(ws, lg);
        if (lg == 0) vm_put_q<F>(ws, active ? w_r[w] : msm_id_h<F>());
        C::add_(ws, lg);
    }
    if (active && lg == 0) {
        const Jac<F> t = vm_get_t<F>(ws);
        Jac<F> res = jac_inf<F>();
        if (!t.z.is_zero()) { res.x = fmul(t.x, t.z); res.y = fmul(t.y, fsqr(t.z)); res.z = t.z; }      // (X : Y : Z) -> Jacobian (X Z, Y Z^2, Z)
        out[r] = res;
    }
}

// ---- partial evaluation p(x, Y) of a bivariate polynomial (mod.rs:228-234) ------------------------------------------------------------
// coef: row-major [rows][stride], row i = the coefficients of y_polynomials[i]; xp[i] = x^i.  Lane j owns column j: adjacent lanes read adjacent
// coefficients of one row.  Columns [cols, ncols) are written as zero (the padding the reference gives every row).
__global__ void __launch_bounds__(256) k_pc_partial_eval(const Fr* __restrict__ coef, uint32_t rows, uint32_t cols, size_t stride, const Fr* __restrict__ xp, uint32_t ncols, Fr* __restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ncols) return;
    Fr acc = Fr::zero();
    if (j < cols) {
#pragma unroll 1
        for (uint32_t i = 0; i < rows; ++i) acc = add(acc, mul(xp[i], coef[(size_t)i * stride + j]));
    }
    out[j] = acc;
}

// ---- KZG quotient and evaluation (mod.rs:96-104) -----------------------------------------------------------------------------------------
// q[i-1] = p[i] + z q[i] is the suffix Horner value  s[j] = sum_{k >= j} p[k] z^(k - j):  q[j] = s[j + 1], p(z) = s[0].
// Chunks of KZG_CHUNK coefficients, one lane each:
//   k_kzg_chunk_sums   h[c] = sum_{k in chunk c} p[k] z^(k - start_c)                          (chunk-local Horner)
//   k_kzg_carry_scan   cin[c] = s[start_(c+1)] = h[c+1] + z^T cin[c+1]: one block; lane l owns `per` consecutive chunks, reduces them with z^T, the
//                      256 lane sums are scanned through LDS with z^(T per), then every lane walks its chunks again with its carry-in
//   k_kzg_quotient     second pass over the chunk from cin[c]: writes s[k] to q[k - 1], s[0] to *eval
// Exact field arithmetic: the result does not depend on the chunking.
constexpr uint32_t KZG_CHUNK = 64;
constexpr uint32_t KZG_SCAN_LANES = 256;
__global__ void __launch_bounds__(256) k_kzg_chunk_sums(const Fr* __restrict__ p, uint32_t m, Fr z, Fr* __restrict__ h) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = (uint64_t)c * KZG_CHUNK;
    if (lo >= m) return;
    const uint32_t hi = lo + KZG_CHUNK < (uint64_t)m ? (uint32_t)(lo + KZG_CHUNK) : m;
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t k = hi; k-- > (uint32_t)lo;) acc = add(mul(acc, z), p[k]);
    h[c] = acc;
}
__global__ void __launch_bounds__(KZG_SCAN_LANES) k_kzg_carry_scan(const Fr* __restrict__ h, uint32_t nchunk, uint32_t per, Fr zT, Fr zTper, Fr* __restrict__ cin) {
    __shared__ Fr sh[KZG_SCAN_LANES];
    const uint32_t l = threadIdx.x;
    const uint64_t lo64 = (uint64_t)l * per;
    const uint32_t lo = lo64 < nchunk ? (uint32_t)lo64 : nchunk, hi = lo64 + per < nchunk ? (uint32_t)(lo64 + per) : nchunk;
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t c = hi; c-- > lo;) acc = add(mul(acc, zT), h[c]);                 // value of lane l's chunks, in units of z^T, from its first chunk
    sh[l] = acc; __syncthreads();
    if (l == 0) {                                                                     // sh[l] <- carry INTO lane l's last chunk = value of everything above lane l
        Fr run = Fr::zero();
#pragma unroll 1
        for (uint32_t t = KZG_SCAN_LANES; t-- > 0;) { const Fr own = sh[t]; sh[t] = run; run = add(mul(run, zTper), own); }
    }
    __syncthreads();
    // A lane whose range is cut short by nchunk holds fewer than `per` chunks, but only the LAST non-empty lane can be short and everything above it is zero,
    // so the uniform factor z^(T per) multiplies zero there.
    Fr run = sh[l];
#pragma unroll 1
    for (uint32_t c = hi; c-- > lo;) { cin[c] = run; run = add(mul(run, zT), h[c]); }
}
__global__ void __launch_bounds__(256) k_kzg_quotient(const Fr* __restrict__ p, uint32_t m, Fr z, const Fr* __restrict__ cin, Fr* __restrict__ q, Fr* __restrict__ eval) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = (uint64_t)c * KZG_CHUNK;
    if (lo >= m) return;
    const uint32_t hi = lo + KZG_CHUNK < (uint64_t)m ? (uint32_t)(lo + KZG_CHUNK) : m;
    Fr acc = cin[c];
#pragma unroll 1
    for (uint32_t k = hi; k-- > (uint32_t)lo;) {
        acc = add(mul(acc, z), p[k]);                                                 // s[k]
        if (k) q[k - 1] = acc; else *eval = acc;
    }
}

inline Fr fr_pow_u(Fr b, size_t k) { Fr r = Fr::one(); while (k) { if (k & 1) r = mul(r, b); b = mul(b, b); k >>= 1; } return r; }
// The launch sequence of the scan (host): p = m >= 1 coefficients in device memory, h and cin = ceil(m / KZG_CHUNK) elements each, q = m + 1 elements
// (q[0 .. m - 1) the quotient, q[m] = p(z); q[m - 1] is not written).  per_override = 0: the lane share of the formula; the device harness
// (tests/device/fr_edges.hip) passes other shares, any per with per * KZG_SCAN_LANES >= nchunk is valid.
inline void kzg_quotient_launch(hipStream_t stream, const Fr* p, size_t m, const Fr& z, Fr* h, Fr* cin, Fr* q, size_t per_override = 0) {
    const size_t nchunk = (m + KZG_CHUNK - 1) / KZG_CHUNK, per = per_override ? per_override : (nchunk + KZG_SCAN_LANES - 1) / KZG_SCAN_LANES;
    const Fr zT = fr_pow_u(z, KZG_CHUNK), zTper = fr_pow_u(zT, per);
    const dim3 grid((unsigned)((nchunk + 255) / 256));
    hipLaunchKernelGGL(k_kzg_chunk_sums, grid, dim3(256), 0, stream, p, (uint32_t)m, z, h);
    hipLaunchKernelGGL(k_kzg_carry_scan, dim3(1), dim3(KZG_SCAN_LANES), 0, stream, h, (uint32_t)nchunk, (uint32_t)per, zT, zTper, cin);
    hipLaunchKernelGGL(k_kzg_quotient, grid, dim3(256), 0, stream, p, (uint32_t)m, z, cin, q, q + m);
}

}  // namespace ripp
