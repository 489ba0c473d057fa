// Kernels of the first tier of the transparent polynomial commitment (ip_proofs/src/applications/poly_commit/transparent.rs:43-48):
//   GIPAWithSSM<ScalarInnerProduct, PedersenCommitment<G1>, IdentityCommitment<Fr>>, a scalar message m folded against G1 keys ck and the
//   structured scalars b.  Per round (gipa.rs:207-291), h = len / 2:
//     com_1 = (<ck[:h], m[h:]>, 0, <m[h:], b[:h]>)      com_2 = (<ck[h:], m[:h]>, 0, <m[:h], b[h:]>)
//     m <- c m[h:] + m[:h]      b <- c^-1 b[h:] + b[:h]      ck <- c^-1 ck[h:] + ck[:h]
//
//   k_tpc_digits_cross   digit pass of the batched MSM pipeline (msm_batch.hpp) for the round's TWO Pedersen commitments as rows 0 and 1 over the
//                        WHOLE key vector: row 0 carries m[h + i] at base i < h, row 1 carries m[i] at base h + i; the other half of each row is
//                        zero digits, which sort into no bucket.  Everything after the digit pass runs unchanged.
//   k_fr_dot2            both inner products of the round from the crossed halves, one partial per (block, product)
//   k_fold_fr2           both scalar folds of the round
#pragma once
#include "msm_batch.hpp"

namespace ripp {

// p: the plan of one row over p.nreal = 2 h bases.  grid = (ceil(2 h / 256), 2); row r writes its digits at digits + r * p.nwin * p.n.
__global__ void __launch_bounds__(256) k_tpc_digits_cross(const Fr* __restrict__ m, uint32_t h, MsmPlan p, uint16_t* __restrict__ digits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (i >= p.nreal) return;
    uint16_t* const dg = digits + (size_t)r * (size_t)p.nwin * p.n;
    Fr k = Fr::zero();
    if (r == 0) { if (i < h) k = from_mont(m[h + i]); }
    else if (i >= h && i < 2 * h) k = from_mont(m[i - h]);
    const uint32_t lam[8] = RIPP_GLV_LAMBDA;
    const uint32_t lam_mu[5] = RIPP_GLV_LAMBDA_MU;
    uint32_t rem[5];
    msm_divmod<4, 5>(k.l, lam, lam_mu, rem);                                          // k = q * lambda + rem, both < 2^128 (msm.hpp k_msm_digits)
    msm_emit_digits(rem, 5, i, p, dg, nullptr);
    msm_emit_digits(k.l, 8, p.nreal + i, p, dg, nullptr);
}

// partials[y * gridDim.x + x]: y = 0 the block sums of <m[h:], b[:h]>, y = 1 those of <m[:h], b[h:]> (the host adds the <= 2 x 1024 partials, as for k_fr_dot)
__global__ void __launch_bounds__(256) k_fr_dot2(const Fr* __restrict__ m, const Fr* __restrict__ b, uint32_t h, Fr* __restrict__ partials) {
    __shared__ Fr sh[256];
    const Fr* const l = blockIdx.y == 0 ? m + h : m;
    const Fr* const r = blockIdx.y == 0 ? b : b + h;
    Fr acc = Fr::zero();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < h; i += gridDim.x * blockDim.x) acc = add(acc, mul(l[i], r[i]));
    sh[threadIdx.x] = acc; __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) sh[threadIdx.x] = add(sh[threadIdx.x], sh[threadIdx.x + s]); __syncthreads(); }
    if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// grid = (ceil(h / 256), 2): y = 0  m_out[i] = c m[h + i] + m[i],  y = 1  b_out[i] = c_inv b[h + i] + b[i]   (gipa.rs:262-275)
__global__ void __launch_bounds__(256) k_fold_fr2(const Fr* __restrict__ m, const Fr* __restrict__ b, uint32_t h, Fr c, Fr c_inv, Fr* __restrict__ m_out, Fr* __restrict__ b_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h) return;
    if (blockIdx.y == 0) m_out[i] = add(mul(m[h + i], c), m[i]);
    else b_out[i] = add(mul(b[h + i], c_inv), b[i]);
}

}  // namespace ripp
