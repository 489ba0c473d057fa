// Digit pass of a round of TIPA<ScalarInnerProduct, PedersenCommitment<G2>, PedersenCommitment<G1>, IdentityCommitment<Fr>>
// (ip_proofs/src/tipa/mod.rs:499-526; tipa_scalar_api.inc): the round's TWO G2 Pedersen commitments (gipa.rs:209-231, h = len / 2)
//     com_1.0 = <ck_a[:h], m_a[h:]>      com_2.0 = <ck_a[h:], m_a[:h]>
// as rows 0 and 1 of ONE pass of the batched MSM pipeline (msm_batch.hpp) over the WHOLE key vector, in its G2 form: every term splits four ways
// over the psi endomorphism, k = d0 + d1 u + d2 u^2 + d3 u^3 in base u = |x| (msm.hpp k_msm_digits, the GLS branch), term j * nreal + i carries d_j
// on [u^j] base i.  The other half of each row is zero digits, which sort into no bucket; the sort, the gathered additions over ONE extended array
// of the keys (k_msm_extend_q<Fp2> with split 4), the reductions and the Horner finish run unchanged over 2 x nwin virtual windows.
#pragma once
#include "msm_batch.hpp"

namespace ripp {

// p: the plan of one row over p.nreal = 2 h bases (p.n = 8 h terms).  grid = (ceil(2 h / 256), 2); row r writes its digits at digits + r * p.nwin * p.n.
// Row 0 carries m[h + i] at base i < h, row 1 carries m[i - h] at base h <= i < 2 h.
__global__ void __launch_bounds__(256) k_tipa_scalar_digits_cross_g2(const Fr* __restrict__ m, uint32_t h, MsmPlan p, uint16_t* __restrict__ digits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (i >= p.nreal) return;
    uint16_t* const dg = digits + (size_t)r * (size_t)p.nwin * p.n;
    Fr k = Fr::zero();
    if (r == 0) { if (i < h) k = from_mont(m[h + i]); }
    else if (i >= h && i < 2 * h) k = from_mont(m[i - h]);
    const uint32_t u[2] = RIPP_X_ABS_LIMBS;
    const uint32_t u_mu[7] = RIPP_X_ABS_MU;                                          // floor(2^256 / |x|)
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
        uint32_t rem[3];
        msm_divmod<2, 7>(k.l, u, u_mu, rem);
        msm_emit_digits(rem, 3, j * p.nreal + i, p, dg, nullptr);
    }
    msm_emit_digits(k.l, 8, 3 * p.nreal + i, p, dg, nullptr);                       // k < r < u^4: the last quotient is the top digit
}

}  // namespace ripp
