// Digit pass of a round of GIPA<MultiexponentiationInnerProduct<G1>, AFGHOCommitmentG1, PedersenCommitment<G1>, IdentityCommitment<G1>>
// (ip_proofs/src/gipa.rs:499-530; gipa_mexp_api.inc): the round's FOUR G1 MSMs as rows of ONE pass of the batched pipeline (msm_batch.hpp).
//
// The Pedersen key ck_b and the message m_a of the round (len elements each, h = len / 2) lie side by side in one base array
//     X[0 : len] = ck_b          X[len : 2 len] = m_a
// and every MSM of the round (gipa.rs:209-231) is a row over ALL 2 len bases with the scalars of one half of m_b at one half of one vector:
//     row 0   com_1.1 = <ck_b[h:], m_b[:h]>      m_b[i]     at base           h + i
//     row 1   com_1.2 = <m_a[h:],  m_b[:h]>      m_b[i]     at base     len + h + i
//     row 2   com_2.1 = <ck_b[:h], m_b[h:]>      m_b[h + i] at base               i
//     row 3   com_2.2 = <m_a[:h],  m_b[h:]>      m_b[h + i] at base         len + i
// Every other digit is zero and sorts into no bucket, so the sort, the gathered additions and the reductions run unchanged over 4 x nwin virtual
// windows and gather from ONE extended array of X, built once per round.  Each scalar is used by two rows: it is brought out of Montgomery form and
// split through the endomorphism ONCE.
#pragma once
#include "msm_batch.hpp"

namespace ripp {

__device__ __forceinline__ void gipa_mexp_zero_digits(uint32_t i, const MsmPlan& p, uint16_t* __restrict__ digits) {
    for (int w = 0; w < p.nwin; ++w) digits[(size_t)w * p.n + i] = 0;
}

// p: the plan of one row over p.nreal = 2 len bases (p.n = 4 len terms).  One lane per scalar of m_b, grid = ceil(len / 256).  Lane t owns the base
// positions t and len + t of all four rows (both GLV halves of each: 16 digit columns), so the lanes together write every digit of the pass exactly once:
//     t >= h   m_b[t - h] at position t of row 0 and at position len + t of row 1
//     t <  h   m_b[t + h] at position t of row 2 and at position len + t of row 3
// Row r writes at digits + r * p.nwin * p.n; the GLV quotient of position i is term p.nreal + i.
__global__ void __launch_bounds__(256) k_gipa_mexp_digits(const Fr* __restrict__ m_b, uint32_t len, MsmPlan p, uint16_t* __restrict__ digits) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= len) return;
    const uint32_t h = len >> 1;
    const bool upper = t >= h;
    Fr k = from_mont(m_b[upper ? t - h : t + h]);
    const uint32_t lam[8] = RIPP_GLV_LAMBDA;
    const uint32_t lam_mu[5] = RIPP_GLV_LAMBDA_MU;
    uint32_t rem[5];
    msm_divmod<4, 5>(k.l, lam, lam_mu, rem);                                          // k = q * lambda + rem, both < 2^128 (msm.hpp k_msm_digits)
    const uint32_t live = upper ? 0u : 2u;                                            // the row that carries the scalar at position t; row live + 1 carries it at len + t
    const size_t row = (size_t)p.nwin * p.n;
#pragma unroll 1
    for (uint32_t r = 0; r < 4; ++r) {
        uint16_t* const dg = digits + r * row;
#pragma unroll 1
        for (uint32_t s = 0; s < 2; ++s) {
            const uint32_t pos = s ? len + t : t;
            if (r == live + s) { msm_emit_digits(rem, 5, pos, p, dg, nullptr); msm_emit_digits(k.l, 8, p.nreal + pos, p, dg, nullptr); }
            else { gipa_mexp_zero_digits(pos, p, dg); gipa_mexp_zero_digits(p.nreal + pos, p, dg); }
        }
    }
}

}  // namespace ripp
