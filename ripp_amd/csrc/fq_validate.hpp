// Bulk validation of UNTRUSTED affine points: GroupAffine::is_on_curve + is_in_correct_subgroup_assuming_on_curve of ark-ec 0.4 for a whole vector,
// one lane per point.  Every other kernel of the library assumes points of G1 / G2 proper; these kernels are how a caller establishes that.
//
// Flag per point (the first failing check wins):  0 valid (affine infinity (0, 0) included)   1 a coordinate limb value is >= p
//                                                 2 not on the curve                           3 on the curve, not in the prime-order subgroup
// Subgroup criterion, the same on both curves (u = |x| = BLS_X_ABS; DESIGN.md section 3d has the proofs):
//   G1   phi(P) = [lambda] P   with phi(x, y) = (RIPP_GLV_BETA x, y) and lambda = u^2 - 1 = RIPP_GLV_LAMBDA.  lambda^2 + lambda + 1 = u^4 - u^2 + 1 = r
//        as INTEGERS and phi^2 + phi + 1 = 0 on the whole curve, so the equation gives [r] P = O; on G1 phi acts as lambda (tools/gen_params.py checks it).
//        (With phi + 1 = -phi^2 this is the test phi^2(P) = -[x^2] P of arkworks / blst.)
//   G2   psi'(P) = [u] P       with psi' = gls_image(., 1) = sign(x) psi (the sign of x is folded into the RIPP_PSI1 constants), i.e. psi(P) = [x] P.
//        psi^2 - t psi + p = 0 on the whole twist with t = x + 1, so the equation gives [p - x] P = O, p - x = r (x - 1)^2 / 3; the order of P also divides
//        #E'(Fp2) = h2 r and gcd(h2, (x - 1)^2 / 3) = 1 on both curves, hence [r] P = O.  On G2 psi acts as x.
// Both chains are short (a 127-digit NAF of lambda, a 64-digit NAF of u) and shared by the launch, hence uniform.
//
// HOSTILE INPUT.  The throughput chains run on the incomplete carry-free formulas of fq_curve.hpp / fq_curve2.hpp (jdbl_q / jmadd_q: "accumulator not the
// identity", "T != +-Q").  Points of G1 / G2 never break those preconditions here (every intermediate is [k] P with 1 < k < r and k != +-1); points of small
// order do -- y = 0 doubles to Z = 0, a point of order 3 meets T = -Q at the first addition.  Z = 0 is absorbing in both formulas (Z3 = 2 Y Z; Z3 =
// (Z + H)^2 - Z^2 - H^2), and an addition with H = 0 reports it, so a lane whose chain left the formulas' domain ends with `bad` set or Z = 0: such a lane is
// REDONE with the complete formulas of curve.hpp (val_complete below) and never compared.  The final comparison is projective (no inversion).
#pragma once
#include "bls12_381/curve.hpp"
#include "recode.hpp"     // naf_recode

namespace ripp {

enum : uint8_t { VAL_OK = 0, VAL_RANGE = 1, VAL_CURVE = 2, VAL_SUBGROUP = 3, VAL_REDO = 0x80, VAL_GO = 0xFF };
struct ValDigits { int8_t d[132]; int len; };          // NAF of lambda (G1) or of u (G2), least significant digit first; the top digit is +1

// (host) the two digit strings
inline ValDigits val_digits(const Fp*) { constexpr uint32_t lam[8] = RIPP_GLV_LAMBDA; ValDigits v; std::memset(&v, 0, sizeof v); v.len = naf_recode(lam, 4, v.d, 130); return v; }
inline ValDigits val_digits(const Fp2*) { const uint32_t u[2] = {(uint32_t)BLS_X_ABS, (uint32_t)(BLS_X_ABS >> 32)}; ValDigits v; std::memset(&v, 0, sizeof v); v.len = naf_recode(u, 2, v.d, 130); return v; }

RIPP_HD bool val_reduced(const Fp& a) {                 // limb value < p
    uint32_t borrow = 0;
    for (int i = 0; i < 12; ++i) (void)subb32(a.l[i], FpParams::mod(i), borrow);
    return borrow != 0;
}
RIPP_HD bool val_reduced(const Fp2& a) { return val_reduced(a.c0) && val_reduced(a.c1); }
#if defined(RIPP_BLS12_377)
RIPP_HD Fp val_curve_b(const Fp*) { return Fp::one(); }                                              // y^2 = x^3 + 1
RIPP_HD Fp2 val_curve_b(const Fp2*) { return {Fp::zero(), fp_const(RIPP_FP_TWIST_B1)}; }             // D-type twist: 1 / u
#else
RIPP_HD Fp val_curve_b(const Fp*) { return dbl(dbl(Fp::one())); }                                    // y^2 = x^3 + 4
RIPP_HD Fp2 val_curve_b(const Fp2*) { const Fp b = val_curve_b((const Fp*)nullptr); return {b, b}; } // M-type twist: 4 (1 + u)
#endif
// the endomorphism image the chain's result is compared with: phi(P) on G1, gls_image(P, 1) on G2 (kernels.hpp)
RIPP_HD G1A val_endo(const G1A& p) { return {fmul(p.x, fp_const(RIPP_GLV_BETA)), p.y}; }
RIPP_HD G2A val_endo(const G2A& p) {
    const Fp2 cx = {fp_const(RIPP_PSI1_CX0), fp_const(RIPP_PSI1_CX1)}, cy = {fp_const(RIPP_PSI1_CY0), fp_const(RIPP_PSI1_CY1)};
    return {fmul(conj(p.x), cx), fmul(conj(p.y), cy)};
}
// range, identity, curve equation: a final flag, or VAL_GO for a finite curve point whose subgroup membership is still open
template <class F> RIPP_HD uint8_t val_precheck(const Affine<F>& p) {
    if (!val_reduced(p.x) || !val_reduced(p.y)) return VAL_RANGE;
    if (is_inf(p)) return VAL_OK;
    const F lhs = fsqr(p.y), rhs = add(fmul(fsqr(p.x), p.x), val_curve_b((const F*)nullptr));
    return lhs == rhs ? VAL_GO : VAL_CURVE;
}
// the whole check of one point with the COMPLETE group law (every special case of dbl / add_mixed handled): what the exceptional lanes of the
// throughput kernels are redone with, and -- host and device -- the form tests/host/validate.cpp compares with the definition [r] P = O.
template <class F> RIPP_FN uint8_t val_complete(const Affine<F>& p, const ValDigits& dg) {
    const uint8_t f = val_precheck(p);
    if (f != VAL_GO) return f;
    Jac<F> acc = jac_inf<F>();
    for (int pos = dg.len - 1; pos >= 0; --pos) {
        acc = dbl(acc);
        const int d = dg.d[pos];
        if (d != 0) { Affine<F> t = p; if (d < 0) t.y = neg(t.y); acc = add_mixed(acc, t); }
    }
    if (is_inf(acc)) return VAL_SUBGROUP;              // the image of a finite point is finite
    const Affine<F> e = val_endo(p);
    const F zz = fsqr(acc.z);
    if (!(fmul(e.x, zz) == acc.x)) return VAL_SUBGROUP;
    return fmul(e.y, fmul(zz, acc.z)) == acc.y ? VAL_OK : VAL_SUBGROUP;
}

}  // namespace ripp

#if defined(__HIPCC__)
#include "fq_curve2.hpp"

namespace ripp {

// G1: the launch shape of k_fold_g1_naf_q.  The first digit LOADS the point, so the accumulator is not the identity inside the loop unless the point has
// small order -- and then the lane is redone.
__global__ void __launch_bounds__(256, 2) k_validate_g1_q(const G1A* __restrict__ pts, uint32_t n, ValDigits dg, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
    const G1A* pp = pts + i;
    uint8_t f;
    { const G1A p = *pp; f = val_precheck(p); }
    if (f != VAL_GO) { flags[i] = f; return; }
    AffQ q; Fqn ny;
    { const G1A p = *opaque(pp); q = affq_from(p); ny = fq_reduce(fq_neg(q.y)); }
    JacQ acc; jq_set(acc, q.x, q.y, fq_one());
    bool bad = false;
#pragma unroll 1
    for (int pos = dg.len - 2; pos >= 0; --pos) {
        jdbl_q(acc);
        const int d = dg.d[pos];
        if (d != 0) bad |= jmadd_q(acc, q.x, d < 0 ? ny : q.y);
    }
    bad |= fq_is_zero(fq_reduce(acc.z));               // Z = 0 is absorbing: an identity intermediate shows here
    if (bad) { flags[i] = val_complete<Fp>(*opaque(pp), dg); return; }
    // [lambda] P = (X, Y, Z) against phi(P) = (beta x, y):  beta x Z^2 = X  and  y Z^3 = Y
    Fqn bx = fq_mul(q.x, fq_from_fp(fp_const(RIPP_GLV_BETA))); fq_pin(bx);
    Fqn zz = fq_sqr(acc.z); fq_pin(zz);
    Fqn ex = fq_mul(bx, zz); fq_pin(ex);
    const bool okx = fq_is_zero(fq_reduce(fq_sub(ex, acc.x)));
    Fqn zzz = fq_mul(zz, acc.z); fq_pin(zzz);
    Fqn ey = fq_mul(q.y, zzz); fq_pin(ey);
    const bool oky = fq_is_zero(fq_reduce(fq_sub(ey, acc.y)));
    flags[i] = okx && oky ? VAL_OK : VAL_SUBGROUP;
#endif
}

// G2: the launch shape of k_fold_g2_gls_split_q / k_pow2_mul_g2_q (64 lanes, Y1 of an addition parked in LDS).  Exceptional lanes are marked VAL_REDO and
// redone by k_validate_fix behind this kernel, so that the complete formulas' frame stays out of the throughput kernel (fq_curve2.hpp k_fold_g2_tab_q).
__global__ void __launch_bounds__(64, 2) k_validate_g2_q(const G2A* __restrict__ pts, uint32_t n, ValDigits dg, uint8_t* __restrict__ flags) {
    __shared__ uint4 park_[7 * 64];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#if defined(__HIP_DEVICE_COMPILE__)
    uint4* park = park_ + threadIdx.x;
    const G2A* bp = pts + i;
    uint8_t f;
    { const G2A p = *bp; f = val_precheck(p); }
    if (f != VAL_GO) { flags[i] = f; return; }
    JacQ2 acc; j2_set(acc, f2_from(opaque(bp)->x), f2_from(opaque(bp)->y), Fq2n{fq_one(), fq_zero()});
    f2_pin(acc.z);
    bool bad = false;
#pragma unroll 1
    for (int pos = dg.len - 2; pos >= 0; --pos) {
        jdbl2_q(acc);
        const int d = dg.d[pos];
        if (d == 0) continue;
        bad |= jmadd2_q(acc, [&]() { return f2_from(opaque(bp)->x); }, [&]() { const Fp2 y = opaque(bp)->y; return f2_from(d < 0 ? neg(y) : y); }, park);
    }
    bad |= f2_is_zero(f2_reduce(acc.z));
    if (bad) { flags[i] = VAL_REDO; return; }
    // [u] P = (X, Y, Z) against E = gls_image(P, 1):  E.x Z^2 = X  and  E.y Z^3 = Y
    Fq2n zz = f2_sqrd(acc.z); f2_pin(zz);
    bool ok;
    { const Fp2 cx = {fp_const(RIPP_PSI1_CX0), fp_const(RIPP_PSI1_CX1)};
      Fq2n ex = f2_muld(f2_from(fmul(conj(opaque(bp)->x), cx)), zz); f2_pin(ex);
      ok = f2_is_zero(f2_reduce(f2_sub(ex, acc.x))); }
    Fq2n zzz = f2_muld(zz, acc.z); f2_pin(zzz);
    { const Fp2 cy = {fp_const(RIPP_PSI1_CY0), fp_const(RIPP_PSI1_CY1)};
      Fq2n ey = f2_muld(f2_from(fmul(conj(opaque(bp)->y), cy)), zzz); f2_pin(ey);
      ok = ok && f2_is_zero(f2_reduce(f2_sub(ey, acc.y))); }
    flags[i] = ok ? VAL_OK : VAL_SUBGROUP;
#endif
}

// The lanes marked VAL_REDO, with the complete formulas: a small fixed grid walks the flag bytes 16 at a time (kernels.hpp for_flagged has the measurements
// behind that shape).  flags: 16-byte aligned and readable up to the next multiple of 16.
template <class F>
__global__ void __launch_bounds__(64) k_validate_fix(const Affine<F>* pts, uint32_t n, ValDigits dg, uint8_t* flags) {
    const uint32_t nth = gridDim.x * blockDim.x;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; (uint64_t)c * 16 < n; c += nth) {
        const uint4 w = reinterpret_cast<const uint4*>(flags)[c];
        if (((w.x | w.y | w.z | w.w) & 0x80808080u) == 0) continue;
#pragma unroll 1
        for (uint32_t k = 0; k < 16; ++k) { const uint32_t i = c * 16 + k; if (i < n && flags[i] == VAL_REDO) flags[i] = val_complete<F>(pts[i], dg); }
    }
}

}  // namespace ripp
#endif
