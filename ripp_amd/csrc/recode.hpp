// Host-side scalar recoders of the fold and scaling kernels, and the digit structs they fill (the kernels take the structs by value).
//
// Every fold first rewrites its scalar: G1 scalars split by GLV into two halves below 2^128 (s = k1 + k2 lambda), G2 scalars by GLS into four
// base-u digits (u = |x|); the pieces are recoded as NAF, width-W wNAF or cut again at bit 64, 32 or 16 for the folds with precomputed second
// bases.  Host only and free of the device runtime: besides the standard library this header needs bls12_381/fp.hpp alone, so a plain host
// compiler builds it (tests/host/recoders.cpp drives every recoder stand-alone; tests/test_recoders_cpu.py checks what it prints).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include "bls12_381/fp.hpp"

namespace ripp {

#ifndef RIPP_FOLD_W
#define RIPP_FOLD_W 5                                   // wNAF width of the table folds
#endif
constexpr int FOLD_TAB_M = 1 << (RIPP_FOLD_W - 2);      // odd multiples 1, 3, .., 2 M - 1 per base

struct ScalarBits { uint32_t w[8]; int nbits; };   // canonical little-endian scalar shared by all lanes of a launch
struct NafDigits { int8_t d[260]; int len; };          // NAF of the full-width scalar (k_fold_affine_naf)
struct GlsDigits { int8_t d[4][68]; int len; };        // string j = base-u digit j (NAF: gls_digits, width-W wNAF: gls_wnaf)
struct GlsDigits2 { GlsDigits a, b; };                 // two full-width scalars (k_vm_fold_g2_joint2)
struct GlvDigits { int8_t d1[132]; int8_t d2[132]; int len; };   // NAF strings of the GLV halves s1 / s2 (or of the two 64-bit halves: split64_digits)
struct Gls8Digits { int8_t d[8][36]; int len; };       // d[j] low, d[4 + j] high 32 bits of base-u digit j
struct Wnaf4 { int8_t d[4][36]; int len; };            // G1: string b = 32-bit word b of the 128-bit challenge
struct Wnaf16 { int8_t d[16][20]; int len; };          // G2: string 4 b + j = 16-bit piece b of GLS digit j
struct WnafG1x4 { int8_t d[16][36]; int len; };        // the sixteen strings of the fused G1 fold (fq_curve.hpp)
struct Wnaf16x3 { Wnaf16 s[3]; int len; };             // the three digit sets of the fused G2 fold (fq_curve2.hpp)
struct SplitDigits { int8_t d[8][68]; int len; };     // NAF digit strings; G1: d[0] = low half, d[1] = high half; G2: d[j] low, d[4+j] high of GLS digit j

inline ScalarBits scalar_bits(const Fr& s_mont) {
    const Fr c = from_mont(s_mont);
    ScalarBits sb; int top = -1;
    for (int i = 0; i < 8; ++i) { sb.w[i] = c.l[i]; }
    for (int i = 255; i >= 0; --i) if ((c.l[i >> 5] >> (i & 31)) & 1u) { top = i; break; }
    sb.nbits = top + 1; return sb;
}

// non-adjacent form of a little-endian multi-word integer; returns the digit count (digits[0] = least significant)
inline int naf_recode(const uint32_t* words, int nwords, int8_t* digits, int maxd) {
    uint32_t w[10] = {0};
    for (int i = 0; i < nwords; ++i) w[i] = words[i];
    auto is_zero = [&]() { for (int i = 0; i <= nwords; ++i) if (w[i]) return false; return true; };
    int n = 0;
    while (!is_zero() && n < maxd) {
        int8_t d = 0;
        if (w[0] & 1u) {
            d = (int8_t)(2 - (int)(w[0] & 3u));                // +1 if w = 1 mod 4, -1 if w = 3 mod 4
            if (d > 0) { w[0] &= ~1u; }
            else { for (int i = 0; i <= nwords; ++i) { if (++w[i] != 0) break; } }   // w += 1
        }
        digits[n++] = d;
        for (int i = 0; i < nwords; ++i) w[i] = (w[i] >> 1) | (w[i + 1] << 31);       // w >>= 1
        w[nwords] >>= 1;
    }
    return n;
}
inline NafDigits naf_digits(const Fr& s_mont) {
    const Fr c = from_mont(s_mont);
    NafDigits nd; std::memset(&nd, 0, sizeof nd);
    nd.len = naf_recode(c.l, 8, nd.d, 258);
    return nd;
}
// s = d0 + d1 u + d2 u^2 + d3 u^3 with u = |x| = 0xd201000000010000, each digit NAF-recoded
inline GlsDigits gls_digits(const Fr& s_mont) {
    const Fr c = from_mont(s_mont);
    uint64_t v[4] = {(uint64_t)c.l[0] | ((uint64_t)c.l[1] << 32), (uint64_t)c.l[2] | ((uint64_t)c.l[3] << 32),
                     (uint64_t)c.l[4] | ((uint64_t)c.l[5] << 32), (uint64_t)c.l[6] | ((uint64_t)c.l[7] << 32)};
    GlsDigits g; std::memset(&g, 0, sizeof g);
    int maxlen = 0;
    for (int j = 0; j < 4; ++j) {
        unsigned __int128 rem = 0;                             // v <- v / u, digit = v mod u
        for (int i = 3; i >= 0; --i) { const unsigned __int128 cur = (rem << 64) | v[i]; v[i] = (uint64_t)(cur / BLS_X_ABS); rem = cur % BLS_X_ABS; }
        const uint64_t dj = (uint64_t)rem;
        const uint32_t words[2] = {(uint32_t)dj, (uint32_t)(dj >> 32)};
        const int len = naf_recode(words, 2, g.d[j], 66);
        if (len > maxlen) maxlen = len;
    }
    g.len = maxlen;
    return g;
}

// s = s1 + s2 * lambda (lambda = u^2 - 1 ~ sqrt(r)) by binary long division of the canonical scalar; both halves NAF-recoded
inline void glv_split(const Fr& s_mont, uint32_t rem[9], uint32_t quo[8]) {       // s = rem + quo * lambda, both < 2^128
    const Fr c = from_mont(s_mont);
    const uint32_t lam[8] = RIPP_GLV_LAMBDA;
    for (int i = 0; i < 9; ++i) rem[i] = 0; for (int i = 0; i < 8; ++i) quo[i] = 0;
    for (int bit = 255; bit >= 0; --bit) {                      // rem = rem * 2 + bit;  if rem >= lambda: rem -= lambda, quotient bit = 1
        for (int i = 8; i > 0; --i) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 31);
        rem[0] = (rem[0] << 1) | ((c.l[bit >> 5] >> (bit & 31)) & 1u);
        bool ge = rem[8] != 0;
        if (!ge) { ge = true; for (int i = 7; i >= 0; --i) { if (rem[i] != lam[i]) { ge = rem[i] > lam[i]; break; } } }
        if (ge) { uint32_t borrow = 0; for (int i = 0; i < 8; ++i) rem[i] = subb32(rem[i], lam[i], borrow); rem[8] -= borrow; quo[bit >> 5] |= 1u << (bit & 31); }
    }
}
inline GlvDigits glv_digits(const Fr& s_mont) {
    uint32_t rem[9], quo[8]; glv_split(s_mont, rem, quo);
    GlvDigits g; std::memset(&g, 0, sizeof g);
    const int l1 = naf_recode(rem, 5, g.d1, 131), l2 = naf_recode(quo, 5, g.d2, 131);
    g.len = l1 > l2 ? l1 : l2;
    return g;
}

// digit strings of the folds with a precomputed second base (kernels.hpp, "round-0 folds")
// width-w wNAF (w = RIPP_FOLD_W) of a value < 2^64: odd digits of magnitude < 2^(w-1), at most one nonzero in any w consecutive positions
inline int wnaf4_recode(uint64_t v, int8_t* digits, int maxd, int W = RIPP_FOLD_W) {
    unsigned __int128 k = v; int len = 0;
    while (k != 0 && len < maxd) {
        int d = 0;
        if ((uint64_t)k & 1u) { d = (int)((uint64_t)k & ((1u << W) - 1)); if (d >= (1 << (W - 1))) d -= 1 << W; if (d >= 0) k -= (unsigned)d; else k += (unsigned)(-d); }
        digits[len++] = (int8_t)d;
        k >>= 1;
    }
    return len;
}
inline Wnaf4 split32_wnaf(const Fr& s_mont, int W = RIPP_FOLD_W) {    // 128-bit challenge -> width-W wNAF strings of its four 32-bit words
    const Fr c = from_mont(s_mont);
    Wnaf4 g; std::memset(&g, 0, sizeof g);
    for (int t = 0; t < 4; ++t) g.len = std::max(g.len, wnaf4_recode(c.l[t], g.d[t], 35, W));
    return g;
}
inline int tab_width(int M) { int w = 2; while ((1 << (w - 2)) < M) ++w; return w; }      // M = 2^(W - 2) odd multiples per base <-> wNAF width W
// the sixteen strings of the fused G1 fold (fq_curve.hpp k_fold_g1_fused_q): x0 | k1 | k2 | x1 with x0 x1 = k1 + k2 lambda
inline WnafG1x4 fused_digits_g1(const Fr& x0, const Fr& x1, int W) {
    WnafG1x4 g; std::memset(&g, 0, sizeof g);
    const Fr c0 = from_mont(x0), c1 = from_mont(x1);
    uint32_t rem[9], quo[8]; glv_split(mul(x0, x1), rem, quo);
    const uint32_t* src[4] = {c0.l, rem, quo, c1.l};
    for (int u = 0; u < 4; ++u) for (int b = 0; b < 4; ++b) g.len = std::max(g.len, wnaf4_recode(src[u][b], g.d[4 * u + b], 35, W));
    return g;
}
inline GlvDigits split64_digits(const Fr& s_mont) {                     // 128-bit challenge -> its two 64-bit halves
    const Fr c = from_mont(s_mont);
    GlvDigits g; std::memset(&g, 0, sizeof g);
    const int l1 = naf_recode(&c.l[0], 2, g.d1, 131), l2 = naf_recode(&c.l[2], 2, g.d2, 131);
    g.len = l1 > l2 ? l1 : l2;
    return g;
}
inline bool fits_128(const Fr& s_mont) { const Fr c = from_mont(s_mont); return (c.l[4] | c.l[5] | c.l[6] | c.l[7]) == 0; }
inline Gls8Digits gls8_digits(const Fr& s_mont) {                        // base-u digits (u = |x|), each split at bit 32
    const Fr c = from_mont(s_mont);
    uint64_t v[4] = {(uint64_t)c.l[0] | ((uint64_t)c.l[1] << 32), (uint64_t)c.l[2] | ((uint64_t)c.l[3] << 32),
                     (uint64_t)c.l[4] | ((uint64_t)c.l[5] << 32), (uint64_t)c.l[6] | ((uint64_t)c.l[7] << 32)};
    Gls8Digits g; std::memset(&g, 0, sizeof g);
    int maxlen = 0;
    for (int j = 0; j < 4; ++j) {
        unsigned __int128 rem = 0;
        for (int i = 3; i >= 0; --i) { const unsigned __int128 cur = (rem << 64) | v[i]; v[i] = (uint64_t)(cur / BLS_X_ABS); rem = cur % BLS_X_ABS; }
        const uint64_t dj = (uint64_t)rem;
        const uint32_t lo = (uint32_t)dj, hi = (uint32_t)(dj >> 32);
        const int l1 = naf_recode(&lo, 1, g.d[j], 35), l2 = naf_recode(&hi, 1, g.d[4 + j], 35);
        maxlen = std::max(maxlen, std::max(l1, l2));
    }
    g.len = maxlen;
    return g;
}

inline Wnaf16 gls16_wnaf(const Fr& s_mont, int W = RIPP_FOLD_W) {     // base-u digits, each cut into four 16-bit pieces, width-W wNAF strings
    const Fr c = from_mont(s_mont);
    uint64_t v[4] = {(uint64_t)c.l[0] | ((uint64_t)c.l[1] << 32), (uint64_t)c.l[2] | ((uint64_t)c.l[3] << 32),
                     (uint64_t)c.l[4] | ((uint64_t)c.l[5] << 32), (uint64_t)c.l[6] | ((uint64_t)c.l[7] << 32)};
    Wnaf16 g; std::memset(&g, 0, sizeof g);
    for (int j = 0; j < 4; ++j) {
        unsigned __int128 rem = 0;
        for (int i = 3; i >= 0; --i) { const unsigned __int128 cur = (rem << 64) | v[i]; v[i] = (uint64_t)(cur / BLS_X_ABS); rem = cur % BLS_X_ABS; }
        const uint64_t dj = (uint64_t)rem;
        for (int b = 0; b < 4; ++b) g.len = std::max(g.len, wnaf4_recode((dj >> (16 * b)) & 0xffffu, g.d[4 * b + j], 19, W));
    }
    return g;
}
// the three digit sets of the fused G2 fold (fq_curve2.hpp k_fold_g2_fused_q): x0 x1 (full width) | x0 | x1
inline Wnaf16x3 fused_digits_g2(const Fr& x0, const Fr& x1, int W) {
    Wnaf16x3 g; g.s[0] = gls16_wnaf(mul(x0, x1), W); g.s[1] = gls16_wnaf(x0, W); g.s[2] = gls16_wnaf(x1, W);
    g.len = std::max(g.s[0].len, std::max(g.s[1].len, g.s[2].len));
    return g;
}

inline GlsDigits gls_wnaf(const Fr& s_mont, int W) {                     // base-u digits as width-W wNAF strings (one base, in-round tables)
    const Fr c = from_mont(s_mont);
    uint64_t v[4] = {(uint64_t)c.l[0] | ((uint64_t)c.l[1] << 32), (uint64_t)c.l[2] | ((uint64_t)c.l[3] << 32),
                     (uint64_t)c.l[4] | ((uint64_t)c.l[5] << 32), (uint64_t)c.l[6] | ((uint64_t)c.l[7] << 32)};
    GlsDigits g; std::memset(&g, 0, sizeof g);
    for (int j = 0; j < 4; ++j) {
        unsigned __int128 rem = 0;
        for (int i = 3; i >= 0; --i) { const unsigned __int128 cur = (rem << 64) | v[i]; v[i] = (uint64_t)(cur / BLS_X_ABS); rem = cur % BLS_X_ABS; }
        g.len = std::max(g.len, wnaf4_recode((uint64_t)rem, g.d[j], 66, W));
    }
    return g;
}

// digit strings for vm_fold2.hpp: the same splits as split64_digits / gls8_digits in the SplitDigits layout
inline SplitDigits split_digits_g1(const Fr& s_mont) {
    const GlvDigits g = split64_digits(s_mont);
    SplitDigits d; std::memset(&d, 0, sizeof d);
    for (int i = 0; i < g.len && i < 68; ++i) { d.d[0][i] = g.d1[i]; d.d[1][i] = g.d2[i]; }
    d.len = g.len; return d;
}
inline SplitDigits split_digits_g2(const Fr& s_mont) {
    const Gls8Digits g = gls8_digits(s_mont);
    SplitDigits d; std::memset(&d, 0, sizeof d);
    for (int t = 0; t < 8; ++t) for (int i = 0; i < g.len; ++i) d.d[t][i] = g.d[t][i];
    d.len = g.len; return d;
}

// full-width G1 scalar for the second-base VM fold: GLV halves k1, k2 (< 2^128), each split at bit 64 ->
// d[0] = k1_lo (P), d[1] = k2_lo (phi P), d[2] = k1_hi (2^64 P), d[3] = k2_hi (phi 2^64 P)
inline SplitDigits split_digits_g1_glv(const Fr& s_mont) {
    uint32_t rem[9], quo[8]; glv_split(s_mont, rem, quo);
    SplitDigits d; std::memset(&d, 0, sizeof d);
    const int l0 = naf_recode(&rem[0], 2, d.d[0], 67), l1 = naf_recode(&quo[0], 2, d.d[1], 67), l2 = naf_recode(&rem[2], 2, d.d[2], 67), l3 = naf_recode(&quo[2], 2, d.d[3], 67);
    d.len = std::max(std::max(l0, l1), std::max(l2, l3)); return d;
}

}  // namespace ripp
