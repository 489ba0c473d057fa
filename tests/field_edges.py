"""Cases and expected values for the device harness tests/device/field_edges.hip (TEST INFRASTRUCTURE ONLY).

Every case is built legal by construction for the type it is fed to -- Fq<LM, VB>: 14 limbs of 28 bits, every limb < LM, value < VB p
(ripp_amd/csrc/fq28.hpp) -- and `check_type` asserts it again before the case reaches the device, so a failure on the device means a kernel bug,
never a test that fed a forbidden value.  Expected values are Python integers from the models' P and R' = 2^392.

`lk_model` replays the signed 64-bit column sums of k_line_products_k (ripp_amd/csrc/fq_line_products_k.hpp) exactly, to measure the column
margin and the range of its reduced values on the cases the GPU test runs.
"""
import random

import bls377_model as m377
import bls381_model as m381

NL, W = 14, 28
MASK = (1 << W) - 1
RP = 1 << 392                      # R': the Montgomery radix of the carry-free form
L28 = 1 << 28
LWIDE = (1 << 32) - 16


class Curve:
    def __init__(self, tag, model):
        self.tag, self.m, self.P = tag, model, model.P
        self.P_TOP = self.P >> 364
        self.P28 = to_limbs(self.P)
        self.INV28 = (-pow(self.P, -1, 1 << W)) % (1 << W)
        self.RINV = pow(RP, -1, self.P)
        self.ONE = RP % self.P

    def mont(self, x): return x * RP % self.P           # a field element -> its Montgomery-392 integer
    def unmont(self, x): return x * self.RINV % self.P


# ---- limbs ------------------------------------------------------------------------------------------------------------------------------------
def to_limbs(v):
    """normalised limbs of 0 <= v (the top limb keeps the rest)"""
    assert v >= 0
    return [(v >> (W * i)) & MASK for i in range(NL - 1)] + [v >> (W * (NL - 1))]


def value(limbs):
    return sum(int(l) << (W * i) for i, l in enumerate(limbs))


def largest_limbs(v, LM):
    """the 14 limbs that sum to v, each < LM, with every low limb pushed as high as it can go (greedy from limb 0: the largest
    t <= min(LM - 1, rest) with t = rest mod 2^28); the top limb keeps what is left"""
    assert v >= 0 and LM >= L28
    out, rest = [], v
    for _ in range(NL - 1):
        hi = min(LM - 1, rest)
        t = hi - ((hi - rest) % L28)           # largest t <= hi with t = rest (mod 2^28)
        out.append(t)
        rest = (rest - t) >> W
    out.append(rest)
    assert value(out) == v
    return out


def check_type(limbs, LM, VB, P):
    """the case is a legal Fq<LM, VB>: every limb < LM, value < VB p, every limb a u32"""
    assert len(limbs) == NL
    assert all(0 <= l < LM and l < (1 << 32) for l in limbs), "limb bound"
    assert value(limbs) < VB * P, "value bound"
    return limbs


def words12(v):
    assert 0 <= v < 1 << 384
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(12)]


def from_words(ws): return sum(int(w) << (32 * j) for j, w in enumerate(ws))


CURVES = {"381": Curve("381", m381), "377": Curve("377", m377)}


# ---- the harness's instantiation tables (tests/device/field_edges.hip FE_*_LIST; the GPU test checks them against fe_bounds) ------------------
# Each entry mirrors an engine type; when an engine bound widens, the entry below it must follow (these tests keep passing at the old bound otherwise).
# REDUCE (fq_reduce, fq_norm): 4 fq_reduce(fq_neg(Fqn)) and fq_coord (fq_curve.hpp k_fold_*_q, fq_curve2.hpp gls loady); 8 / 19 / 36 the JZ / JY / JX
#   slots in jacq_to_g1j; 256 fq_from_fp_fast (fq_unpack_shl8); (2^29, 258) FqTabY; 7 / 11 / 14 f2_lazy of H, X3, r in jmadd2_q (BLS12-377) and
#   the Fq2X slot (BLS12-381) in f2_to; 44 rr of jmadd_q; (2^32 - 16, 2500) the widest type fq_reduce and fq_norm accept.
# SUB (fq_sub / fq_neg subtrahends): 2 every product (A, C, J, V, HH, Z1Z1); 4 Fq2C slots (BLS12-377); 8 JZ; 11 X3 of jmadd_q / Fq2X; 16 D of jdbl_q;
#   19 JY; 36 JX; 256 fq_tab_y; (8 (2^28 - 1) + 1, 16) 8C of jdbl_q; (2^29 - 1, 38) 2 Y1 in fq_mul_sub; (5 (2^28 - 1) + 1, 20) and
#   (5 (2^29 - 2) + 1, 40) fq_mul_beta of a coordinate / a doubled value (BLS12-377 f2_muld, f2_sqrd); (4 (2^28 - 1) + 1, 8) I = 4 HH;
#   (14 2^28 - 13, 1000) the widest subtrahend whose difference keeps 32-bit limbs.
# MUL / SQR / DOT / MULSUB: the widest products of jdbl_q and jmadd_q -- table x2 Z1Z1, table y2 Z1, H I, E (D - X3), Y Z, X I, rr^2, (Z + H)^2, the
#   two-product Y3 of fq_mul_sub -- plus the extremes the static checks admit (4 2^28 limbs on both sides, V1 V2 = VMAX).
# F2MUL / F2SQR / F2MULSUB / F2MULFQ: the Fp2 products of jdbl2_q, jmadd2_q and the Miller line evaluation (fq_miller.hpp f2_mul_fq) per curve.
REDUCE = [(L28, 4), (L28, 8), (L28, 19), (L28, 36), (L28, 256), (1 << 29, 258), (L28, 7), (L28, 11), (L28, 14), (L28, 44), (LWIDE, 2500)]
SUB = [(L28, 2), (L28, 4), (L28, 8), (L28, 11), (L28, 16), (L28, 19), (L28, 36), (L28, 256), (8 * (L28 - 1) + 1, 16), ((1 << 29) - 1, 38),
       (5 * (L28 - 1) + 1, 20), (4 * (L28 - 1) + 1, 8), (5 * ((1 << 29) - 2) + 1, 40), (14 * L28 - 13, 1000)]
MUL = [((L28, 2), (L28, 2)), ((L28, 256), (L28, 2)), ((1 << 29, 258), (L28, 8)), ((4 * (L28 - 1) + 1, 8), (L28, 39)),
       ((3 * (L28 - 1) + 1, 6), (3 * L28 - 1, 53)), ((L28, 19), (L28, 8)), ((L28, 36), (4 * (L28 - 1) + 1, 8)),
       ((4 * (L28 - 1) + 1, 8), (4 * (L28 - 1) + 1, 8)), ((L28, 1250), (L28, 2))]
SQR = [(L28, 2), (L28, 36), ((1 << 29) - 1, 38), (3 * (L28 - 1) + 1, 6), (L28, 44), ((1 << 29) - 1, 47), (L28, 50), (4 * (L28 - 1) + 1, 8)]
DOT2 = [((3 * L28, 44), (L28, 14)), (((1 << 29) - 1, 8), ((1 << 29) - 1, 8)), ((L28, 625), (L28, 2))]
DOT4 = [((3 * L28, 22), (L28, 14)), ((L28, 312), (L28, 2))]
MULSUB = [((L28, 44), (L28, 14), ((1 << 29) - 1, 38), (L28, 2)), ((L28, 2), (L28, 2), (L28, 2), (L28, 2))]
F2MUL = {"377": [((L28, 2), (L28, 2)), ((4 * (L28 - 1) + 1, 8), (L28, 2)), ((L28, 4), (4 * (L28 - 1) + 1, 8)), ((L28, 4), (L28, 14)),
                 ((8 * (L28 - 1) + 1, 16), (L28, 2))],
         "381": [((L28, 2), (L28, 2)), ((L28, 256), (L28, 2)), ((1 << 29, 258), (L28, 2)), ((L28, 14), (4 * (L28 - 1) + 1, 8)),
                 ((L28, 11), (4 * (L28 - 1) + 1, 8)), ((L28, 6), (L28, 19)), ((L28, 7), (L28, 8))]}
F2SQR = {"377": [(L28, 2), (L28, 4), (L28, 6), (L28, 12)], "381": [(L28, 2), (L28, 11), (L28, 7), (L28, 13), (L28, 22), (L28, 20), (L28, 8)]}
F2MULSUB = {"377": [], "381": [((L28, 20), (L28, 14), ((1 << 29) - 1, 4), (L28, 7))]}
F2MULFQ = [((L28, 2), (L28, 2)), ((L28, 4), (L28, 256)), ((3 * (L28 - 1) + 1, 6), (L28, 4))]


def table(kind, tag):
    """the Python side of fe_bounds(kind, id): a list of operand (LM, VB) tuples per instantiation"""
    one = lambda lst: [[x] for x in lst]
    return {0: one(REDUCE), 1: one(REDUCE), 2: one(SUB), 3: [list(x) for x in MUL], 4: one(SQR), 5: [list(x) for x in DOT2], 6: [list(x) for x in DOT4],
            7: [list(x) for x in MULSUB], 8: [list(x) for x in F2MUL[tag]], 9: one(F2SQR[tag]), 10: [list(x) for x in F2MULSUB[tag]],
            11: [list(x) for x in F2MULFQ]}[kind]


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
def edge_values(C, VB):
    """VB p - 1, 0 and p: the operand values at the bound, at zero and at the modulus"""
    return [VB * C.P - 1, 0, C.P]


def reduce_inputs(C, VB):
    """k p - 1, k p, k p + 1, k p + 2^364 - 1 for every k below the bound (values < VB p)"""
    out = []
    for k in range(VB):
        for d in (-1, 0, 1, (1 << 364) - 1):
            v = k * C.P + d
            if 0 <= v < VB * C.P:
                out.append((k, d, v))
    return out


def operand(C, v, LM, VB):
    """v < VB p as a legal Fq<LM, VB> in largest-limb form"""
    return check_type(largest_limbs(v, LM), LM, VB, C.P)


def subtrahend_max(C, L2, V2):
    """the largest subtrahend Fq<L2, V2> admits limb by limb: every low limb at L2 - 1 and the top limb as large as V2 p allows"""
    low = sum((L2 - 1) << (W * i) for i in range(NL - 1))
    top = (V2 * C.P - 1 - low) >> (W * (NL - 1))
    assert top >= 0
    return check_type([L2 - 1] * (NL - 1) + [top], L2, V2, C.P)


def storage_values(C, rng):
    P = C.P
    vals = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2]
    vals += [P - (1 << k) for k in (1, 8, 27, 28, 29, 31, 32, 33, 63, 64, 200, 364, 370, 376)]
    for b in range(28, 384, 28):               # every 28-bit boundary straddled: bits b-2 .. b+1 set / the low bits set
        vals += [(0xF << (b - 2)), (1 << b) - 1]
    for b in range(32, 384, 32):               # every 32-bit boundary
        vals += [(0xF << (b - 2)), (1 << b) - 1]
    vals += [sum(MASK << (W * i) for i in range(0, 13, 2)) % P, sum(0xFFFFFFFF << (64 * i) for i in range(6)) % P]
    vals += [rng.randrange(P) for _ in range(16)]
    return [v for v in vals if 0 <= v < P]


def line_coeff_values(C, rng):
    """canonical line coefficients chosen to be extreme"""
    P = C.P
    vals = [0, 1, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, (1 << 364) - 1, sum(MASK << (W * i) for i in range(0, 14, 2)) % P,
            sum(MASK << (W * i) for i in range(1, 14, 2)) % P]
    vals += [P - (1 << k) for k in (1, 27, 28, 56, 200, 363)]
    return [v % P for v in vals], [rng.randrange(P) for _ in range(8)]


# ---- Fp2 / Fp12 helpers ----------------------------------------------------------------------------------------------------------------------
def f2_expect_mul(C, a, b):
    """a, b: (c0, c1) Montgomery integers -> Montgomery integer pair of the product (u^2 = -beta)"""
    r = C.m.f2mul((C.unmont(a[0]), C.unmont(a[1])), (C.unmont(b[0]), C.unmont(b[1])))
    return (C.mont(r[0]), C.mont(r[1]))


def line_element(C, l):
    """stage 1's line (l0, l1, l2) of Fp2 values -> the flat w-basis element (M-type: l0 + l1 w^2 + l2 w^3; D-type: l0 + l1 w + l2 w^3)"""
    z = (0, 0)
    if C.tag == "381":
        return [l[0], z, l[1], l[2], z, z]
    return [l[0], l[1], z, l[2], z, z]


def expected_accumulator(C, lines):
    """what one accumulator of stage 2a holds after the given lines (each: 6 canonical integers = the 12 words as stage 1 stored them), as 6 tower-order
    Fp2 values of canonical integers: the words of a line ARE Montgomery-392 integers, the accumulator starts at one (R' mod p)"""
    acc = [(1, 0)] + [(0, 0)] * 5
    for ws in lines:
        l = [(C.unmont(ws[2 * f]), C.unmont(ws[2 * f + 1])) for f in range(3)]
        acc = C.m.f12mul(acc, line_element(C, l))
    return [(C.mont(c[0]), C.mont(c[1])) for c in C.m.f12_to_tower(acc)]


# ---- the signed column sums of k_line_products_k, replayed -------------------------------------------------------------------------------------
class LkStats:
    def __init__(self): self.col_max, self.vmin, self.vmax = 0, 0.0, 0.0


def _conv_add(col, x, y, st):
    """col += x (*) y row by row, as lk_mads1 / lk_mads2 accumulate (recording the largest partial column)"""
    for i in range(NL):
        xi = x[i]
        if xi == 0:
            continue
        for j in range(NL):
            col[i + j] += xi * y[j]
        m = max(abs(c) for c in col)
        if m > st.col_max: st.col_max = m


def lk_reduce(C, col, st):
    """lk_reduce_cols: signed Montgomery reduction of 27 columns; limbs 0..12 in [0, 2^28), limb 13 signed"""
    col = list(col)
    carry = 0
    for k in range(NL):
        s = col[k] + carry
        m = ((s & 0xFFFFFFFF) * C.INV28) & MASK
        for jj in range(1, NL):
            col[k + jj] += m * C.P28[jj]
            st.col_max = max(st.col_max, abs(col[k + jj]))
        s += m * C.P28[0]
        st.col_max = max(st.col_max, abs(s))
        assert s & MASK == 0
        carry = s >> W
    r = []
    for k in range(NL, 2 * NL - 1):
        s = col[k] + carry
        st.col_max = max(st.col_max, abs(s))
        r.append(s & MASK)
        carry = s >> W
    r.append(carry)
    return r


def _signed_value(l): return sum(v << (W * i) for i, v in enumerate(l))


def lk_model(C, lines, st, finals=None):
    """one accumulator of k_line_products_k over `lines` (6 canonical integers each): returns the 6 tower-order canonical Fp2 outputs and
    updates `st` with the largest |column| met and the range of the reduced values (in units of p); `finals` receives the 12 signed values the kernel
    makes canonical at its write-out (+ p, then up to two subtractions of p)"""
    P = C.P
    f = [[to_limbs(C.ONE), [0] * NL]] + [[[0] * NL, [0] * NL] for _ in range(5)]
    for ws in lines:
        # the line values of one group (fq_line_products_k.hpp build_y): per coefficient -c0, -c1, c0 + c1 and xi's images c1 - c0, -(c0 + c1), 2 c0
        units = {}
        for tc, base in ((0, 0), (1, 3), (2, 9)):
            c0, c1 = to_limbs(ws[2 * tc]), to_limbs(ws[2 * tc + 1])
            s = to_limbs(ws[2 * tc] + ws[2 * tc + 1])
            units[base] = [-x for x in c0]; units[base + 1] = [-x for x in c1]; units[base + 2] = s
            if tc:
                units[base + 3] = [b - a for a, b in zip(c0, c1)]; units[base + 4] = [-x for x in s]
                units[base + 5] = to_limbs(2 * ws[2 * tc])
        new = []
        for k in range(6):
            terms = [(f[k], 0), (f[(k + 4) % 6], 3 + (3 if k < 2 else 0)), (f[(k + 3) % 6], 9 + (3 if k < 3 else 0))]
            U, V = [0] * (2 * NL - 1), [0] * (2 * NL - 1)
            for x, u in terms:
                _conv_add(U, x[0], units[u], st)
                _conv_add(V, x[1], units[u + 1], st)
            U, V = [a + b for a, b in zip(U, V)], [b - a for a, b in zip(U, V)]
            st.col_max = max(st.col_max, max(abs(c) for c in U + V))
            re = lk_reduce(C, V, st)
            for x, u in terms:
                _conv_add(U, [a + b for a, b in zip(x[0], x[1])], units[u + 2], st)
            im = lk_reduce(C, U, st)
            for r in (re, im):
                v = _signed_value(r) / P
                st.vmin, st.vmax = min(st.vmin, v), max(st.vmax, v)
                assert -(1 << 31) <= r[-1] < (1 << 31)
            new.append([re, im])
        f = new
    tower = [0, 2, 4, 1, 3, 5]
    if finals is not None:
        finals.extend(_signed_value(f[k][part]) for k in tower for part in (0, 1))
    return [tuple(_signed_value(f[k][part]) % P for part in (0, 1)) for k in tower]


# ---- stage-2a cases: (M, T, rows) and the line buffer ------------------------------------------------------------------------------------------
LP_SHAPES = [(2, 1, 1), (3, 1, 2), (30, 10, 1), (20, 10, 2), (5, 7, 1), (23, 10, 1), (40, 13, 3), (45, 21, 1), (50, 22, 2)]


def lp_lines(C, M, rows, seed):
    """rows x M lines of 6 canonical coefficients: extreme values in rotating combinations, every few lines a random one"""
    rng = random.Random(seed)
    ext, rnd = line_coeff_values(C, rng)
    out = []
    for r in range(rows):
        row = []
        for i in range(M):
            if (i + r) % 5 == 4:
                row.append([rng.choice(rnd) for _ in range(6)])
            else:
                row.append([ext[(i * 7 + f * 3 + r * 11 + (i * f) % 5) % len(ext)] for f in range(6)])
        out.append(row)
    return out


# line pairs (one accumulator each) whose final reduced values in k_line_products_k reach [p, 1.01 p): the write-out needs its SECOND subtraction of p
# there (found by a search with lk_model over the seeds below; test_field_edges_cpu.py checks that they still do)
LP_HIGH_SEEDS = [166, 190, 195, 217, 335, 343]


def lp_high_lines(C, seed):
    rng = random.Random(seed)
    ext, rnd = line_coeff_values(C, random.Random(seed ^ 0x5A5A))
    pool = ext + rnd
    return [[rng.choice(pool) for _ in range(6)] for _ in range(2)]


def lp_extreme_sequences(C):
    """two- and three-line sequences on ONE accumulator with every coefficient of every line at an extreme, so that after the first line both Karatsuba operands
    (accumulator and line) sit at the extremes: every low limb at 2^28 - 1 (2^364 - 1, the largest column of k_line_products_k: lk_model), alternating
    0 / 2^28 - 1 limbs in both phases, and p - 1"""
    P = C.P
    top = (1 << 364) - 1
    ev = sum(MASK << (W * i) for i in range(0, NL, 2)) % P
    od = sum(MASK << (W * i) for i in range(1, NL, 2)) % P
    return {"top2": [[top] * 6] * 2, "top3": [[top] * 6] * 3, "alt2": [[ev, od] * 3] * 2, "alt3": [[ev, od] * 3] * 3, "altr3": [[od, ev] * 3] * 3,
            "pm1_3": [[P - 1] * 6] * 3}
