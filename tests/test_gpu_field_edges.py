"""GPU (-m gpu): the carry-free field arithmetic, its group law and stage 2a of the pairing product AT THEIR BOUNDS, through the device harness
tests/device/field_edges.hip (built from the production headers by build(): tests/device/build/libfield_edges_{381,377}.so).

Every case is a legal value of the type it is fed to, built in tests/field_edges.py at the extremes the type admits (largest-limb forms, k p - 1 .. k p + 2^364 - 1,
the largest subtrahend, table bounds, lifted Jacobian coordinates); every result is checked against Python integers: its own bound claims (limbs, value) and
its value mod p."""
import ctypes
import os
import random

import numpy as np
import pytest

import field_edges as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = ["381", "377"]
U32P = ctypes.POINTER(ctypes.c_uint32)


class Harness:
    def __init__(self, tag):
        path = os.path.join(HERE, "device", "build", "libfield_edges_%s.so" % tag)
        assert os.path.exists(path), "device harness missing: %s (build() builds it: make -C tests/device)" % path
        self.lib = ctypes.CDLL(path)
        self.tag, self.C = tag, F.CURVES[tag]
        self.lib.fe_line_products.argtypes = [ctypes.c_int, U32P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, U32P]
        assert self.lib.fe_curve() == int(tag)

    def call(self, name, *args):
        conv = []
        for a in args:
            if isinstance(a, np.ndarray):
                assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
                conv.append(a.ctypes.data_as(U32P))
            else:
                conv.append(a)
        rc = getattr(self.lib, name)(*conv)
        assert rc == 0, "%s returned %d" % (name, rc)


@pytest.fixture(scope="module")
def H(engine):
    return {t: Harness(t) for t in CURVES}


def arr(rows, width):
    a = np.zeros((len(rows), width), dtype=np.uint32)
    for i, r in enumerate(rows):
        a[i, :len(r)] = r
    return a


def limbs_ok(row, P, VB=2):
    """a reduced value: every limb < 2^28, value < VB p"""
    return all(int(x) <= F.MASK for x in row) and F.value(row) < VB * P


def sub_lm(L1, L2):
    """the limb bound fq_sub's result type claims (fq28.hpp sub_lm)"""
    B = ((L2 + F.MASK) >> F.W) << F.W
    while B - (B >> F.W) + 1 < L2:
        B += 1 << F.W
    return L1 + F.MASK + B


# ---- tables -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CURVES)
def test_instantiation_tables_match(H, tag):
    h = H[tag]
    for kind in range(12):
        tab = F.table(kind, tag)
        assert h.lib.fe_count(kind) == len(tab), kind
        for i, ops in enumerate(tab):
            lv = (ctypes.c_uint64 * 8)()
            assert h.lib.fe_bounds(kind, i, lv) == 0
            assert [(lv[2 * j], lv[2 * j + 1]) for j in range(len(ops))] == [tuple(o) for o in ops], (kind, i)


# ---- a. reduction and zero test ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CURVES)
def test_reduce_and_is_zero_at_every_bound(H, tag):
    h, C = H[tag], H[tag].C
    P = C.P
    for rid, (LM, VB) in enumerate(F.REDUCE):
        cases = []
        for k, d, v in F.reduce_inputs(C, VB):
            cases.append((v, F.check_type(F.to_limbs(v), LM, VB, P)))
            if LM > F.L28:                                 # (at LM = 2^28 the largest-limb form is the normalised one)
                cases.append((v, F.operand(C, v, LM, VB)))
        a = arr([c[1] for c in cases], 14)
        out, flag = np.zeros_like(a), np.zeros(len(cases), dtype=np.uint32)
        h.call("fe_reduce", rid, a, out, flag, len(cases))
        for (v, _), o, z in zip(cases, out, flag):
            assert limbs_ok(o, P), (LM, VB, hex(v))
            assert F.value(o) % P == v % P, (LM, VB, hex(v))
            assert bool(z) == (v % P == 0), ("fq_is_zero", LM, VB, hex(v))


# ---- b. fq_canon, fq_is_zero and fq_norm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CURVES)
def test_canon_and_is_zero(H, tag):
    h, P = H[tag], H[tag].C.P
    vals = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2, P - 2, P + 2]
    a = arr([F.to_limbs(v) for v in vals], 14)
    out, flag = np.zeros_like(a), np.zeros(len(vals), dtype=np.uint32)
    h.call("fe_canon", a, out, flag, len(vals))
    for v, o, z in zip(vals, out, flag):
        assert [int(x) for x in o] == F.to_limbs(v % P), hex(v)
        assert bool(z) == (v % P == 0), hex(v)


@pytest.mark.parametrize("tag", CURVES)
def test_norm_largest_limb_forms(H, tag):
    h, C = H[tag], H[tag].C
    rng = random.Random(5)
    for rid, (LM, VB) in enumerate(F.REDUCE):
        vals = F.edge_values(C, VB) + [VB * C.P - 1 - (1 << 364), (VB - 1) * C.P] + [rng.randrange(VB * C.P) for _ in range(8)]
        a = arr([F.operand(C, v, LM, VB) for v in vals], 14)
        out = np.zeros_like(a)
        h.call("fe_norm", rid, a, out, len(vals))
        for v, o in zip(vals, out):
            assert F.value(o) == v and all(int(x) <= F.MASK for x in o), (LM, VB, hex(v))


# ---- c. subtraction with the largest subtrahend -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CURVES)
def test_sub_largest_subtrahend(H, tag):
    h, C = H[tag], H[tag].C
    P = C.P
    for sid, (L2, V2) in enumerate(F.SUB):
        bs = [F.subtrahend_max(C, L2, V2)] + [F.operand(C, v, L2, V2) for v in F.edge_values(C, V2)]
        a = arr(bs, 14)
        out = np.zeros((len(bs), 56), dtype=np.uint32)
        h.call("fe_sub", sid, a, out, len(bs))
        for b, o in zip(bs, out):
            vb = F.value(b)
            for part, L1 in ((o[0:14], 1), (o[14:28], F.L28), (o[28:42], F.L28), (o[42:56], F.L28)):
                # no limb wrapped: the limbs add up to exactly (V2 + 1) p - b (K's value), each below the result type's limb bound
                assert F.value(part) == (V2 + 1) * P - vb, ("limb wrapped", L2, V2, [hex(int(x)) for x in part])
                assert all(int(x) < sub_lm(L1, L2) for x in part), (L2, V2)


# ---- d. products with the widest operands ------------------------------------------------------------------------------------------------------
def _pairs(C, t1, t2, rng, n_rand=6):
    (L1, V1), (L2, V2) = t1, t2
    va = F.edge_values(C, V1) + [rng.randrange(V1 * C.P) for _ in range(n_rand)]
    vb = F.edge_values(C, V2) + [rng.randrange(V2 * C.P) for _ in range(n_rand)]
    out = [(x, y) for x in va[:3] for y in vb[:3]] + list(zip(va[3:], vb[3:]))
    return [(x, y, F.operand(C, x, L1, V1), F.operand(C, y, L2, V2)) for x, y in out]


def _check_prod(C, o, expect, what):
    assert limbs_ok(o, C.P), ("bound", what)
    assert F.value(o) % C.P == expect % C.P, ("value", what)


@pytest.mark.parametrize("tag", CURVES)
def test_mul_sqr_dot_widest_operands(H, tag):
    h, C = H[tag], H[tag].C
    P, RI = C.P, C.RINV
    rng = random.Random(11)
    for mid, (t1, t2) in enumerate(F.MUL):
        cs = _pairs(C, t1, t2, rng)
        a, b = arr([c[2] for c in cs], 14), arr([c[3] for c in cs], 14)
        out = np.zeros_like(a)
        h.call("fe_mul", mid, a, b, out, len(cs))
        for (x, y, _, _), o in zip(cs, out):
            _check_prod(C, o, x * y * RI, ("mul", t1, t2, hex(x), hex(y)))
    for qid, t in enumerate(F.SQR):
        vals = F.edge_values(C, t[1]) + [rng.randrange(t[1] * P) for _ in range(6)]
        a = arr([F.operand(C, v, *t) for v in vals], 14)
        out = np.zeros_like(a)
        h.call("fe_sqr", qid, a, out, len(vals))
        for v, o in zip(vals, out):
            _check_prod(C, o, v * v * RI, ("sqr", t, hex(v)))
    for nt, tab in ((2, F.DOT2), (4, F.DOT4)):
        for did, (t1, t2) in enumerate(tab):
            cases = []
            for e in range(3):                      # every term at the same edge, then mixed edges, then random
                cases.append([(F.edge_values(C, t1[1])[e], F.edge_values(C, t2[1])[e]) for _ in range(nt)])
            cases.append([(F.edge_values(C, t1[1])[j % 3], F.edge_values(C, t2[1])[(j + 1) % 3]) for j in range(nt)])
            cases += [[(rng.randrange(t1[1] * P), rng.randrange(t2[1] * P)) for _ in range(nt)] for _ in range(4)]
            a = arr([sum((F.operand(C, x, *t1) for x, _ in cs), []) for cs in cases], nt * 14)
            b = arr([sum((F.operand(C, y, *t2) for _, y in cs), []) for cs in cases], nt * 14)
            out = np.zeros((len(cases), 14), dtype=np.uint32)
            h.call("fe_dot", nt, did, a, b, out, len(cases))
            for cs, o in zip(cases, out):
                _check_prod(C, o, sum(x * y for x, y in cs) * RI, ("dot", nt, t1, t2))
    for msid, ts in enumerate(F.MULSUB):
        cases = [[F.edge_values(C, t[1])[e] for t in ts] for e in range(3)]
        cases += [[F.edge_values(C, t[1])[(e + j) % 3] for j, t in enumerate(ts)] for e in range(3)]
        cases += [[rng.randrange(t[1] * P) for t in ts] for _ in range(4)]
        a = arr([sum((F.operand(C, v, *t) for v, t in zip(cs, ts)), []) for cs in cases], 56)
        out = np.zeros((len(cases), 14), dtype=np.uint32)
        h.call("fe_mul_sub", msid, a, out, len(cases))
        for cs, o in zip(cases, out):
            _check_prod(C, o, (cs[0] * cs[1] - cs[2] * cs[3]) * RI, ("mul_sub", ts, [hex(v) for v in cs]))


def _f2_vals(C, t, rng):
    e = F.edge_values(C, t[1])
    return [(x, y) for x in e for y in e] + [(rng.randrange(t[1] * C.P), rng.randrange(t[1] * C.P)) for _ in range(4)]


def _f2op(C, v, t): return F.operand(C, v[0], *t) + F.operand(C, v[1], *t)


@pytest.mark.parametrize("tag", CURVES)
def test_fp2_products_widest_operands(H, tag):
    h, C = H[tag], H[tag].C
    P = C.P
    rng = random.Random(13)
    beta = 1 if tag == "381" else 5
    for fid, (t1, t2) in enumerate(F.F2MUL[tag]):
        va, vb = _f2_vals(C, t1, rng), _f2_vals(C, t2, rng)
        cases = [(x, y) for x in va[:9:4] for y in vb[:9]] + list(zip(va[9:], vb[9:]))
        a, b = arr([_f2op(C, x, t1) for x, _ in cases], 28), arr([_f2op(C, y, t2) for _, y in cases], 28)
        out = np.zeros_like(a)
        h.call("fe_f2mul", fid, a, b, out, len(cases))
        for (x, y), o in zip(cases, out):
            e = F.f2_expect_mul(C, x, y)
            _check_prod(C, o[:14], e[0], ("f2_muld c0", t1, t2)); _check_prod(C, o[14:], e[1], ("f2_muld c1", t1, t2))
    for fid, t in enumerate(F.F2SQR[tag]):
        va = _f2_vals(C, t, rng)
        a = arr([_f2op(C, x, t) for x in va], 28)
        out = np.zeros((len(va), 42), dtype=np.uint32)
        h.call("fe_f2sqr", fid, a, out, len(va))
        for x, row, o in zip(va, a, out):
            e = F.f2_expect_mul(C, x, x)
            _check_prod(C, o[:14], e[0], ("f2_sqrd c0", t)); _check_prod(C, o[14:28], e[1], ("f2_sqrd c1", t))
            # fq_mul_beta: beta a, limb-wise (lazy): every limb exactly beta times the operand's
            assert [int(v) for v in o[28:42]] == [beta * int(v) for v in row[:14]], ("fq_mul_beta", t)
    for fid, ts in enumerate(F.F2MULSUB[tag]):
        cases = [[_f2_vals(C, t, rng)[(e * 4 + j) % 9] for j, t in enumerate(ts)] for e in range(9)]
        cases += [[(rng.randrange(t[1] * P), rng.randrange(t[1] * P)) for t in ts] for _ in range(4)]
        a = arr([sum((_f2op(C, v, t) for v, t in zip(cs, ts)), []) for cs in cases], 112)
        out = np.zeros((len(cases), 28), dtype=np.uint32)
        h.call("fe_f2mulsub", fid, a, out, len(cases))
        for cs, o in zip(cases, out):
            ab, cd = F.f2_expect_mul(C, cs[0], cs[1]), F.f2_expect_mul(C, cs[2], cs[3])
            _check_prod(C, o[:14], ab[0] - cd[0], ("f2_muld_sub c0", ts)); _check_prod(C, o[14:], ab[1] - cd[1], ("f2_muld_sub c1", ts))
    for fid, (t1, t2) in enumerate(F.F2MULFQ):
        va = _f2_vals(C, t1, rng)
        vs = F.edge_values(C, t2[1]) + [rng.randrange(t2[1] * P)]
        cases = [(x, s) for x in va for s in vs]
        a, b = arr([_f2op(C, x, t1) for x, _ in cases], 28), arr([F.operand(C, s, *t2) for _, s in cases], 14)
        out = np.zeros_like(a)
        h.call("fe_f2mulfq", fid, a, b, out, len(cases))
        for (x, s), o in zip(cases, out):
            _check_prod(C, o[:14], x[0] * s * C.RINV, ("f2_mul_fq", t1, t2)); _check_prod(C, o[14:], x[1] * s * C.RINV, ("f2_mul_fq", t1, t2))


# ---- e. storage conversions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CURVES)
def test_storage_round_trips(H, tag):
    h, C = H[tag], H[tag].C
    P = C.P
    vals = F.storage_values(C, random.Random(17))
    a = arr([F.words12(v) for v in vals], 12)
    out = np.zeros((len(vals), 122), dtype=np.uint32)
    h.call("fe_storage", a, out, len(vals))
    for v, o in zip(vals, out):
        o = [int(x) for x in o]
        assert o[0:14] == F.to_limbs(v), ("fq_unpack", hex(v))
        assert F.from_words(o[14:26]) == v, ("fq_pack", hex(v))
        assert o[26:40] == F.to_limbs(v << 8) and all(x <= F.MASK for x in o[26:40]), ("fq_unpack_shl8", hex(v))
        # engine values are Mont-384: x * 2^-384 -> Mont-392 integers x * 2^8
        assert limbs_ok(o[40:54], P) and F.value(o[40:54]) % P == (v << 8) % P, ("fq_from_fp", hex(v))
        assert limbs_ok(o[54:68], P) and F.value(o[54:68]) % P == (v << 8) % P, ("fq_from_fp_fast", hex(v))
        assert F.from_words(o[68:80]) == v, ("fq_to_fp(fq_from_fp)", hex(v))
        assert o[80:94] == F.to_limbs(v << 8) and F.value(o[80:94]) < 256 * P, ("fq_tab", hex(v))
        assert o[94:108] == o[80:94] and o[108:122] == o[80:94], ("f2_tab", hex(v))
    # fq_to_fp on reduced values at their edges: [0, 2p) with normalised limbs
    reds = [0, 1, P - 1, P, P + 1, 2 * P - 1] + [v for v in vals if v < P][:16]
    a = arr([F.to_limbs(v) for v in reds], 14)
    out = np.zeros((len(reds), 12), dtype=np.uint32)
    h.call("fe_to_fp", a, out, len(reds))
    for v, o in zip(reds, out):
        assert F.from_words(o) == (v * pow(2, -8, P)) % P, ("fq_to_fp", hex(v))


# ---- f. group law on lifted coordinates ----------------------------------------------------------------------------------------------------------
def _slots(tag, g2):
    if not g2:
        return (36, 19, 8)
    return (11, 7, 8) if tag == "381" else (4, 4, 4)


def _jac(F_, pt, z):
    """affine (x, y) -> Jacobian (x z^2, y z^3, z) over field bundle F_"""
    z2 = F_.mul(z, z)
    return F_.mul(pt[0], z2), F_.mul(pt[1], F_.mul(z2, z)), z


def _group_cases(C, g2):
    m = C.m
    Fb = m._Fp2 if g2 else m._Fp
    mul = m.g2_mul if g2 else m.g1_mul
    P1, Q1 = mul(1234567), mul(7654321)
    rng = random.Random(19)
    if g2:
        zs = [(1, 0), (C.P - 1, 0), (2, 0), (0, 1), (rng.randrange(C.P), rng.randrange(C.P))]
    else:
        zs = [1, C.P - 1, 2, (C.P + 1) // 2, rng.randrange(C.P)]
    neg = m.ec_neg(Fb, P1)
    return Fb, P1, [(z, q, name) for z in zs for q, name in ((P1, "P"), (neg, "-P"), (Q1, "Q"))]


def _fld(C, v, g2, VB, LM=F.L28):
    """a field value (Fp or Fp2 integers, canonical) in Montgomery-392 form + (VB - 1) p, largest-limb form"""
    if g2:
        return sum((F.operand(C, C.mont(c) + (VB - 1) * C.P, LM, VB) for c in v), [])
    return F.operand(C, C.mont(v) + (VB - 1) * C.P, LM, VB)


def _unfld(C, limbs, g2):
    if g2:
        return (C.unmont(F.value(limbs[:14])), C.unmont(F.value(limbs[14:28])))
    return C.unmont(F.value(limbs))


def _affine(Fb, X, Y, Z):
    zi = Fb.inv(Z); zi2 = Fb.mul(zi, zi)
    return Fb.mul(X, zi2), Fb.mul(Y, Fb.mul(zi2, zi))


@pytest.mark.parametrize("tag", CURVES)
@pytest.mark.parametrize("g2", [False, True], ids=["G1", "G2"])
def test_group_law_lifted_coordinates(H, tag, g2):
    h, C = H[tag], H[tag].C
    m, P = C.m, C.P
    Fb, P1, cases = _group_cases(C, g2)
    sx, sy, sz = _slots(tag, g2)
    w = 28 if g2 else 14
    modes = [1, 2] if (not g2 or tag == "381") else [1]
    fn = "fe_g2" if g2 else "fe_g1"
    for mode in [0] + modes:
        rows, expect = [], []
        for z, q, name in cases:
            if mode == 0 and name != "P":
                continue
            X, Y, Z = _jac(Fb, P1, z)
            row = _fld(C, X, g2, sx) + _fld(C, Y, g2, sy) + _fld(C, Z, g2, sz)
            if mode == 0:
                row += [0] * (2 * w); expect.append((m.ec_add(Fb, P1, P1), False))
            elif mode == 1:
                row += _fld(C, q[0], g2, 1) + _fld(C, q[1], g2, 1); expect.append((m.ec_add(Fb, P1, q), name != "Q"))
            else:                                     # table operands: x2 < 256p, y2 < 258p with limbs < 2^29
                row += _fld(C, q[0], g2, 256) + _fld(C, q[1], g2, 258, 1 << 29); expect.append((m.ec_add(Fb, P1, q), name != "Q"))
            rows.append(row)
        a = arr(rows, 5 * w)
        out, flag = np.zeros((len(rows), 3 * w), dtype=np.uint32), np.zeros(len(rows), dtype=np.uint32)
        h.call(fn, mode, a, out, flag, len(rows))
        for (want, special), o, f in zip(expect, out, flag):
            assert bool(f) == special, ("special flag", tag, g2, mode)
            if special:
                continue
            for part, VB in ((o[0:w], sx), (o[w:2 * w], sy), (o[2 * w:3 * w], sz)):
                assert all(int(x) <= F.MASK for x in part), ("limbs", tag, g2, mode)
                for c in range(0, w, 14):
                    assert F.value(part[c:c + 14]) < VB * P, ("slot bound", tag, g2, mode, VB)
            got = _affine(Fb, _unfld(C, o[0:w], g2), _unfld(C, o[w:2 * w], g2), _unfld(C, o[2 * w:3 * w], g2))
            assert got == want, ("group law", tag, g2, mode)


# ---- g. stage 2a of the pairing product on chosen lines ---------------------------------------------------------------------------------------------
def run_line_products(h, kara, lines, M, T, rows):
    stride = M + 3
    buf = np.zeros((rows, 18, stride, 4), dtype=np.uint32)
    for r in range(rows):
        for i in range(M):
            for f in range(6):
                w = F.words12(lines[r][i][f])
                for c in range(3):
                    buf[r, 3 * f + c, i, :] = w[4 * c:4 * c + 4]
    part = np.zeros((rows, 36, T, 4), dtype=np.uint32)
    h.call("fe_line_products", kara, buf, stride, M, T, rows, part)
    return part


@pytest.mark.parametrize("tag,kara", [("381", 1), ("381", 0), ("377", 0)], ids=["381-k", "381-q", "377-q"])
def test_line_products_extreme_lines(H, tag, kara):
    h, C = H[tag], H[tag].C
    for si, (M, T, rows) in enumerate(F.LP_SHAPES):
        lines = F.lp_lines(C, M, rows, seed=100 + si)
        part = run_line_products(h, kara, lines, M, T, rows)
        for r in range(rows):
            for tt in range(T):
                want = F.expected_accumulator(C, [lines[r][i] for i in range(tt, M, T)])
                for j in range(6):
                    for p_ in range(2):
                        got = F.from_words(part[r, j * 6 + p_ * 3:j * 6 + p_ * 3 + 3, tt, :].reshape(12))
                        assert got == want[j][p_], ("line products", tag, kara, (M, T, rows), r, tt, j, p_)
    # one accumulator per row over a line pair whose final values reach [p, 1.01 p) in k_line_products_k (tests/field_edges.py LP_HIGH_SEEDS)
    lines = [F.lp_high_lines(C, s) for s in F.LP_HIGH_SEEDS]
    part = run_line_products(h, kara, lines, 2, 1, len(lines))
    for r, ls in enumerate(lines):
        want = F.expected_accumulator(C, ls)
        for j in range(6):
            for p_ in range(2):
                got = F.from_words(part[r, j * 6 + p_ * 3:j * 6 + p_ * 3 + 3, 0, :].reshape(12))
                assert got == want[j][p_], ("line products, final value >= p", tag, kara, F.LP_HIGH_SEEDS[r], j, p_)
    # one accumulator per row over two or three lines with every coefficient at an extreme (tests/field_edges.py lp_extreme_sequences): the largest
    # int64 columns of k_line_products_k (2^61.70 by lk_model, test_field_edges_cpu.py)
    seqs = F.lp_extreme_sequences(C)
    for M in (2, 3):
        names = [k for k, ls in seqs.items() if len(ls) == M]
        part = run_line_products(h, kara, [seqs[k] for k in names], M, 1, len(names))
        for r, name in enumerate(names):
            want = F.expected_accumulator(C, seqs[name])
            for j in range(6):
                for p_ in range(2):
                    got = F.from_words(part[r, j * 6 + p_ * 3:j * 6 + p_ * 3 + 3, 0, :].reshape(12))
                    assert got == want[j][p_], ("line products, extreme sequence", tag, kara, name, j, p_)
