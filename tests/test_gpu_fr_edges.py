"""GPU (-m gpu): the 32-bit Montgomery form Mont<P> (Fr and Fp: the inline-asm column-accumulator mul / mul2_add, add, sub, neg, to / from Montgomery form), the
Barrett division msm_divmod, the five digit passes that copy it, the KZG quotient scan with its production launch sequence, k_pc_partial_eval, k_fr_dot /
k_fr_dot2 and k_fold_fr / k_fold_fr2, AT THEIR EDGES, through the device harness tests/device/fr_edges.hip (built from the production headers by build():
tests/device/build/libfr_edges_{381,377}.so).

The cases and the model are those of tests/fr_edges.py (tests/test_fr_edges_model_cpu.py shows that the lists reach both reduction branches and both Barrett
outcomes and that the scan model is suffix Horner).  The reference is Python integers only and every comparison is exact."""
import ctypes
import os
import random

import numpy as np
import pytest

import fr_edges as E

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = E.TAGS
OPS = {"mul": 0, "sqr": 1, "add": 2, "sub": 3, "neg": 4, "from_mont": 5, "to_mont": 6, "mul2_add": 7, "mul_cios": 8}
SENTINEL = int.from_bytes(b"\xA5" * 32, "little")
PLAN_FIELDS = ["c", "nwin", "nb", "n", "ch", "seg", "nreal", "gmin"]
MSM_DIGITS, BATCH, TPC_CROSS, GIPA_MEXP, TIPA_CROSS_G2 = range(5)
GUARD = 4096


def pack(vals, nlimb=8):
    """integers -> (n, nlimb) words"""
    nb = 4 * nlimb
    return np.frombuffer(b"".join(v.to_bytes(nb, "little") for v in vals), dtype=np.uint32).reshape(len(vals), nlimb).copy()


def unpack(a, nlimb=8):
    nb = 4 * nlimb
    raw = np.ascontiguousarray(a, dtype=np.uint32).tobytes()
    return [int.from_bytes(raw[o:o + nb], "little") for o in range(0, len(raw), nb)]


class Harness:
    def __init__(self, tag):
        path = os.path.join(HERE, "device", "build", "libfr_edges_%s.so" % tag)
        assert os.path.exists(path), "device harness missing: %s (build() builds it: make -C tests/device)" % path
        self.lib = ctypes.CDLL(path)
        self.tag, self.C = tag, E.CURVES[tag]
        self.r = self.C.r
        assert self.lib.fe_curve() == int(tag)

    def _call(self, name, *args):
        conv = [a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else a for a in args]
        rc = getattr(self.lib, name)(*conv)
        assert rc == 0, "%s returned %d" % (name, rc)

    def mont(self, fname, op, cases):
        """cases: tuples of 1, 2 or 4 raw operands -> the raw results"""
        F = self.C.field(fname)
        cols = [pack([c[min(j, len(c) - 1)] for c in cases], F.N) for j in range(4)]
        out = np.zeros_like(cols[0])
        self._call("fe_mont", 0 if fname == "fr" else 1, OPS[op], *cols, ctypes.c_uint32(len(cases)), out)
        return unpack(out, F.N)

    def divmod(self, by_x, ks):
        n = len(ks)
        q, rem = np.zeros((n, 24 if by_x else 8), dtype=np.uint32), np.zeros((n, 9 if by_x else 5), dtype=np.uint32)
        self._call("fe_divmod", int(by_x), pack(ks), ctypes.c_uint32(n), q, rem)
        if not by_x: return unpack(q), unpack(rem, 5)
        return [unpack(row) for row in q], [unpack(row, 3) for row in rem]

    def plan(self, nreal, split, rows=0, c=0):
        out = np.zeros(8, dtype=np.uint32)
        self._call("fe_plan", ctypes.c_size_t(nreal), split, ctypes.c_size_t(rows), c, ctypes.c_uint32(0), ctypes.c_uint32(0), out)
        return dict(zip(PLAN_FIELDS, (int(v) for v in out)))

    def digits(self, which, scalars, arg, stride, rows, plan):
        """scalars: canonical integers (sent in Montgomery form).  Returns (digits, guard, histogram or None)"""
        nd = rows * plan["nwin"] * plan["n"]
        dg = np.zeros(nd + GUARD, dtype=np.uint16)
        hist = np.zeros(plan["nwin"] * plan["nb"], dtype=np.uint32)
        pw = np.array([plan[f] for f in PLAN_FIELDS], dtype=np.uint32)
        self._call("fe_digits", which, pack([self.C.fr.mont(k) for k in scalars]), ctypes.c_size_t(len(scalars)), ctypes.c_uint32(arg), ctypes.c_size_t(stride),
                   ctypes.c_uint32(rows), pw, ctypes.c_size_t(GUARD), dg, hist)
        return dg[:nd], dg[nd:], (hist if which == MSM_DIGITS else None)

    def kzg_scan(self, p, z, per):
        """plain p, z -> plain (h, cin, q, eval) and the raw slots the kernels must leave alone"""
        F, m = self.C.fr, len(p)
        nchunk = (m + 63) // 64
        h, cin, q = np.zeros((nchunk + 1, 8), dtype=np.uint32), np.zeros((nchunk + 1, 8), dtype=np.uint32), np.zeros((m + 2, 8), dtype=np.uint32)
        self._call("fe_kzg_scan", pack([F.mont(v) for v in p]), ctypes.c_size_t(m), pack([F.mont(z)]), ctypes.c_size_t(per), h, cin, q)
        h, cin, q = unpack(h), unpack(cin), unpack(q)
        untouched = [h[nchunk], cin[nchunk], q[m - 1], q[m + 1]]
        return [F.plain(v) for v in h[:nchunk]], [F.plain(v) for v in cin[:nchunk]], [F.plain(v) for v in q[:m - 1]], F.plain(q[m]), untouched

    def partial_eval(self, coef, rows, cols, stride, xp, ncols, out_len):
        F = self.C.fr
        out = np.zeros((out_len, 8), dtype=np.uint32)
        self._call("fe_partial_eval", pack([F.mont(v) for v in coef]), ctypes.c_uint32(rows), ctypes.c_uint32(cols), ctypes.c_size_t(stride), pack([F.mont(v) for v in xp]),
                   ctypes.c_uint32(ncols), ctypes.c_size_t(out_len), out)
        return unpack(out)

    def fr_dot(self, two, l, r, n, grid):
        F = self.C.fr
        out = np.zeros((grid * (2 if two else 1) + 1, 8), dtype=np.uint32)
        self._call("fe_fr_dot", int(two), pack([F.mont(v) for v in l]), pack([F.mont(v) for v in r]), ctypes.c_uint32(n), ctypes.c_uint32(grid), out)
        return unpack(out)

    def fold_fr(self, hi, lo, s, out_len):
        F = self.C.fr
        out = np.zeros((out_len, 8), dtype=np.uint32)
        self._call("fe_fold_fr", pack([F.mont(v) for v in hi]), pack([F.mont(v) for v in lo]), ctypes.c_uint32(len(hi)), pack([F.mont(s)]), ctypes.c_size_t(out_len), out)
        return unpack(out)

    def fold_fr2(self, m, b, h, c, c_inv, out_len):
        F = self.C.fr
        mo, bo = np.zeros((out_len, 8), dtype=np.uint32), np.zeros((out_len, 8), dtype=np.uint32)
        self._call("fe_fold_fr2", pack([F.mont(v) for v in m]), pack([F.mont(v) for v in b]), ctypes.c_uint32(h), pack([F.mont(c)]), pack([F.mont(c_inv)]), ctypes.c_size_t(out_len), mo, bo)
        return unpack(mo), unpack(bo)


@pytest.fixture(scope="module")
def H(engine):
    return {t: Harness(t) for t in CURVES}


def first_diff(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w: return i, g, w
    return None


# ---- a. Mont<P> ------------------------------------------------------------------------------------------------------------------------------------------
def mont_cases(tag, fname, op):
    if op in ("mul", "mul_cios"): return E.mul_cases(tag, fname)
    if op == "add": return E.add_cases(tag, fname)
    if op == "sub": return E.sub_cases(tag, fname)
    if op == "mul2_add": return E.mul2_cases(tag)
    return tuple((v,) for v in E.operands(tag, fname))


@pytest.mark.parametrize("op", ["mul", "sqr", "add", "sub", "neg", "from_mont", "to_mont", "mul_cios", "mul2_add"])
@pytest.mark.parametrize("fname", ["fr", "fp"])
@pytest.mark.parametrize("tag", CURVES)
def test_mont_ops(H, tag, fname, op):
    h = H[tag]
    if op == "mul2_add" and fname == "fr":
        a = pack([1])
        assert h.lib.fe_mont(0, OPS[op], *[a.ctypes.data_as(ctypes.c_void_p)] * 4, ctypes.c_uint32(1), a.ctypes.data_as(ctypes.c_void_p)) == -1      # the form of Fp only
        return
    cases = mont_cases(tag, fname, op)
    got = h.mont(fname, op, cases)
    assert len(got) == len(cases)
    m = h.C.field(fname).m
    for i, (c, g) in enumerate(zip(cases, got)):
        assert g < m, (op, "not canonical", i, [hex(v) for v in c], hex(g))
        assert g == E.expect(tag, fname, op, c), (op, "case", i, [hex(v) for v in c], hex(g))


@pytest.mark.parametrize("fname", ["fr", "fp"])
@pytest.mark.parametrize("tag", CURVES)
def test_device_mul_is_device_mul_cios(H, tag, fname):
    cases = E.mul_cases(tag, fname)
    assert H[tag].mont(fname, "mul", cases) == H[tag].mont(fname, "mul_cios", cases)


# ---- b. msm_divmod -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CURVES)
def test_divmod_lambda(H, tag):
    ks, lam = E.divmod_cases(tag), E.CURVES[tag].lam
    q, rem = H[tag].divmod(False, ks)
    for k, qq, rr in zip(ks, q, rem):
        assert (qq, rr) == divmod(k, lam), (hex(k), hex(qq), hex(rr))


@pytest.mark.parametrize("tag", CURVES)
def test_divmod_x_chain(H, tag):
    ks, x = E.divmod_cases(tag), E.CURVES[tag].x
    q, rem = H[tag].divmod(True, ks)
    for k, qs, rs in zip(ks, q, rem):
        assert list(zip(qs, rs)) == E.x_chain(tag, k), (hex(k), [hex(v) for v in qs], [hex(v) for v in rs])
        digits = rs + [qs[2]]
        assert sum(d * x**j for j, d in enumerate(digits)) == k and all(d < 1 << 64 for d in digits)


# ---- c. digit passes -------------------------------------------------------------------------------------------------------------------------------------------
def check_digit_buffer(h, got, guard, plan, split, rows, placement, what):
    want = E.expected_digits(h.tag, plan, split, rows, placement)
    got = [int(v) for v in got]
    assert 0xFFFF not in got, (what, "a digit was never written", got.index(0xFFFF) if 0xFFFF in got else None)
    assert len(got) == len(want) and got == want, (what, plan, first_diff(got, want))
    assert guard.size == GUARD and bool((guard == 0xFFFF).all()), (what, "the guard region was written")


@pytest.mark.parametrize("nreal", [1, 255, 256, 257])
@pytest.mark.parametrize("split", [1, 2, 4])
@pytest.mark.parametrize("tag", CURVES)
def test_msm_digits(H, tag, split, nreal):
    h = H[tag]
    ks = E.digit_scalars(tag, nreal, split)
    placement = {(0, i): k for i, k in enumerate(ks)}
    seen = set()
    for c in [0] + list(range(4, 14)):
        plan = h.plan(nreal, split, c=c)
        E.check_plan(plan, split, nreal)
        assert c == 0 or plan["c"] == c
        seen.add(plan["c"])
        for k in ks[:16]: E.check_digit_model(tag, k, split, plan)
        got, guard, hist = h.digits(MSM_DIGITS, ks, 0, 0, 1, plan)
        check_digit_buffer(h, got, guard, plan, split, 1, placement, ("k_msm_digits", split, nreal, c))
        comps = [E.components(tag, k, split) for k in ks]                      # the scalars read back from the device's digits
        for i in range(nreal):
            for j in range(split):
                assert sum(int(got[w * plan["n"] + j * nreal + i]) << (w * plan["c"]) for w in range(plan["nwin"])) == comps[i][j]
        assert [int(v) for v in hist] == E.histogram(plan, [int(v) for v in got]), ("histogram", split, nreal, c)
    assert seen == set(range(4, 14))


def batch_plan(h, nreal, split, rows, c):
    plan = h.plan(nreal, split, rows=rows, c=c)
    E.check_plan(plan, split, nreal)
    return plan


@pytest.mark.parametrize("c", [0, 4, 13])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("tag", CURVES)
def test_msm_digits_batch(H, tag, rows, c):
    h, r = H[tag], H[tag].r
    for nreal, cols, gap in [(1, 0, 2), (2, 1, 1), (256, 255, 3), (257, 256, 3), (300, 5, 7), (258, 257, 1)]:
        stride = cols + gap
        plan = batch_plan(h, nreal, 2, rows, c)
        ks = E.digit_scalars(tag, rows * cols, 10 + rows)
        flat, placement = [], {}
        for row in range(rows):
            for i in range(stride):
                flat.append(ks[row * cols + i] if i < cols else r - 1)         # the stride gap holds r - 1: read, it would show as non-zero digits
                if i < cols: placement[(row, i)] = ks[row * cols + i]
        got, guard, _ = h.digits(BATCH, flat, cols, stride, rows, plan)
        check_digit_buffer(h, got, guard, plan, 2, rows, placement, ("k_msm_digits_batch", rows, nreal, cols, stride, c))


@pytest.mark.parametrize("c", [0, 4, 13])
@pytest.mark.parametrize("hh", [1, 2, 128, 129])
@pytest.mark.parametrize("which", [TPC_CROSS, TIPA_CROSS_G2])
@pytest.mark.parametrize("tag", CURVES)
def test_cross_digit_passes(H, tag, which, hh, c):
    """row 0 carries m[h + i] at base i < h, row 1 carries m[i] at base h + i; the other half of each row is zero digits (DESIGN.md sections 4c, 4e)"""
    h = H[tag]
    split = 2 if which == TPC_CROSS else 4
    plan = batch_plan(h, 2 * hh, split, 2, c)
    m = E.digit_scalars(tag, 2 * hh, 20 + hh)
    placement = {}
    for i in range(hh):
        placement[(0, i)] = m[hh + i]
        placement[(1, hh + i)] = m[i]
    got, guard, _ = h.digits(which, m, hh, 0, 2, plan)
    check_digit_buffer(h, got, guard, plan, split, 2, placement, ("cross", which, hh, c))


@pytest.mark.parametrize("c", [0, 4, 13])
@pytest.mark.parametrize("ln", [2, 4, 256, 258])
@pytest.mark.parametrize("tag", CURVES)
def test_gipa_mexp_digits(H, tag, ln, c):
    """X = ck_b | m_a (2 len bases).  row 0: m_b[i] at h + i, row 1: m_b[i] at len + h + i, row 2: m_b[h + i] at i, row 3: m_b[h + i] at len + i"""
    h = H[tag]
    hh = ln // 2
    plan = batch_plan(h, 2 * ln, 2, 4, c)
    mb = E.digit_scalars(tag, ln, 30 + ln)
    placement = {}
    for i in range(hh):
        placement[(0, hh + i)] = mb[i]
        placement[(1, ln + hh + i)] = mb[i]
        placement[(2, i)] = mb[hh + i]
        placement[(3, ln + i)] = mb[hh + i]
    got, guard, _ = h.digits(GIPA_MEXP, mb, ln, 0, 4, plan)
    check_digit_buffer(h, got, guard, plan, 2, 4, placement, ("k_gipa_mexp_digits", ln, c))


# ---- d. the KZG scan ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.scan_cases(), ids=lambda c: "m%d_per%d" % (c[0], c[1]))
@pytest.mark.parametrize("tag", CURVES)
def test_kzg_scan(H, tag, case):
    m, per, points = case
    h, r = H[tag], H[tag].r
    for zn in points:
        z = E.scan_point(tag, zn)
        for kind in E.SCAN_POLYS:
            p = E.scan_poly(tag, m, kind, z)
            wh, wcin, wq, wev = E.scan_model(p, z, r, per)
            gh, gcin, gq, gev, untouched = h.kzg_scan(p, z, per)
            what = (tag, m, per, zn, kind)
            assert gh == wh, (what, "h", first_diff(gh, wh))
            assert gcin == wcin, (what, "cin", first_diff(gcin, wcin))
            assert gq == wq, (what, "q", first_diff(gq, wq))
            assert gev == wev, (what, "eval", hex(gev), hex(wev))
            assert untouched == [SENTINEL] * 4, (what, "a slot behind h, cin, the quotient or eval was written", [hex(v) for v in untouched])


def test_kzg_scan_refuses_a_short_lane_share(H):
    p = pack([1] * 64 * 257)
    out = np.zeros((64 * 257 + 2, 8), dtype=np.uint32)
    args = [a.ctypes.data_as(ctypes.c_void_p) for a in (p, pack([2]))]
    assert H["381"].lib.fe_kzg_scan(args[0], ctypes.c_size_t(64 * 257), args[1], ctypes.c_size_t(1), *[out.ctypes.data_as(ctypes.c_void_p)] * 3) == -1


# ---- e. k_pc_partial_eval ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2, 3, 64])
@pytest.mark.parametrize("tag", CURVES)
def test_partial_eval(H, tag, rows):
    h, r = H[tag], H[tag].r
    rnd = random.Random("partial_eval %s %d" % (tag, rows))
    for cols, ncols in [(1, 1), (255, 256), (256, 257), (257, 513), (5, 300)]:
        for stride in (cols, cols + 3):
            edge = [0, r - 1, 1]
            coef = [(edge[(i + j) % 3] if (i * cols + j) % 5 == 0 else rnd.randrange(r)) if j < cols else r - 1 for i in range(rows) for j in range(stride)]
            xp = [edge[i % 3] if i % 4 == 1 else rnd.randrange(r) for i in range(rows)]
            out_len = ncols + 9
            got = h.partial_eval(coef, rows, cols, stride, xp, ncols, out_len)
            want = [h.C.fr.mont(sum(xp[i] * coef[i * stride + j] for i in range(rows)) % r) if j < cols else 0 for j in range(ncols)] + [SENTINEL] * 9
            assert got == want, (rows, cols, ncols, stride, first_diff(got, want))


# ---- f. k_fr_dot / k_fr_dot2 ---------------------------------------------------------------------------------------------------------------------------------------
def dot_operands(tag, count, seed):
    r = E.CURVES[tag].r
    rnd = random.Random("dot %s %d %d" % (tag, count, seed))
    edge = [r - 1, 0, 1, r - 2]
    return [edge[(i // 3) % 4] if i % 3 == 0 else rnd.randrange(r) for i in range(count)]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 513, 1025])
@pytest.mark.parametrize("tag", CURVES)
def test_fr_dot(H, tag, n):
    h, r, F = H[tag], H[tag].r, H[tag].C.fr
    l, rr = dot_operands(tag, n, 0), dot_operands(tag, n, 1)[::-1]
    rr[0] = r - 1; l[0] = r - 1                                               # (r - 1)^2 among the products
    want = sum(a * b for a, b in zip(l, rr)) % r
    for grid in sorted({1, 2, 3, (n + 255) // 256}):
        got = h.fr_dot(False, l, rr, n, grid)
        assert got[grid] == SENTINEL and all(v < r for v in got[:grid]), (n, grid)
        assert sum(F.plain(v) for v in got[:grid]) % r == want, (n, grid)
        for b in range(grid):                                                # each block's partial is the sum of the indices its lanes stride over
            idx = [i for i in range(n) if (i // 256) % grid == b]
            assert F.plain(got[b]) == sum(l[i] * rr[i] for i in idx) % r, (n, grid, b)


@pytest.mark.parametrize("hh", [1, 255, 256, 257, 511, 513, 1025])
@pytest.mark.parametrize("tag", CURVES)
def test_fr_dot2(H, tag, hh):
    """partials[0 : grid] sum to <m[h:], b[:h]>, partials[grid : 2 grid] to <m[:h], b[h:]>"""
    h, r, F = H[tag], H[tag].r, H[tag].C.fr
    m, b = dot_operands(tag, 2 * hh, 2), dot_operands(tag, 2 * hh, 3)[::-1]
    m[hh] = r - 1; b[0] = r - 1; m[0] = 2; b[2 * hh - 1] = 3                   # (r - 1)^2 in the first product only: the halves cannot be mistaken for each other
    want0 = sum(x * y for x, y in zip(m[hh:], b[:hh])) % r
    want1 = sum(x * y for x, y in zip(m[:hh], b[hh:])) % r
    assert want0 != want1
    for grid in sorted({1, 2, 3, (hh + 255) // 256}):
        got = h.fr_dot(True, m, b, hh, grid)
        assert got[2 * grid] == SENTINEL and all(v < r for v in got[:2 * grid]), (hh, grid)
        assert sum(F.plain(v) for v in got[:grid]) % r == want0, (hh, grid, "<m[h:], b[:h]>")
        assert sum(F.plain(v) for v in got[grid:2 * grid]) % r == want1, (hh, grid, "<m[:h], b[h:]>")


# ---- g. k_fold_fr / k_fold_fr2 ---------------------------------------------------------------------------------------------------------------------------------------
def fold_scalars(tag):
    r = E.CURVES[tag].r
    return [0, 1, r - 1, random.Random("fold " + tag).randrange(2, r - 1)]


@pytest.mark.parametrize("half", [1, 255, 256, 257])
@pytest.mark.parametrize("tag", CURVES)
def test_fold_fr(H, tag, half):
    h, r, F = H[tag], H[tag].r, H[tag].C.fr
    hi, lo = dot_operands(tag, half, 4), dot_operands(tag, half, 5)[::-1]
    hi[0] = lo[0] = r - 1
    for s in fold_scalars(tag):
        got = h.fold_fr(hi, lo, s, half + 5)
        want = [F.mont((a * s + b) % r) for a, b in zip(hi, lo)] + [SENTINEL] * 5
        assert got == want, (half, hex(s), first_diff(got, want))


@pytest.mark.parametrize("half", [1, 255, 256, 257])
@pytest.mark.parametrize("tag", CURVES)
def test_fold_fr2(H, tag, half):
    """m_out = c m[h:] + m[:h] and b_out = c_inv b[h:] + b[:h]: c and c_inv are INDEPENDENT values here, so a swap shows"""
    h, r, F = H[tag], H[tag].r, H[tag].C.fr
    m, b = dot_operands(tag, 2 * half, 6), dot_operands(tag, 2 * half, 7)[::-1]
    m[half] = b[half] = m[0] = b[0] = r - 1
    sc = fold_scalars(tag)
    for c in sc:
        for c_inv in sc:
            mo, bo = h.fold_fr2(m, b, half, c, c_inv, half + 5)
            wm = [F.mont((m[half + i] * c + m[i]) % r) for i in range(half)] + [SENTINEL] * 5
            wb = [F.mont((b[half + i] * c_inv + b[i]) % r) for i in range(half)] + [SENTINEL] * 5
            assert mo == wm, (half, hex(c), hex(c_inv), "m_out", first_diff(mo, wm))
            assert bo == wb, (half, hex(c), hex(c_inv), "b_out", first_diff(bo, wb))
