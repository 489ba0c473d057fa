"""GPU (-m gpu): stage 1 of the pairing product -- k_vm_miller_lines (vm.hpp), k_miller_lines_q (fq_miller.hpp), k_miller_lines (kernels.hpp) -- line by
line against the textbook formulas, and the scalar dense tree k_fp12_tree, through the device harness tests/device/miller_edges.hip (built from the
production headers by build(): tests/device/build/libmiller_edges_{381,377}.so); then the small launch sizes of every stage-1 / stage-2 / tree form
through the engine itself against the oracle.

The reference, the comparison rule (a stored triple equals k x the reference triple for one k in Fp, no tolerance) and the point sets are in
tests/miller_edges.py, checked on the CPU by tests/test_miller_edges_cpu.py.  Every launch is checked whole: all stored words below p, the unit line bit
for bit where a pair has a point at infinity, the harness's sentinel untouched at every lane position >= M."""
import ctypes
import os

import numpy as np
import pytest

import miller_edges as E

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = ["381", "377"]
KINDS = {0: "k_vm_miller_lines", 1: "k_miller_lines_q", 2: "k_miller_lines"}
U32P = ctypes.POINTER(ctypes.c_uint32)
BIG = 2 ** 32 - 1


def _words(v): return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


class Harness:
    def __init__(self, tag):
        path = os.path.join(HERE, "device", "build", "libmiller_edges_%s.so" % tag)
        assert os.path.exists(path), "device harness missing: %s (build() builds it: make -C tests/device)" % path
        self.lib = ctypes.CDLL(path)
        self.tag, self.C = tag, E.CURVES[tag]
        assert self.lib.me_curve() == int(tag) and self.lib.me_n_lines() == self.C.n_lines == {"381": 68, "377": 69}[tag] and self.lib.me_max_share() == 4
        self.lib.me_sentinel.restype = ctypes.c_uint32
        self.sentinel = self.lib.me_sentinel()
        self.lib.me_lines.argtypes = [ctypes.c_int, U32P, ctypes.c_uint32, U32P, ctypes.c_uint32, U32P, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int, U32P]
        self.lib.me_fp12_tree.argtypes = [U32P, ctypes.c_uint32, U32P, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32]
        self.unit = np.array(E.unit_words(tag), dtype=np.uint32).reshape(18, 4)
        self.pw = np.array(_words(self.C.P), dtype=np.uint32)

    def pack(self, pts, g2):
        """model points (None = infinity = all zero) -> the engine's Montgomery-384 words"""
        nf = 4 if g2 else 2
        out = np.zeros((len(pts), nf * 12), dtype=np.uint32)
        for i, pt in enumerate(pts):
            if pt is None: continue
            cs = (pt[0][0], pt[0][1], pt[1][0], pt[1][1]) if g2 else pt
            out[i] = [w for c in cs for w in _words(c * E.R384 % self.C.P)]
        return out

    def lines(self, kind, g1, g2, sets, M, stride=None, no_share=0):
        """-> the whole line buffer as (nprod, N_LINES, 18 chunks, stride, 4 words)"""
        stride = ((M + 63) & ~63) if stride is None else stride
        a, b = self.pack(g1, False), self.pack(g2, True)
        s = np.array(sets, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros((len(s), self.C.n_lines, 18, stride, 4), dtype=np.uint32)
        rc = self.lib.me_lines(kind, a.ctypes.data_as(U32P), len(a), b.ctypes.data_as(U32P), len(b), s.ctypes.data_as(U32P), len(s), M, stride, no_share, out.ctypes.data_as(U32P))
        if rc > 0: pytest.exit("me_lines (%s): HIP error %d -- nothing more is started on this device" % (KINDS[kind], rc), returncode=3)
        assert rc == 0, "me_lines refused its arguments (%s)" % KINDS[kind]
        return out

    def check_whole(self, buf, M, what):
        """the sentinel at every lane position >= M; every stored 12-word vector < p"""
        assert (buf[:, :, :, M:, :] == self.sentinel).all(), (what, "sentinel overwritten at a lane >= M")
        w = buf[:, :, :, :M, :].transpose(0, 1, 3, 2, 4).reshape(-1, 12)
        lt, eq = np.zeros(len(w), dtype=bool), np.ones(len(w), dtype=bool)
        for k in range(11, -1, -1):
            lt |= eq & (w[:, k] < self.pw[k]); eq &= w[:, k] == self.pw[k]
        assert lt.all(), (what, "a stored value >= p", int((~lt).sum()))

    def ints(self, buf, p, lanes):
        """{lane: [six raw integers per step]} of product p"""
        nl = self.C.n_lines
        out = {}
        for i in lanes:
            raw = np.ascontiguousarray(buf[p, :, :, i, :]).tobytes()
            out[i] = [tuple(int.from_bytes(raw[(s * 6 + k) * 48:(s * 6 + k + 1) * 48], "little") for k in range(6)) for s in range(nl)]
        return out

    def check_pairs(self, buf, p, lanes, g1, g2, po, qo, what):
        """product p (P vector at g1[po:], Q vector at g2[qo:]) at the given lanes: unit bit for bit where a point is at infinity, else k x the reference"""
        C = self.C
        got = self.ints(buf, p, lanes)
        for i in lanes:
            ref = E.ref_lines(self.tag, g1[po + i], g2[qo + i])
            if ref is None:
                assert (buf[p, :, :, i, :] == self.unit).all(), (what, "product", p, "lane", i, "not the unit line")
                continue
            for s in range(C.n_lines):
                assert E.scale_equal(C.P, tuple(E.decode(C, v) for v in got[i][s]), ref[s]), (what, "product", p, "lane", i, "step", s)

    def check_same_lines(self, buf, other, nprod, M, what):
        """every lane of every product of two launches over the same pairs: equal up to one factor of Fp per line"""
        P = self.C.P
        for p in range(nprod):
            a, b = self.ints(buf, p, range(M)), self.ints(other, p, range(M))
            for i in range(M):
                for s in range(self.C.n_lines):
                    x, y = a[i][s], b[i][s]
                    if x == y: continue
                    assert any(y) and E.scale_equal(P, x, y), (what, "product", p, "lane", i, "step", s)

    def tree(self, vals, Tin, R, rows):
        """vals[row][j]: 12 integers -> k_fp12_tree's output as [row][j] tuples of 12 integers (and the raw buffer)"""
        Tout = (Tin + R - 1) // R
        a = np.zeros((rows, 36, Tin, 4), dtype=np.uint32)
        for r in range(rows):
            for j in range(Tin):
                a[r, :, j, :] = np.array([w for c in vals[r][j] for w in _words(c)], dtype=np.uint32).reshape(36, 4)
        out = np.zeros((rows, 36, Tout, 4), dtype=np.uint32)
        rc = self.lib.me_fp12_tree(a.ctypes.data_as(U32P), Tin, out.ctypes.data_as(U32P), Tout, R, rows)
        if rc > 0: pytest.exit("me_fp12_tree: HIP error %d -- nothing more is started on this device" % rc, returncode=3)
        assert rc == 0, "me_fp12_tree refused its arguments"
        res = []
        for r in range(rows):
            row = []
            for j in range(Tout):
                raw = np.ascontiguousarray(out[r, :, j, :]).tobytes()
                row.append(tuple(int.from_bytes(raw[48 * k:48 * k + 48], "little") for k in range(12)))
            res.append(row)
        return res


@pytest.fixture(scope="module")
def H(engine):
    return {t: Harness(t) for t in CURVES}


def _lanes(M): return range(M) if M <= 65 else sorted({0, 63, 64, 255, 256, M - 1} & set(range(M)))


# ---- one product ---------------------------------------------------------------------------------------------------------------------------------------
SHAPES = {0: [1, 3, 4, 5, 15, 16, 17], 1: [1, 63, 64, 65, 255, 256, 257], 2: [1, 63, 64, 65, 255, 256, 257]}       # 4 pairs per wave and 16 per block on the VM; 64 and 256 lanes


@pytest.fixture(scope="module")
def plain_big(H):
    """k_miller_lines at M = 255, 256, 257 on set (a), checked against the reference at the boundary lanes: what the other two kernels are held against there"""
    out = {}
    for tag in CURVES:
        ps, qs = E.subgroup_points(tag, 257)
        for M in (255, 256, 257):
            buf = H[tag].lines(2, ps, qs, [(0, 0)], M)
            H[tag].check_whole(buf, M, ("plain", tag, M))
            H[tag].check_pairs(buf, 0, _lanes(M), ps, qs, 0, 0, ("plain", tag, M))
            out[tag, M] = buf
    return out


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("tag", CURVES)
def test_single_product_every_lane(H, plain_big, tag, kind):
    h = H[tag]
    ps, qs = E.subgroup_points(tag, 257)
    for M in SHAPES[kind]:
        strides = [None] + ([((M + 63) & ~63) + 64] if M in (17, 65) else [])
        for stride in strides:
            what = (KINDS[kind], tag, M, stride)
            buf = plain_big[tag, M] if (kind == 2 and M >= 255 and stride is None) else h.lines(kind, ps, qs, [(0, 0)], M, stride)
            h.check_whole(buf, M, what)
            h.check_pairs(buf, 0, _lanes(M), ps, qs, 0, 0, what)
            if kind == 1 and M >= 255: h.check_same_lines(buf, plain_big[tag, M], 1, M, what)
    if kind == 0:                                                  # the VM kernel over many blocks: every lane against k_miller_lines
        for M in (255, 256, 257):
            buf = h.lines(0, ps, qs, [(0, 0)], M)
            h.check_whole(buf, M, (KINDS[0], tag, M))
            h.check_pairs(buf, 0, _lanes(M), ps, qs, 0, 0, (KINDS[0], tag, M))
            h.check_same_lines(buf, plain_big[tag, M], 1, M, (KINDS[0], tag, M))


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("tag", CURVES)
def test_lines_give_the_model_pairing(H, tag, kind):
    """the independent anchor: the kernel's lines of four subgroup pairs through miller_combine's recurrence and the model's final exponentiation"""
    h, C = H[tag], E.CURVES[tag]
    ps, qs = E.subgroup_points(tag, 257)
    buf = h.lines(kind, ps, qs, [(0, 0)], 4)
    got = h.ints(buf, 0, range(4))
    for i in range(4):
        lines = [tuple(E.decode(C, v) for v in t) for t in got[i]]
        assert C.m.final_exponentiation(E.combine(C, lines)) == E.model_pairing(tag, ps[i], qs[i]), (KINDS[kind], tag, i)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("tag", CURVES)
def test_edge_coordinates(H, tag, kind):
    """every edge P with every edge Q of set (b): coordinates 0, 1, 2, p - 1, p - 2 through the conversions and the lazy bounds of both steps"""
    h = H[tag]
    eg1, (eg2, _) = E.edge_g1(tag), E.edge_g2(tag)
    g1 = [Pt for Pt in eg1 for _ in eg2]
    g2 = [Q for _ in eg1 for Q in eg2]
    M = len(g1)
    buf = h.lines(kind, g1, g2, [(0, 0)], M)
    h.check_whole(buf, M, (KINDS[kind], tag, "edge"))
    h.check_pairs(buf, 0, range(M), g1, g2, 0, 0, (KINDS[kind], tag, "edge"))


# ---- several products: chains, skip flags, row offsets ------------------------------------------------------------------------------------------------
SIX = [(0, 0), (16, 0), (32, 0), (48, 0), (64, 8), (80, 8)]           # four P vectors on one Q vector, then two on a second one
FIVE = [(0, 0), (16, 0), (32, 0), (48, 0), (64, 0)]                   # a chain of 4 and a chain of 1
THREE = [(0, 0), (16, 0), (32, 8)]


def _pools(tag, M):
    ps, qs = E.subgroup_points(tag, 257 + 80)
    return list(ps[:M + 80]), list(qs[:M + 8])


def _check_products(h, kind, g1, g2, sets, M, what, no_share=0):
    buf = h.lines(kind, g1, g2, sets, M, no_share=no_share)
    h.check_whole(buf, M, what)
    for p, (po, qo) in enumerate(sets): h.check_pairs(buf, p, _lanes(M), g1, g2, po, qo, what)
    return buf


def _infinity_matrix(h, kind, g1, g2, sets, M, base, patterns, what):
    """At lanes 0, 63, 64 and M - 1 in turn, each pattern of infinities (launch r puts pattern (j + r) mod n at the j-th of these lanes, so n launches show
    every pattern at every lane): ("P", t) only product t's P, ("Q",) only the Q of product 0's vector, ("both",) product 0's P and that Q.  A product's
    rows at a lane are the unit line exactly where ITS P or ITS Q is at infinity, and everything else is what the launch without infinities stored."""
    lanes = [i for i in (0, 63, 64, M - 1) if i < M]
    for r in range(len(patterns)):
        a, b = list(g1), list(g2)
        for j, i in enumerate(lanes):
            pat = patterns[(j + r) % len(patterns)]
            if pat[0] == "P": a[sets[pat[1]][0] + i] = None
            if pat[0] in ("Q", "both"): b[sets[0][1] + i] = None
            if pat[0] == "both": a[sets[0][0] + i] = None
        want = base.copy()
        units = 0
        for p, (po, qo) in enumerate(sets):
            for i in range(M):
                if a[po + i] is None or b[qo + i] is None: want[p, :, :, i, :] = h.unit; units += 1
        assert units >= len(lanes)
        got = h.lines(kind, a, b, sets, M)
        bad = np.argwhere((got != want).any(axis=(2, 4)))
        assert len(bad) == 0, (what, "launch", r, "first differing (product, step, lane)", bad[0].tolist(), "of", len(bad))


@pytest.mark.parametrize("M", [65, 257])
@pytest.mark.parametrize("tag", CURVES)
def test_shared_chains(H, tag, M):
    h = H[tag]
    g1, g2 = _pools(tag, M)
    base = _check_products(h, 1, g1, g2, SIX, M, ("chains", tag, M))
    if M > 65:                                                    # every lane of every product against k_miller_lines on the same six products
        plain = _check_products(h, 2, g1, g2, SIX, M, ("chains, plain kernel", tag, M))
        h.check_same_lines(base, plain, len(SIX), M, ("chains vs plain", tag, M))
    alone = _check_products(h, 1, g1, g2, SIX, M, ("chains, sharing off", tag, M), no_share=1)
    assert np.array_equal(alone, base), "a product's lines depend on the chain it shares"        # canonical words of the same field elements
    _check_products(h, 1, g1, g2, FIVE, M, ("chain of 4 + chain of 1", tag, M))
    _infinity_matrix(h, 1, g1, g2, SIX, M, base, [("P", 0), ("P", 1), ("P", 2), ("P", 3), ("Q",), ("both",)], ("chains, infinities", tag, M))


@pytest.mark.parametrize("M", [65, 257])
@pytest.mark.parametrize("kind", [0, 2])
@pytest.mark.parametrize("tag", CURVES)
def test_three_products_rows_and_infinities(H, tag, kind, M):
    """grid.y = product: the row offset blockIdx.y * N_LINES and each product's own skip flag"""
    h = H[tag]
    g1, g2 = _pools(tag, M)
    base = _check_products(h, kind, g1, g2, THREE, M, (KINDS[kind], "three products", tag, M))
    _infinity_matrix(h, kind, g1, g2, THREE, M, base, [("P", 0), ("P", 1), ("P", 2), ("Q",), ("both",)], (KINDS[kind], "three products, infinities", tag, M))


# ---- k_fp12_tree -----------------------------------------------------------------------------------------------------------------------------------------
TREE_TINS = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257]


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("tag", CURVES)
def test_fp12_tree(H, tag, R):
    """out[j] = prod_{k < R, j + k Tout < Tin} in[j + k Tout], bit for bit: Montgomery-384 operands, so every product carries one factor 2^-384 and the
    result is canonical.  Value classes of tests/vm_edges.py (zero, one in a single coefficient, p - 1 everywhere, random)."""
    import vm_edges as VE
    import vm_model as VM
    from vm_model import vmgen
    h, C = H[tag], E.CURVES[tag]
    name = VM.TAGS[tag]
    vmgen.set_curve(name)
    try:
        def mont_mul(f, g):
            r = vmgen.f12m([(f[2 * i], f[2 * i + 1]) for i in range(6)], [(g[2 * i], g[2 * i + 1]) for i in range(6)])
            return tuple(c * C.rinv % C.P for pair in r for c in pair)
        for rows in (1, 3):
            for Tin in TREE_TINS:
                vals = [VE.tree_input(VM.CURVES[name], Tin, row) for row in range(rows)]
                Tout = (Tin + R - 1) // R
                got = h.tree(vals, Tin, R, rows)
                for row in range(rows):
                    for j in range(Tout):
                        acc = tuple(vals[row][j])
                        for k in range(1, R):
                            if j + k * Tout < Tin: acc = mont_mul(acc, vals[row][j + k * Tout])
                        assert got[row][j] == acc, (tag, "R", R, "Tin", Tin, "row", row, "j", j)
    finally:
        vmgen.set_curve("bls12_381")


# ---- the engine's small launches, every form -------------------------------------------------------------------------------------------------------------
STAGE1 = {"vm": {}, "carry-free": dict(vm_lines_max=0), "plain": dict(vm_lines_max=0, ml_fq_min=BIG)}
STAGE2 = {"default": {}, "no karatsuba": dict(no_lp_karatsuba=1), "plain": dict(lp_fq_min=BIG)}
TREES = {"default": {}, "no vm tree": dict(vm_tree_max=0)}


_ORACLE = {}          # the oracle's values, once per curve and size


def _engine(engine, tag):
    if tag == "381":
        import orclib as o
        o.lib()
        return engine, o
    import orclib377 as o
    import ripp_amd.bls12_377 as R377
    R377.init(0); o.lib()
    return R377, o


def _accumulators(tag, stage2):
    """T of Engine::enqueue_stage2 for one product: max(per_wave, (SIMDs * RIPP_OCC_PROD / N_LINES) * per_wave), per_wave = 10 accumulators for the
    Karatsuba line products (BLS12-381, default form) and 21 otherwise; SIMDs = 4 per compute unit, as Engine::init counts them (the harness's me_n_simd)"""
    n_simd = Harness(tag).lib.me_n_simd()
    assert n_simd > 0
    per_wave = 10 if (tag == "381" and stage2 == "default") else 21
    return max(per_wave, (n_simd * 2 // E.CURVES[tag].n_lines) * per_wave)


@pytest.mark.parametrize("stage1", list(STAGE1))
@pytest.mark.parametrize("tag", CURVES)
def test_engine_small_sizes_every_form(engine, tag, stage1):
    """PairingInnerProduct at the sizes around one block, one wave of accumulators and the accumulator count T, and two-product SIPP launches, under every
    stage-1 x stage-2 x tree form: byte-identical to the oracle (computed once per size)"""
    R, o = _engine(engine, tag)
    want, sipp = _ORACLE.setdefault((tag, "ip"), {}), _ORACLE.setdefault((tag, "sipp"), {})

    def inputs(n):
        a, b = o.gen_g1(31, n), o.gen_g2(37, n)
        if n > 2: a[0] = 0; b[n - 1] = 0
        return o.blind_g1(a, 1), o.blind_g2(b, 2)
    try:
        for s2, c2 in STAGE2.items():
            T = _accumulators(tag, s2)
            sizes = [1, 2, 9, 10, 11, 20, 21, 22, T - 1, T, T + 1, 3 * T + 1]
            for tr, c3 in TREES.items():
                R.configure(**STAGE1[stage1], **c2, **c3)
                for n in sizes:
                    aj, bj = inputs(n)
                    if n not in want:
                        rc, want[n] = o.pairing_product_j(aj, bj)
                        assert rc == 0
                    assert np.array_equal(R.PairingInnerProduct.inner_product(aj, bj), want[n]), (tag, stage1, s2, tr, n)
                for n in (2, 64):
                    a, b, r = o.gen_g1(41, n), o.gen_g2(43, n), o.gen_scalars(47, n)
                    if n not in sipp:
                        v = o.product_of_pairings_with_coeffs(a, b, r)
                        rc, proof, _ = o.sipp_prove(a, b, r, v)
                        assert rc == 0
                        sipp[n] = (v, proof)
                    v, proof = sipp[n]
                    assert np.array_equal(R.product_of_pairings_with_coeffs(a, b, r), v), (tag, stage1, s2, tr, n)
                    assert np.array_equal(R.SIPP.prove(a, b, r, v), proof), (tag, stage1, s2, tr, "sipp", n)
    finally:
        R.configure()
