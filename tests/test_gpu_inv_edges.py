"""GPU (-m gpu): the device field inversion (fp_inv_bingcd, fp_inv_kaliski, finv), the Fp2 inverse, to_affine and the batch normalisation k_normalize<F>
AT THEIR EDGES, through the device harness tests/device/inv_edges.hip (built from the production headers by build():
tests/device/build/libinv_edges_{381,377}.so), and the public ripp_normalize_g1 / ripp_normalize_g2 around the sizes at which a lane gets a second and a
third point.

The inversion inputs are the list of tests/inv_edges.py (tests/test_inv_model_cpu.py runs the model of tools/inv_model.py over it and shows that only its
structured values reach the last of the 26 outer iterations).  The reference is Python integers only, every comparison is exact, and every output word
must be canonical (< p)."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import inv_edges as E
import inv_model as IM

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = E.TAGS
U32P = ctypes.POINTER(ctypes.c_uint32)
RBITS = 384
BINGCD, KALISKI, FINV = 0, 1, 2
FORMS = [BINGCD, KALISKI, FINV]


def pack(vals):
    """integers < 2^384 -> (n, 12) words"""
    return np.frombuffer(b"".join(v.to_bytes(48, "little") for v in vals), dtype=np.uint32).reshape(len(vals), 12).copy()


def unpack(a):
    """(..., 12 k) words -> a flat list of integers, 12 words each"""
    raw = np.ascontiguousarray(a, dtype=np.uint32).tobytes()
    return [int.from_bytes(raw[o:o + 48], "little") for o in range(0, len(raw), 48)]


class Harness:
    def __init__(self, tag):
        path = os.path.join(HERE, "device", "build", "libinv_edges_%s.so" % tag)
        assert os.path.exists(path), "device harness missing: %s (build() builds it: make -C tests/device)" % path
        self.lib = ctypes.CDLL(path)
        self.tag, self.C = tag, IM.CURVES[tag]
        self.P = self.C.P
        self.beta = 5 if tag == "377" else 1                       # Fp2 = Fp[u] / (u^2 + beta)
        assert self.lib.ie_curve() == int(tag)

    def _call(self, name, *args):
        rc = getattr(self.lib, name)(*[a.ctypes.data_as(U32P) if isinstance(a, np.ndarray) else a for a in args])
        assert rc == 0, "%s returned %d" % (name, rc)

    def fp_inv(self, which, vals, block):
        a = pack(vals); out = np.zeros_like(a)
        self._call("ie_fp_inv", which, a, len(vals), block, out)
        return unpack(out)

    def fp2_inv(self, pairs):
        a = pack([c for pr in pairs for c in pr]); out = np.zeros_like(a)
        self._call("ie_fp2_inv", a, len(pairs), out)
        r = unpack(out)
        return list(zip(r[0::2], r[1::2]))

    def _points(self, name, g2, pts, *extra):
        """pts: n x 3 coordinates of NF integers each -> n x 2 coordinates"""
        nf = 2 if g2 else 1
        a = pack([w for pt in pts for c in pt for w in c]); out = np.zeros((len(pts) * 2 * nf, 12), dtype=np.uint32)
        self._call(name, g2, a, len(pts), *extra, out)
        r = unpack(out)
        return [(tuple(r[2 * nf * i:2 * nf * i + nf]), tuple(r[2 * nf * i + nf:2 * nf * (i + 1)])) for i in range(len(pts))]

    def normalize(self, g2, pts, T): return self._points("ie_normalize", g2, pts, T)
    def to_affine(self, g2, pts): return self._points("ie_to_affine", g2, pts)

    # ---- the reference: Python integers.  Values travel in Montgomery form (x 2^384)
    def mont(self, x): return x * (1 << RBITS) % self.P
    def plain(self, w): return w * pow(1 << RBITS, -1, self.P) % self.P

    def f2_mul(self, a, b):
        return ((a[0] * b[0] - self.beta * a[1] * b[1]) % self.P, (a[0] * b[1] + a[1] * b[0]) % self.P)

    def f2_inv(self, a):
        n = pow((a[0] * a[0] + self.beta * a[1] * a[1]) % self.P, -1, self.P)
        return (a[0] * n % self.P, -a[1] * n % self.P)

    def norm(self, a): return (a[0] * a[0] + self.beta * a[1] * a[1]) % self.P


@pytest.fixture(scope="module")
def H(engine):
    return {t: Harness(t) for t in CURVES}


@functools.lru_cache(maxsize=None)
def expected_list(tag):
    return tuple(E.expected(tag, y) for y in E.values(tag))


def check_inv(h, which, vals, block, what):
    got = h.fp_inv(which, vals, block)
    assert len(got) == len(vals)
    for i, (y, g) in enumerate(zip(vals, got)):
        assert g < h.P, (what, "not canonical", which, block, i, hex(y), hex(g))
        assert g == E.expected(h.tag, y), (what, which, block, "lane", i, hex(y), hex(g))


# ---- a. the inversion, all three forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("which", FORMS)
@pytest.mark.parametrize("tag", CURVES)
def test_inversion_over_the_whole_list(H, tag, which, block):
    """y^-1 2^768 mod p for every value of the list (0 for 0), one lane each, in list order: neighbours 2^k - 1, 2^k, 2^k + 1 share a wave"""
    h = H[tag]
    vals = E.values(tag)
    assert len(vals) % 64 != 0
    got = h.fp_inv(which, vals, block)
    want = expected_list(tag)
    for i, (y, g, w) in enumerate(zip(vals, got, want)):
        assert g < h.P and g == w, (which, block, "lane", i, hex(y), hex(g), hex(w))


@functools.lru_cache(maxsize=None)
def mixed_layout(tag):
    """the list's extremes laid out so that every wave mixes lanes that leave the loops at different times: zero lanes (never live), the shortest Kaliski
    runs (k = BITS), the longest (k up to 2 BITS - 1), the inputs that need all 26 outer iterations of the binary GCD, and random values; then waves with
    one live lane among zeros, one zero among full runs, and a wave of zeros between two ordinary ones"""
    C = IM.CURVES[tag]
    vals, ks = E.values(tag), E.kaliski_steps(tag)
    order = sorted((i for i in range(len(vals)) if vals[i]), key=lambda i: ks[i])
    short = [vals[i] for i in order if ks[i] == C.BITS]
    longest = [vals[i] for i in order[-16:]]
    assert short and ks[order[-1]] == 2 * C.BITS - 1
    full, rnd = list(E.full_run(tag)), list(E.randoms(tag))
    pools = [[0], short, longest, full, rnd]
    out = []
    for w in range(8):
        for j in range(64):
            pool = pools[(j + w) % 5]
            out.append(pool[(j // 5 + 3 * w) % len(pool)])
    out += [0] * 63 + [longest[-1]]                                   # one live lane keeps its wave in the Kaliski loop to the end
    out += [full[0]] + [0] * 63
    out += (full * 11)[:31] + [0] + (full * 11)[31:63]
    out += [0] * 64
    out += [short[j % len(short)] if j % 2 else longest[j % len(longest)] for j in range(64)]
    out += full[:5] + [0, 1, longest[-1]]                             # a ragged last wave
    assert len(out) % 64 == 8
    return tuple(out)


@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("which", FORMS)
@pytest.mark.parametrize("tag", CURVES)
def test_inversion_in_mixed_waves(H, tag, which, block):
    check_inv(H[tag], which, mixed_layout(tag), block, "mixed")


@pytest.mark.parametrize("which", FORMS)
@pytest.mark.parametrize("tag", CURVES)
def test_inversion_of_zero_waves_and_ragged_launches(H, tag, which):
    """a launch whose waves are all zero (no lane is ever live), and launches whose size is no multiple of the wave: 1, 63, 65, 130, 257 lanes"""
    h = H[tag]
    for block in (64, 256):
        check_inv(h, which, [0] * 192, block, "zero waves")
        check_inv(h, which, [0] * 70, block, "zero waves, ragged")
    src = list(E.full_run(tag)) + list(E.structured(tag)[:40]) + list(E.randoms(tag)[:300])
    for n, block in ((1, 64), (63, 64), (65, 64), (130, 256), (257, 256)):
        check_inv(h, which, src[:n], block, "n = %d" % n)
        check_inv(h, which, src[-n:], block, "n = %d" % n)


# ---- b. the Fp2 inverse ----------------------------------------------------------------------------------------------------------------------------------
def sqrt_mod(a, p):
    """a square root of a mod p, or None (Tonelli-Shanks)"""
    a %= p
    if a == 0: return 0
    if pow(a, (p - 1) // 2, p) != 1: return None
    q, s = p - 1, 0
    while q % 2 == 0: q //= 2; s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1: z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1: t2 = t2 * t2 % p; i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    assert r * r % p == a
    return r


def with_norm(h, c, count):
    """`count` elements (a0, a1) of Fp2 with a0^2 + beta a1^2 = c"""
    out, a1 = [], 0
    while len(out) < count:
        a1 += 1
        a0 = sqrt_mod(c - h.beta * a1 * a1, h.P)
        if a0 is not None:
            out += [(a0, a1), (h.P - a0, h.P - a1)]
    return out[:count]


@pytest.mark.parametrize("tag", CURVES)
def test_fp2_inverse_with_zero_parts_and_unit_norms(H, tag):
    """finv(Fp2) = conj(a) / norm(a), norm = a0^2 + a1^2 (BLS12-381) / a0^2 + 5 a1^2 (BLS12-377): a zero part, both parts at p - 1, elements whose norm is
    1 or p - 1 -- as a value and as the word the inversion receives (value 2^-384) --, parts whose WORDS come from the edge list, random elements, 0 -> 0"""
    h = H[tag]
    p = h.P
    rnd = random.Random(77 + int(tag))
    rinv = pow(1 << RBITS, -1, p)
    plain = [(1, 0), (0, 1), (p - 1, p - 1), (p - 1, 0), (0, p - 1), (2, 0), (0, 2), (1, 1), (1, p - 1)]
    for c in (1, p - 1, rinv, p - rinv):                              # the norm whose Montgomery word is 1 / p - 1: value +-2^-384
        els = with_norm(h, c, 6)
        assert all(h.norm(a) == c for a in els)
        plain += els
    for _ in range(8):                                                # z / conj(z) has norm 1
        z = (rnd.randrange(p), rnd.randrange(1, p))
        w = h.f2_mul(z, h.f2_inv((z[0], -z[1] % p)))
        assert h.norm(w) == 1
        plain.append(w)
    plain += [(rnd.randrange(p), rnd.randrange(p)) for _ in range(200)]
    words = [(h.mont(a0), h.mont(a1)) for a0, a1 in plain]
    lst = E.structured(tag)
    picks = [lst[i] for i in range(0, len(lst), 13)] + list(E.full_run(tag))
    words += [(y, 0) for y in picks] + [(0, y) for y in picks] + [(y, picks[(i * 7 + 1) % len(picks)]) for i, y in enumerate(picks)]
    words += [(0, 0)] * 3
    got = h.fp2_inv(words)
    assert len(got) == len(words)
    for i, (a, g) in enumerate(zip(words, got)):
        assert g[0] < p and g[1] < p, ("not canonical", i)
        if a == (0, 0):
            assert g == (0, 0), i
            continue
        e = h.f2_inv((h.plain(a[0]), h.plain(a[1])))
        assert g == (h.mont(e[0]), h.mont(e[1])), ("element", i, hex(a[0]), hex(a[1]))


# ---- c. k_normalize<F> and to_affine ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 1), (5, 5), (37, 5), (64, 64), (65, 64), (257, 256), (300, 7), (1024, 64)]
Z_PATTERNS = ["one", "minus_one", "list"]
INF_PATTERNS = {
    "none": lambda i, n, T: False,
    "all": lambda i, n, T: True,
    "first of every chain": lambda i, n, T: i < T,
    "last of every chain": lambda i, n, T: i + T >= n,
    "every other point": lambda i, n, T: (i + i // T) % 2 == 1,           # alternating along every chain and across the lanes
    "whole chains": lambda i, n, T: (i % T) % 3 == (1 if T > 1 else 0),    # lanes that invert 1 beside ordinary lanes
}
NMAX = max(n for n, _ in SHAPES)


@functools.lru_cache(maxsize=None)
def point_pool(tag, g2, zpat):
    """NMAX points (words of X, Y, Z) with their expected affine words, computed once: coordinates are arbitrary field elements (the kernel does field
    arithmetic only), never X = Y = 0; Z = 1, Z = p - 1 (both parts on G2), or Z words from the edge list (on G2 one part is zero at every fifth point)"""
    h = Harness(tag)
    p = h.P
    rnd = random.Random(1000 * int(tag) + 10 * g2 + Z_PATTERNS.index(zpat))
    nf = 2 if g2 else 1
    zs = [y for y in E.structured(tag) if y]
    pts, want = [], []
    for i in range(NMAX):
        X = tuple(rnd.randrange(1, p) for _ in range(nf)); Y = tuple(rnd.randrange(1, p) for _ in range(nf))
        if i % 9 == 4: X = (0,) * nf                                   # a zero coordinate of a finite point
        if i % 9 == 7: Y = (0,) * nf
        if zpat == "one": Z = (h.mont(1),) + (0,) * (nf - 1)
        elif zpat == "minus_one": Z = (h.mont(p - 1),) * nf
        else:
            Z = tuple(zs[(11 * (nf * i + c)) % len(zs)] for c in range(nf))
            if g2 and i % 5 == 1: Z = (Z[0], 0)
            if g2 and i % 5 == 3: Z = (0, Z[1])
        x, y, z = ([h.plain(w) for w in c] for c in (X, Y, Z))
        if g2:
            zi = h.f2_inv(tuple(z)); zi2 = h.f2_mul(zi, zi)
            ax, ay = h.f2_mul(tuple(x), zi2), h.f2_mul(tuple(y), h.f2_mul(zi2, zi))
        else:
            zi = pow(z[0], -1, p)
            ax, ay = (x[0] * zi * zi % p,), (y[0] * zi * zi * zi % p,)
        pts.append((X, Y, Z)); want.append((tuple(h.mont(v) for v in ax), tuple(h.mont(v) for v in ay)))
    return pts, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_T%d" % s)
@pytest.mark.parametrize("g2", [0, 1], ids=["g1", "g2"])
@pytest.mark.parametrize("tag", CURVES)
def test_normalize_chains_with_infinities(H, tag, g2, shape):
    """k_normalize<Fp> / k_normalize<Fp2> with T lanes over n points (lane t: t, t + T, ...; T = n: one point per lane, the lane inverts Z itself; the
    last lanes of (37, 5), (65, 64), (257, 256), (300, 7) are one point shorter): (X / Z^2, Y / Z^3), and (0, 0) for Z = 0, with the points at infinity
    at the start, at the end, alternating, everywhere, and filling whole chains; to_affine on the same points"""
    h = H[tag]
    n, T = shape
    nf = 2 if g2 else 1
    zero = ((0,) * nf, (0,) * nf)
    for zpat in Z_PATTERNS:
        pool, pool_want = point_pool(tag, g2, zpat)
        for name, inf in INF_PATTERNS.items():
            pts, want = [], []
            for i in range(n):
                X, Y, Z = pool[i]
                if inf(i, n, T): pts.append((X, Y, (0,) * nf)); want.append(zero)
                else: pts.append((X, Y, Z)); want.append(pool_want[i])
            got = h.normalize(g2, pts, T)
            assert len(got) == n
            for i in range(n):
                assert all(w < h.P for c in got[i] for w in c), ("not canonical", zpat, name, i)
                assert got[i] == want[i], ("k_normalize", zpat, name, "point", i, "lane", i % T, "position", i // T)
            if name in ("none", "every other point"):
                assert h.to_affine(g2, pts) == want, ("to_affine", zpat, name)


def test_normalize_refuses_bad_lane_counts(H):
    a = np.zeros((4, 36), dtype=np.uint32); out = np.zeros((4, 24), dtype=np.uint32)
    for T in (0, 5):
        assert H["381"].lib.ie_normalize(0, a.ctypes.data_as(U32P), 4, T, out.ctypes.data_as(U32P)) == -1


# ---- d. the public path around K = 1 -> 2 -> 3 ------------------------------------------------------------------------------------------------------------
PUBLIC_N = [131071, 131072, 131073, 196608]


@pytest.fixture(scope="module")
def blinded(engine, orc):
    """max(PUBLIC_N) oracle-blinded Jacobian points of each group (every test takes a prefix)"""
    n = max(PUBLIC_N)
    return orc.blind_g1(engine.synth_g1(4242, n), 11), orc.blind_g2(engine.synth_g2(2424, n), 12)


@pytest.mark.parametrize("n", PUBLIC_N)
def test_public_normalize_at_the_lane_batch_switches(engine, orc, blinded, n):
    """ripp_normalize_g1 / ripp_normalize_g2 (BLS12-381) where engine.hip::normalize_dev changes the points per lane K = min(16, max(1, n / 65536)),
    T = ceil(n / K): 131 071 (K = 1), 131 072 (K = 2), 131 073 (K = 2, the last lane one point short), 196 608 (K = 3); infinity at 0, T - 1, T, n - 1
    and on every point of one lane; against the oracle's normalisation"""
    K = min(16, max(1, n // 65536)); T = (n + K - 1) // K
    assert (K, T) == {131071: (1, 131071), 131072: (2, 65536), 131073: (2, 65537), 196608: (3, 65536)}[n]
    at = sorted({0, T - 1, T % n, n - 1} | {i for i in range(12345, n, T)})
    assert len([i for i in at if i % T == 12345]) == K
    for src, norm_gpu, norm_cpu in ((blinded[0], engine.normalize_batch_g1, orc.normalize_g1), (blinded[1], engine.normalize_batch_g2, orc.normalize_g2)):
        pj = src[:n].copy()
        pj[at] = 0
        got, want = norm_gpu(pj), norm_cpu(pj)
        assert not want[at].any() and want[1].any()
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, ("points that differ", bad[:8], "lanes", bad[:8] % T)
