"""Inputs shared by tests/test_validate_inputs_cpu.py and tests/test_gpu_validate.py: untrusted G1 / G2 points of both curves, by class, each with the
flag the DEFINITION gives it -- limb range, curve equation, then `ec_mul(F, R, P) is None` -- never an endomorphism.  Built from
tests/model/bls381_model.py / bls377_model.py alone, with a fixed seed.

A point is a tuple of 2 (G1) or 4 (G2: x.c0, x.c1, y.c0, y.c1) integers: the MONTGOMERY limb values as they lie in a ripp_g1a / ripp_g2a, which may
be >= p for the `unreduced` class.  Flags: 0 valid, 1 a coordinate >= p, 2 not on the curve, 3 on the curve but outside the prime-order subgroup."""
import ctypes
import functools
import random

import numpy as np

SEED = 0x56414C
TAGS = ("381", "377")
RP = 1 << 384
OK, RANGE, CURVE, SUBGROUP = 0, 1, 2, 3
# What the search for small-order points must find: points with x = 0 (order 3), with y = 0 (order 2: all three roots of x^3 = -b or none) and the odd
# primes below 3000 that divide the group order (one point of each order).  Asserted in classes(), so the lists cannot silently become empty.
# BLS12-381: (0, +-2); no 2-torsion (h1 and h2 are odd).  BLS12-377: (0, +-1), (-1, 0) and its two images under x -> w x.  Neither twist has a point with
# x = 0 or y = 0; the cofactor of BLS12-377's twist has no prime factor below 2 000 000 at all, so its G2 has no small-order points to offer.
SMALL_ORDER = {("381", 1): {"x=0": 2, "y=0": 0, "primes": (3, 11)}, ("381", 2): {"x=0": 0, "y=0": 0, "primes": (13, 23, 2713)},
               ("377", 1): {"x=0": 2, "y=0": 3, "primes": (3, 7, 13, 499)}, ("377", 2): {"x=0": 0, "y=0": 0, "primes": ()}}


def sqrt_fp(a, p):
    """a root of a mod p, or None: p = 3 mod 4 on BLS12-381, Tonelli-Shanks (p - 1 = 2^46 t) on BLS12-377"""
    a %= p
    if a == 0: return 0
    if pow(a, (p - 1) // 2, p) != 1: return None
    if p % 4 == 3: return pow(a, (p + 1) // 4, p)
    q, s = p - 1, 0
    while q % 2 == 0: q //= 2; s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1: z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1: t2 = t2 * t2 % p; i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c = i, b * b % p
        t, r = t * c % p, r * b % p
    return r


def sqrt_fp2(a, p, nr):
    """a root of a0 + a1 u in Fp[u] / (u^2 - nr), or None"""
    a0, a1 = a[0] % p, a[1] % p
    sq = lambda x: ((x[0] * x[0] + nr * x[1] * x[1]) % p, 2 * x[0] * x[1] % p)
    if a1 == 0:
        s = sqrt_fp(a0, p)
        if s is not None: return (s, 0)
        s = sqrt_fp(a0 * pow(nr, -1, p), p)
        return None if s is None else (0, s)
    s = sqrt_fp(a0 * a0 - nr * a1 * a1, p)
    if s is None: return None
    for t in ((a0 + s) * pow(2, -1, p) % p, (a0 - s) * pow(2, -1, p) % p):
        x0 = sqrt_fp(t, p)
        if x0:
            r = (x0, a1 * pow(2 * x0, -1, p) % p)
            if sq(r) == (a0, a1): return r
    return None


class Curve:
    def __init__(self, tag):
        import bls377_model, bls381_model
        self.tag, self.M = tag, (bls381_model if tag == "381" else bls377_model)
        M = self.M
        self.P, self.R, self.X = M.P, M.R, M.X
        self.nr = -1 if tag == "381" else -5                                   # u^2
        self.b = {1: 4 if tag == "381" else 1, 2: M.f2muls(M.XI, 4) if tag == "381" else M.B_TWIST}
        self.F = {1: M._Fp, 2: M._Fp2}
        self.gen = {1: M.G1, 2: M.G2}
        x = self.X
        self.h = {1: (x - 1) ** 2 // 3, 2: (x**8 - 4 * x**7 + 5 * x**6 - 4 * x**4 + 6 * x**3 - 4 * x**2 - 4 * x + 13) // 9}      # cofactors: #E(Fp) = h1 r, #E'(Fp2) = h2 r

    def on_curve(self, g, pt): return pt is None or (self.M.g1_on_curve(pt) if g == 1 else self.M.g2_on_curve(pt))
    def mul(self, g, k, pt): return self.M.ec_mul(self.F[g], k, pt)
    def add(self, g, a, b): return self.M.ec_add(self.F[g], a, b)
    def neg(self, g, pt): return self.M.ec_neg(self.F[g], pt)

    def lift(self, g, x, sign=0):
        """the curve point with this x (and the root of the given parity index), or None when x^3 + b has no root"""
        F = self.F[g]
        rhs = F.add(F.mul(F.mul(x, x), x), self.b[g])
        y = sqrt_fp(rhs, self.P) if g == 1 else sqrt_fp2(rhs, self.P, self.nr)
        if y is None: return None
        return (x, F.sub(F.zero, y) if sign else y)

    # ---- raw form ----
    def mont(self, v): return v * RP % self.P
    def raw(self, g, pt):
        if pt is None: return (0,) * (2 * g)
        return (self.mont(pt[0]), self.mont(pt[1])) if g == 1 else (self.mont(pt[0][0]), self.mont(pt[0][1]), self.mont(pt[1][0]), self.mont(pt[1][1]))

    def flag(self, g, raw):
        """the definition"""
        if any(v >= self.P for v in raw): return RANGE
        if not any(raw): return OK
        c = [v * pow(RP, -1, self.P) % self.P for v in raw]
        pt = (c[0], c[1]) if g == 1 else ((c[0], c[1]), (c[2], c[3]))
        if not self.on_curve(g, pt): return CURVE
        return OK if self.mul(g, self.R, pt) is None else SUBGROUP


@functools.lru_cache(maxsize=None)
def curve(tag): return Curve(tag)


def rows(raws):
    """raw points -> the flat C-ABI array (n, 12) / (n, 24) of uint64"""
    if not raws: return np.zeros((0, 12), dtype=np.uint64)
    return np.frombuffer(b"".join(v.to_bytes(48, "little") for r in raws for v in r), dtype=np.uint64).reshape(len(raws), 6 * len(raws[0])).copy()


@functools.lru_cache(maxsize=None)
def classes(tag, g):
    """{class name: [(raw point, flag by the definition), ..]}, at most 32 points per class"""
    C = curve(tag); rng = random.Random("%d/%s/%d" % (SEED, tag, g))
    P, R, u = C.P, C.R, abs(C.X)
    rand_fe = (lambda: rng.randrange(P)) if g == 1 else (lambda: (rng.randrange(P), rng.randrange(P)))

    def random_curve_points(count):
        out = []
        while len(out) < count:
            pt = C.lift(g, rand_fe(), rng.randrange(2))
            if pt is not None: out.append(pt)
        return out

    cls = {}
    ks = [1, 2, R - 1, u, u - 1, u + 1, u * u % R, u * u - 1, u * u + 1] + [rng.randrange(1, R) for _ in range(6)]
    sub = [C.mul(g, k, C.gen[g]) for k in ks]
    cls["subgroup"] = sub + [C.neg(g, p) for p in sub]
    cls["infinity"] = [None]
    outside = random_curve_points(8)
    cls["outside"] = outside
    torsion = [C.mul(g, R, q) for q in outside]
    assert all(t is not None for t in torsion)
    cls["torsion"] = torsion                                                   # pure cofactor torsion: [h] T = O
    cls["mixed"] = [C.add(g, sub[9 + (i % 6)], t) for i, t in enumerate(torsion)]
    # small orders: x = 0 (y^2 = b: order 3) and y = 0 (order 2: found as the 2-part of a curve point)
    small = {"x=0": [], "y=0": []}
    zero = C.F[g].zero
    for s in (0, 1):
        pt = C.lift(g, zero, s)
        if pt is not None and pt[1] != zero and pt not in small["x=0"]: small["x=0"].append(pt)
    N = C.h[g] * R

    def of_order(l):
        """a point of prime order l: the l-part of a curve point, multiplied by l until the next multiple is O (None when l does not divide N)"""
        m = N
        while m % l == 0: m //= l
        if m == N: return None
        for q in outside:
            t = C.mul(g, m, q)
            while t is not None and C.mul(g, l, t) is not None: t = C.mul(g, l, t)
            if t is not None: return t
        raise AssertionError("no point of order %d among the multiples tried" % l)

    t = of_order(2)
    if t is not None:
        assert t[1] == zero
        w = 2
        while pow(w, (P - 1) // 3, P) == 1: w += 1
        w = pow(w, (P - 1) // 3, P)                                            # a primitive cube root of unity: x^3 = -b has the roots x, w x, w^2 x
        small["y=0"] = [(C.F[g].muls(t[0], pow(w, i, P)), zero) for i in range(3)]
        assert all(C.on_curve(g, s) for s in small["y=0"])
    # ... and one point of every other prime order l < 3000 that divides the group order: the chains meet O or +-P within their first steps
    primes = [l for l in range(3, 3000, 2) if N % l == 0 and all(l % q for q in range(3, int(l**0.5) + 1, 2))]
    prime_pts = [of_order(l) for l in primes]
    found = {"x=0": len(small["x=0"]), "y=0": len(small["y=0"]), "primes": tuple(primes)}
    assert found == SMALL_ORDER[(tag, g)], (tag, g, found)
    cls["small"] = small["x=0"] + small["y=0"] + [t for t in prime_pts if t not in small["x=0"] + small["y=0"]]
    raw = {name: [C.raw(g, p) for p in pts] for name, pts in cls.items()}
    F = C.F[g]
    raw["offcurve"] = [C.raw(g, (p[0], F.add(p[1], F.one))) for p in sub[9:13]]
    unred = []
    for i, p in enumerate(sub[9:13]):
        r = list(C.raw(g, p))
        k = [0, 2 * g - 1, g, 1][i] % (2 * g)                                  # G1: x, y, y, y;  G2: x.c0, y.c1, y.c0, x.c1
        r[k] += P
        assert r[k] < 1 << 384
        unred.append(tuple(r))
    raw["unreduced"] = unred
    return {name: [(r, C.flag(g, r)) for r in rs] for name, rs in raw.items()}


@functools.lru_cache(maxsize=None)
def mixed(tag, g):
    """every class in one list of (raw, flag), classes interleaved"""
    c = classes(tag, g)
    out, i = [], 0
    while any(i < len(v) for v in c.values()):
        out += [v[i] for v in c.values() if i < len(v)]
        i += 1
    return out


def vector(tag, g, n):
    """The mixed list rotated by n and cut (or cycled) to length n, with a bad point forced to index 0, to index n - 1 and to both sides of the wave seam
    (63 | 64) and of the block seam (255 | 256) where n reaches them -> (array, flags)."""
    m = mixed(tag, g)
    bad = [e for e in m if e[1] != OK]
    v = [m[(n + i) % len(m)] for i in range(n)]
    for j, i in enumerate(sorted({0, n - 1, 63, 64, 255, 256})):
        if i < n: v[i] = bad[(n + j) % len(bad)]
    return rows([e[0] for e in v]), np.array([e[1] for e in v], dtype=np.uint8)


def valid(tag, g, n):
    """n valid points (cycled from the subgroup class) -> array"""
    s = classes(tag, g)["subgroup"]
    return rows([s[i % len(s)][0] for i in range(n)])


def tampered_images(tag, g, L):
    """[(compress, image, parse result, accepted)] built with the library's own serialisers (host code): a valid point, the identity, and one tampered
    image per class -- a coordinate >= p, bad flag bits, an uncompressed point off the curve, a compressed x without a root, a curve point outside the subgroup"""
    C, cls = curve(tag), classes(tag, g)
    size = {(1, 0): 96, (1, 1): 48, (2, 0): 192, (2, 1): 96}
    fn = {(1, 0): L.ripp_ser_g1, (1, 1): L.ripp_ser_g1_compressed, (2, 0): L.ripp_ser_g2, (2, 1): L.ripp_ser_g2_compressed}

    def ser(raw, c):
        row = rows([raw]); out = np.zeros(size[(g, c)], dtype=np.uint8)
        fn[(g, c)](row.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
        return bytearray(out.tobytes())

    good = cls["subgroup"][9][0]
    k = next(k for k in range(1, 200) if C.lift(g, k if g == 1 else (k, 0)) is None)          # x = k: x^3 + b has no root (y is not in a compressed image)
    noroot = (C.mont(k), C.mont(1)) if g == 1 else (C.mont(k), 0, C.mont(1), 0)
    out = []
    for c in (0, 1):
        out.append((c, ser(good, c), 0, 1))
        out.append((c, ser((0,) * (2 * g), c), 0, 1))
        img = ser(good, c)                                                      # the first coordinate in the image := p
        if tag == "381": pb = bytearray(C.P.to_bytes(48, "big")); pb[0] |= img[0] & 0xE0; img[0:48] = pb
        else: pb = bytearray(C.P.to_bytes(48, "little")); pb[47] |= img[47] & 0xC0 if (g == 1 and c == 1) else 0; img[0:48] = pb
        out.append((c, img, 1, 0))
        img = ser(good, c)                                                      # flag bits: the compression bit of the zcash layout flipped / both SWFlags set
        if tag == "381": img[0] ^= 0x80
        else: img[-1] |= 0xC0
        out.append((c, img, 1, 0))
        if c == 0: out.append((c, ser(cls["offcurve"][0][0], c), 2, 0))
        else: out.append((c, ser(tuple(noroot), c), 2, 0))
        out.append((c, ser(cls["outside"][0][0], c), 0, 0))                    # parses; the subgroup test rejects it
    return out


def summary(flags):
    """(n_bad, first_bad) of a flag vector; for (n, 3) proof flags an item is bad when any member is"""
    f = np.asarray(flags)
    b = (f != 0) if f.ndim == 1 else (f != 0).any(axis=1)
    idx = np.flatnonzero(b)
    return len(idx), int(idx[0]) if len(idx) else len(f)
