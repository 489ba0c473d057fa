"""Inputs and reference for the stage-1 tests (TEST INFRASTRUCTURE ONLY): the Miller lines of a pair (P, Q) step by step in Python integers, the rule
that compares a stored line with them, and the point sets of tests/test_miller_edges_cpu.py and tests/test_gpu_miller_edges.py.

Reference.  The homogeneous doubling and addition steps bls12_381/pairing.hpp documents (line_double, line_add, M-type twist on BLS12-381 and D-type on
BLS12-377), evaluated over the Fp2 of tests/model, started at T = Q, Z = 1 and walked over the bits of |x| below the top one.  A step's line is the
triple of Fp2 coefficients in the order the kernels store it (kernels.hpp LINE_SLOT_*): (free, xP-scaled, yP-scaled) at w^0, w^2, w^3 on BLS12-381,
(yP-scaled, xP-scaled, free) at w^0, w^1, w^3 on BLS12-377.

Comparison.  The kernels walk other representatives of the same projective point (the VM carries 4 s^2 x the doubled point, k_miller_lines_q -4 x it
and stores every coefficient times 2^8, its addition line negated): a stored triple equals k x the reference triple for ONE k in Fp, k != 0, which the
final exponentiation removes.  scale_equal checks exactly that, with no tolerance: k is fixed by the first non-zero Fp component of the reference and all
six components must agree.  A factor from Fp2 \\ Fp is NOT removed by regrouping the per-step products and is rejected.

Point sets.  (a) distinct subgroup points P_i = [i + 1] G1, Q_i = [i + 1] G2 built by repeated addition; (b) curve points with coordinates at the ends
of the field -- they need NOT lie in the prime-order subgroups: the line kernels are defined on any curve point, and the final exponentiation of the
combined lines is still the value every correct Miller loop gives; (c) infinity as (0, 0)."""
import functools

import bls377_model as m377
import bls381_model as m381

MODELS = {"381": m381, "377": m377}
R384 = 1 << 384
EDGE_SEARCH = 64
LINE_POS = {"381": (0, 2, 3), "377": (0, 1, 3)}          # the power of w each stored coefficient multiplies


class Curve:
    def __init__(self, tag):
        self.tag, self.m = tag, MODELS[tag]
        m = self.m
        self.P = m.P
        self.x_abs = m.X_ABS if tag == "381" else m.X
        self.bits = bin(self.x_abs)[3:]                                   # the 63 bits below the top one, high to low
        self.n_lines = len(self.bits) + self.bits.count("1")
        self.conj = tag == "381"                                          # x < 0
        self.b = 4 if tag == "381" else 1
        self.b_twist = m.f2muls(m.XI, 4) if tag == "381" else m.B_TWIST
        self.beta = -1 if tag == "381" else m.BETA                        # u^2
        self.one_m = R384 % self.P                                        # Montgomery-384 one
        self.rinv = pow(R384, -1, self.P)
        self.i2 = pow(2, -1, self.P)


CURVES = {t: Curve(t) for t in MODELS}


# ---- field helpers the models lack -------------------------------------------------------------------------------------------------------------------
def fp_sqrt(P, a):
    """a square root of a mod P (Tonelli-Shanks: BLS12-377's p - 1 is divisible by 2^46), or None"""
    a %= P
    if a == 0: return 0
    if pow(a, (P - 1) // 2, P) != 1: return None
    q, s = P - 1, 0
    while q % 2 == 0: q //= 2; s += 1
    z = 2
    while pow(z, (P - 1) // 2, P) != P - 1: z += 1
    c, x, t, mm = pow(z, q, P), pow(a, (q + 1) // 2, P), pow(a, q, P), s
    while t != 1:
        i, t2 = 0, t
        while t2 != 1: t2 = t2 * t2 % P; i += 1
        b = pow(c, 1 << (mm - i - 1), P)
        x, c, mm = x * b % P, b * b % P, i
        t = t * c % P
    return x


def f2_sqrt(C, a):
    """a square root of a = a0 + a1 u in Fp2 = Fp[u]/(u^2 - beta), or None:  with s^2 = N(a) = a0^2 - beta a1^2 and x0^2 = (a0 + s) / 2, x1 = a1 / (2 x0)"""
    P, a0, a1 = C.P, a[0] % C.P, a[1] % C.P
    if a0 == 0 and a1 == 0: return (0, 0)
    s = fp_sqrt(P, a0 * a0 - C.beta * a1 * a1)
    if s is None: return None
    for sg in (s, P - s):
        h = (a0 + sg) * C.i2 % P
        if h == 0: continue
        x0 = fp_sqrt(P, h)
        if x0 is None: continue
        r = (x0, a1 * pow(2 * x0, -1, P) % P)
        if C.m.f2mul(r, r) == (a0, a1): return r
    if a1 == 0:                                                            # a0 is no square in Fp: the root is purely imaginary, x1^2 = a0 / beta
        x1 = fp_sqrt(P, a0 * pow(C.beta, -1, P))
        if x1 is not None and C.m.f2mul((0, x1), (0, x1)) == (a0, 0): return (0, x1)
    return None


# ---- one step ------------------------------------------------------------------------------------------------------------------------------------
def _slots(C, free, cx, cy): return (free, cx, cy) if C.tag == "381" else (cy, cx, free)


def step_double(C, T):
    """pairing.hpp line_double without P: T <- 2T and the line's (free, xP-factor, yP-factor) = (i, 3 j, -h)"""
    m = C.m
    X, Y, Z = T
    a = m.f2muls(m.f2mul(X, Y), C.i2)
    b, c = m.f2mul(Y, Y), m.f2mul(Z, Z)
    e = m.f2mul(C.b_twist, m.f2muls(c, 3))
    f = m.f2muls(e, 3)
    g = m.f2muls(m.f2add(b, f), C.i2)
    yz = m.f2add(Y, Z)
    h = m.f2sub(m.f2mul(yz, yz), m.f2add(b, c))
    i = m.f2sub(e, b)
    j = m.f2mul(X, X)
    e2 = m.f2mul(e, e)
    T2 = (m.f2mul(a, m.f2sub(b, f)), m.f2sub(m.f2mul(g, g), m.f2muls(e2, 3)), m.f2mul(b, h))
    return T2, (i, m.f2muls(j, 3), m.f2neg(h))


def step_add(C, T, Q):
    """pairing.hpp line_add without P: T <- T + Q (Q affine) and (free, xP-factor, yP-factor) = (j, -theta, lambda); also (theta, lambda)"""
    m = C.m
    X, Y, Z = T
    qx, qy = Q
    theta, lam = m.f2sub(Y, m.f2mul(qy, Z)), m.f2sub(X, m.f2mul(qx, Z))
    c, d = m.f2mul(theta, theta), m.f2mul(lam, lam)
    e, f, g = m.f2mul(lam, d), m.f2mul(Z, c), m.f2mul(X, d)
    h = m.f2sub(m.f2add(e, f), m.f2muls(g, 2))
    T2 = (m.f2mul(lam, h), m.f2sub(m.f2mul(theta, m.f2sub(g, h)), m.f2mul(e, Y)), m.f2mul(Z, e))
    j = m.f2sub(m.f2mul(theta, qx), m.f2mul(lam, qy))
    return T2, (j, m.f2neg(theta), lam), (theta, lam)


_chain_cache = {}


def chain(tag, Q):
    """Q's chain: ([(free, xP-factor, yP-factor)] per step, degenerate) -- degenerate when a step reaches Z = 0 or theta = lambda = 0 (T = +-Q or a
    point of small order on the way): the projective formulas then stop describing the line"""
    key = (tag, Q)
    if key not in _chain_cache:
        C = CURVES[tag]
        T, out, bad = (Q[0], Q[1], (1, 0)), [], False
        for bit in C.bits:
            T, l = step_double(C, T); out.append(l); bad |= T[2] == (0, 0)
            if bit == "1":
                T, l, (theta, lam) = step_add(C, T, Q); out.append(l)
                bad |= T[2] == (0, 0) or (theta == (0, 0) and lam == (0, 0))
        assert len(out) == C.n_lines
        _chain_cache[key] = (out, bad)
    return _chain_cache[key]


def ref_lines(tag, Pt, Q):
    """the N_LINES reference triples of the pair in stored slot order, each a tuple of six Fp components; None for a pair with a point at infinity"""
    if Pt is None or Q is None: return None
    C = CURVES[tag]
    m = C.m
    steps, _ = chain(tag, Q)
    out = []
    for free, cx, cy in steps:
        t = _slots(C, free, m.f2muls(cx, Pt[0]), m.f2muls(cy, Pt[1]))
        out.append((t[0][0], t[0][1], t[1][0], t[1][1], t[2][0], t[2][1]))
    return out


def unit_words(tag):
    """the 72 words of the unit line: Montgomery-384 one at w^0, zero elsewhere"""
    one = CURVES[tag].one_m
    return [(one >> (32 * k)) & 0xFFFFFFFF for k in range(12)] + [0] * 60


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------------------
def scale_equal(P, got, ref):
    """got == k ref for one k in Fp, k != 0 (six Fp components each); cross-multiplied, so no inverse"""
    assert len(got) == 6 and len(ref) == 6
    j = next((i for i in range(6) if ref[i] % P), None)
    assert j is not None, "an all-zero reference line"
    if got[j] % P == 0: return False
    return all(got[i] * ref[j] % P == ref[i] * got[j] % P for i in range(6))


def decode(C, v):
    """stored integer (12 words) -> the field element it stands for as a Montgomery-384 value"""
    return v * C.rinv % C.P


def line_to_f12(C, t):
    """six Fp components in stored order -> the model's flat Fp12 (coefficients of w^0 .. w^5)"""
    f = [(0, 0)] * 6
    for k, pos in enumerate(LINE_POS[C.tag]): f[pos] = (t[2 * k] % C.P, t[2 * k + 1] % C.P)
    return f


def combine(C, lines):
    """miller_combine (pairing.hpp) on one pair's lines: f <- f^2 l per bit, f <- f l after a set bit, conjugated on BLS12-381"""
    m = C.m
    f, s = m.F12_ONE, 0
    for bit in C.bits:
        f = m.f12mul(m.f12mul(f, f), line_to_f12(C, lines[s])); s += 1
        if bit == "1":
            f = m.f12mul(f, line_to_f12(C, lines[s])); s += 1
    assert s == C.n_lines
    return m.f12conj(f) if C.conj else f


@functools.lru_cache(maxsize=None)
def model_pairing(tag, Pt, Q): return CURVES[tag].m.pairing(Pt, Q)


# ---- point sets ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def subgroup_points(tag, n):
    """(a): ([P_0 .. P_{n-1}], [Q_0 .. Q_{n-1}]), P_i = [i + 1] G1, Q_i = [i + 1] G2 by repeated addition"""
    m = MODELS[tag]
    ps, qs, p, q = [], [], None, None
    for _ in range(n):
        p, q = m.g1_add(p, m.G1), m.g2_add(q, m.G2)
        ps.append(p); qs.append(q)
    return ps, qs


def g1_on_curve(C, pt): return (pt[1] * pt[1] - pt[0] ** 3 - C.b) % C.P == 0
def g2_on_curve(C, q):
    m = C.m
    return m.f2sub(m.f2mul(q[1], q[1]), m.f2add(m.f2mul(m.f2mul(q[0], q[0]), q[0]), C.b_twist)) == (0, 0)


def _g1_roots(C, x):
    y = fp_sqrt(C.P, x ** 3 + C.b)
    if y is None: return []
    return sorted({(x % C.P, y), (x % C.P, (C.P - y) % C.P)})


@functools.lru_cache(maxsize=None)
def edge_g1(tag):
    """(b), G1: from x = 0 upwards and from x = p - 1 downwards, the first x with x^3 + b a square, with both roots y.  Where the two roots coincide
    (BLS12-377: x = p - 1 gives y = 0) the search goes on to the next x as well, so that each end contributes at least two distinct points."""
    C = CURVES[tag]
    out = []
    for start, step in ((0, 1), (C.P - 1, -1)):
        got, x = [], start
        while len(got) < 2:
            got += _g1_roots(C, x); x += step
        out += got
    return out


@functools.lru_cache(maxsize=None)
def edge_g2(tag):
    """(b), G2: for each family x = (c, 0), (0, c), (p - 1 - c, p - 1 - c), c = 0, 1, ..: the first x with x^3 + b' a square whose points have no
    degenerate chain (chain()), with both roots y; also the number of candidates skipped for a degenerate chain.  The search of a family stops after
    EDGE_SEARCH values of c: on BLS12-377 the family (0, c) has no point at all (x^3 + b' = (0, -5 c^3 - 1/5) is purely imaginary, its norm 5 k^2 is
    no square in Fp as u^2 = -5 is none and -1 is one, so it is no square in Fp2)"""
    C = CURVES[tag]
    m = C.m
    out, skipped = [], 0
    for fam in (lambda c: (c, 0), lambda c: (0, c), lambda c: (C.P - 1 - c, C.P - 1 - c)):
        for c in range(EDGE_SEARCH):
            x = fam(c)
            y = f2_sqrt(C, m.f2add(m.f2mul(m.f2mul(x, x), x), C.b_twist))
            if y is None: continue
            pts = sorted({(x, y), (x, m.f2neg(y))})
            if any(p in out for p in pts): continue                        # (0, 0) opens two families
            if any(chain(tag, p)[1] for p in pts): skipped += 1; continue
            out += pts
            break
    return out, skipped
