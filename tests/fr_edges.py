"""The cases and the Python-integer model for the scalar-field kernels and the 32-bit Montgomery form Mont<P> (ripp_amd/csrc/bls12_381/fp.hpp), per curve
("381" / "377"), shared by tests/test_fr_edges_model_cpu.py (the conditions on the case lists, the scan model against suffix Horner, the digit model) and
tests/test_gpu_fr_edges.py (the device code through tests/device/fr_edges.hip).

The moduli come from orclib / orclib377, |x| and lambda from the existing input modules (tipa_generic_inputs, orclib377's x) with lambda = x^2 - 1; nothing is
read from the headers under test.  Everything is exact integer arithmetic."""
import functools
import random

import orclib
import orclib377
import fold_edge_scalars as FES
import tipa_generic_inputs as TGI

TAGS = ["381", "377"]
N_RANDOM = 200
N_FORCED = 30                       # products built to land in the t >= m branch (below)
KZG_CHUNK, KZG_SCAN_LANES = 64, 256


class Field:
    def __init__(self, name, m, nlimb):
        self.name, self.m, self.N = name, m, nlimb
        self.bits = 32 * nlimb
        self.R = 1 << self.bits
        self.minv = pow(-m, -1, self.R)                             # -m^-1 mod R
        self.rinv = pow(self.R, -1, m)

    def mont(self, v): return v * self.R % self.m
    def plain(self, w): return w * self.rinv % self.m

    def redc_t(self, x):
        """the unsubtracted Montgomery value t = (x + q m) / R, q = -x m^-1 mod R, of x < m R: what mul / mul_cios / mul2_add hold before reduce_once"""
        q = x * self.minv % self.R
        t, rem = divmod(x + q * self.m, self.R)
        assert rem == 0 and t < 2 * self.m
        return t


class Curve:
    def __init__(self, tag):
        o = orclib if tag == "381" else orclib377
        self.tag, self.r, self.p = tag, o.R, o.P
        self.x = TGI.X_ABS if tag == "381" else 0x8508C00000000001
        self.lam = self.x * self.x - 1
        assert self.r == self.x**4 - self.x**2 + 1 and (self.lam * self.lam + self.lam + 1) % self.r == 0
        if tag == "381": assert self.lam == TGI.LAMBDA
        self.fr, self.fp = Field("fr", self.r, 8), Field("fp", self.p, 12)

    def field(self, name): return self.fr if name == "fr" else self.fp


CURVES = {t: Curve(t) for t in TAGS}


def _unique(seq):
    seen, out = set(), []
    for v in seq:
        if v not in seen:
            seen.add(v); out.append(v)
    return out


# ---- operands of the Montgomery operations --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structured(tag, fname):
    F = CURVES[tag].field(fname)
    m = F.m
    vals = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, F.R % m, F.R * F.R % m]
    for k in range(1, F.N):
        vals += [v for v in (1 << (32 * k), (1 << (32 * k)) - 1) if v < m]
    low = (1 << (32 * (F.N - 1))) - 1                                   # the largest value below m whose low N - 1 limbs are all ones
    top = m >> (32 * (F.N - 1))
    vals.append(((top << (32 * (F.N - 1))) | low) if ((top << (32 * (F.N - 1))) | low) < m else (((top - 1) << (32 * (F.N - 1))) | low))
    assert all(0 <= v < m for v in vals)
    return tuple(_unique(vals))


@functools.lru_cache(maxsize=None)
def randoms(tag, fname):
    F = CURVES[tag].field(fname)
    rnd = random.Random("fr_edges %s %s" % (tag, fname))
    return tuple(rnd.randrange(F.m) for _ in range(N_RANDOM))


def operands(tag, fname):
    return structured(tag, fname) + randoms(tag, fname)


@functools.lru_cache(maxsize=None)
def mul_cases(tag, fname):
    """(a, b): every structured pair, the random values against their neighbours and against every structured value's first partner, and N_FORCED products built
    for the t >= m branch: for a random odd a and a quotient word q = R - 1 - j, b = -q m a^-1 mod R gives a b = -q m (mod R), kept when b < m"""
    F = CURVES[tag].field(fname)
    s, r = structured(tag, fname), randoms(tag, fname)
    cases = [(a, b) for a in s for b in s]
    cases += [(r[i], r[(i + 1) % len(r)]) for i in range(len(r))]
    cases += [(r[i], s[i % len(s)]) for i in range(len(r))]
    rnd = random.Random("fr_edges forced %s %s" % (tag, fname))
    forced = []
    while len(forced) < N_FORCED:
        a = rnd.randrange(F.m) | 1
        if a >= F.m: continue
        q = F.R - 1 - rnd.randrange(1 << 16)
        b = -q * F.m * pow(a, -1, F.R) % F.R
        if b < F.m and F.redc_t(a * b) >= F.m: forced.append((a, b))
    return tuple(cases + forced)


@functools.lru_cache(maxsize=None)
def mul2_cases(tag, fname="fp"):
    """(a, b, c, d) for mul2_add: structured and random quadruples, and N_FORCED built for the t >= m branch as in mul_cases (d solves c d = -q m - a b mod R)"""
    F = CURVES[tag].field(fname)
    s, r = structured(tag, fname), randoms(tag, fname)
    big = [F.m - 1, F.m - 2, (F.m + 1) // 2, s[-1]]
    cases = [(a, b, c, d) for a in big for b in big for c in big[:2] for d in big[:2]]
    cases += [(s[i], s[(i * 7 + 1) % len(s)], s[(i * 3 + 2) % len(s)], s[(i * 5 + 3) % len(s)]) for i in range(len(s))]
    cases += [(0, a, 0, a) for a in big] + [(a, 0, b, 0) for a, b in zip(big, big[1:])] + [(F.m - 1, F.m - 1, 0, 0), (0, 0, F.m - 1, F.m - 1), (1, 1, 1, 1)]
    cases += [(r[i], r[(i + 1) % len(r)], r[(i + 2) % len(r)], r[(i + 3) % len(r)]) for i in range(len(r))]
    rnd = random.Random("fr_edges forced2 %s %s" % (tag, fname))
    forced = []
    while len(forced) < N_FORCED:
        a, b, c = rnd.randrange(F.m), rnd.randrange(F.m), rnd.randrange(F.m) | 1
        if c >= F.m: continue
        q = F.R - 1 - rnd.randrange(1 << 16)
        d = (-q * F.m - a * b) * pow(c, -1, F.R) % F.R
        if d < F.m and F.redc_t(a * b + c * d) >= F.m: forced.append((a, b, c, d))
    return tuple(cases + forced)


@functools.lru_cache(maxsize=None)
def add_cases(tag, fname):
    """every structured pair, random pairs, and for many a the b with a + b in {m - 1, m, m + 1, 2 m - 2} (both sides of reduce_once's branch, and its largest input)"""
    F = CURVES[tag].field(fname)
    m, s, r = F.m, structured(tag, fname), randoms(tag, fname)
    cases = [(a, b) for a in s for b in s] + [(r[i], r[(i + 1) % len(r)]) for i in range(len(r))]
    for a in operands(tag, fname):
        for target in (m - 1, m, m + 1, 2 * m - 2):
            b = target - a
            if 0 <= b < m: cases.append((a, b))
    return tuple(_unique(cases))


@functools.lru_cache(maxsize=None)
def sub_cases(tag, fname):
    """every structured pair, random pairs, a = b, (0, m - 1), (m - 1, 0), a = b - 1"""
    F = CURVES[tag].field(fname)
    m, s, r = F.m, structured(tag, fname), randoms(tag, fname)
    cases = [(a, b) for a in s for b in s] + [(r[i], r[(i + 1) % len(r)]) for i in range(len(r))]
    cases += [(a, a) for a in operands(tag, fname)] + [(0, m - 1), (m - 1, 0)] + [(b - 1, b) for b in operands(tag, fname) if b >= 1]
    return tuple(_unique(cases))


def expect(tag, fname, op, args):
    """the raw result of the device operation on raw operands (R = 2^(32 N)): the products carry one factor R^-1"""
    F = CURVES[tag].field(fname)
    m, ri = F.m, F.rinv
    if op in ("mul", "mul_cios"): return args[0] * args[1] * ri % m
    if op == "sqr": return args[0] * args[0] * ri % m
    if op == "add": return (args[0] + args[1]) % m
    if op == "sub": return (args[0] - args[1]) % m
    if op == "neg": return -args[0] % m
    if op == "from_mont": return args[0] * ri % m
    if op == "to_mont": return args[0] * F.R % m
    if op == "mul2_add": return (args[0] * args[1] + args[2] * args[3]) * ri % m
    raise KeyError(op)


def branch_counts(tag, fname, cases):
    """(number of cases with t < m, with t >= m) of the unsubtracted Montgomery value of a b (+ c d)"""
    F = CURVES[tag].field(fname)
    hi = sum(1 for c in cases if F.redc_t(c[0] * c[1] + (c[2] * c[3] if len(c) == 4 else 0)) >= F.m)
    return len(cases) - hi, hi


# ---- msm_divmod ----------------------------------------------------------------------------------------------------------------------------------------
N_MULTIPLES = 24


def divisor(tag, which):
    C = CURVES[tag]
    return C.lam if which == "lambda" else C.x


@functools.lru_cache(maxsize=None)
def divmod_cases(tag):
    """canonical k < r for both divisors: the Fr operands, the fold / scaling edges, j d and j d - 1 for j in {1, 2, 3, floor(r / d)}, r - 1, and N_MULTIPLES random
    multiples of each divisor (every exact multiple takes the correction step)"""
    C = CURVES[tag]
    r = C.r
    ks = list(operands(tag, "fr")) + [v % r for v in FES.scalars(tag)]
    rnd = random.Random("fr_edges divmod " + tag)
    for d in (C.lam, C.x):
        for j in (1, 2, 3, r // d):
            ks += [j * d, j * d - 1]
        ks += [rnd.randrange(1, r // d) * d for _ in range(N_MULTIPLES)]
    ks.append(r - 1)
    assert all(0 <= k < r for k in ks)
    return tuple(_unique(ks))


def barrett_shortfall(k, d):
    """floor(k / d) - floor(k mu / 2^256), mu = floor(2^256 / d): the number of corrections msm_divmod's loop makes"""
    return k // d - ((k * ((1 << 256) // d)) >> 256)


def x_chain(tag, k):
    """the three divisions of the GLS branch: [(quotient, remainder)] * 3; the digits are the remainders and the last quotient"""
    x, out = CURVES[tag].x, []
    for _ in range(3):
        k, rem = divmod(k, x)
        out.append((k, rem))
    return out


# ---- digit passes --------------------------------------------------------------------------------------------------------------------------------------
NBITS = {1: 255, 2: 128, 4: 64}


def components(tag, k, split):
    """the split of canonical k the digit passes make: itself; (remainder, quotient) by lambda; the four base-|x| digits"""
    C = CURVES[tag]
    if split == 1: return [k]
    if split == 2: return [k % C.lam, k // C.lam]
    return [k // C.x**j % C.x for j in range(3)] + [k // C.x**3]


def windows(v, c, nwin):
    return [(v >> (w * c)) & ((1 << c) - 1) for w in range(nwin)]


def check_plan(plan, split, nreal):
    """what every plan the tests use must satisfy for the digit model to hold; plan = dict(c, nwin, nb, n, nreal, ...) as the harness returns it"""
    assert 4 <= plan["c"] <= 13 and plan["nb"] == 1 << plan["c"] and plan["nreal"] == nreal and plan["n"] == split * nreal, plan
    assert plan["nwin"] * plan["c"] >= NBITS[split] and (plan["nwin"] - 1) * plan["c"] < NBITS[split], plan


def check_digit_model(tag, k, split, plan):
    """components below 2^nbits, and the windows reconstruct each exactly"""
    comps = components(tag, k, split)
    C = CURVES[tag]
    assert sum(v * (1 if split == 1 else C.lam if split == 2 else C.x) ** j for j, v in enumerate(comps)) == k
    for v in comps:
        assert 0 <= v < 1 << NBITS[split], (hex(k), split)
        ws = windows(v, plan["c"], plan["nwin"])
        assert sum(d << (w * plan["c"]) for w, d in enumerate(ws)) == v and all(d < plan["nb"] for d in ws)
    return comps


def expected_digits(tag, plan, split, rows, placement):
    """placement: {(row, base position): canonical scalar}.  Returns the whole digit buffer [rows][nwin][n] as a flat list: term j * nreal + position of window w
    holds window w of component j of the scalar placed there, every other digit is zero"""
    nwin, n, nreal, c = plan["nwin"], plan["n"], plan["nreal"], plan["c"]
    out = [0] * (rows * nwin * n)
    for (row, pos), k in placement.items():
        assert 0 <= row < rows and 0 <= pos < nreal
        for j, v in enumerate(components(tag, k, split)):
            for w, d in enumerate(windows(v, c, nwin)):
                out[(row * nwin + w) * n + j * nreal + pos] = d
    return out


def histogram(plan, digits):
    """the counts k_msm_digits adds up: per window, the non-zero digits"""
    nwin, n, nb = plan["nwin"], plan["n"], plan["nb"]
    h = [0] * (nwin * nb)
    for w in range(nwin):
        for d in digits[w * n:(w + 1) * n]:
            if d: h[w * nb + d] += 1
    return h


def digit_scalars(tag, count, seed):
    """`count` canonical scalars for a digit pass: the split edges first (cycled if count is small), then seeded random ones, with 0 and r - 1 always present"""
    C = CURVES[tag]
    edge = [C.r - 1, 0, C.lam, C.lam - 1, (C.r - 1) // C.lam * C.lam, C.x, C.x - 1, C.x**3, C.x**3 - 1, (1 << 128) - 1, (C.x - 1) * (1 + C.x + C.x**2 + C.x**3) % C.r, 1, (1 << 64) - 1]
    rnd = random.Random("fr_edges digits %s %d" % (tag, seed))
    return [edge[i] if i < len(edge) else rnd.randrange(C.r) for i in range(count)]


# ---- the KZG scan ---------------------------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 64 * 255 + 1, 64 * 256 - 1, 64 * 256, 64 * 256 + 1, 64 * 257, 64 * 257 + 63, 64 * 510 + 1, 64 * 511, 64 * 512, 64 * 512 + 1,
              64 * 513 + 5, 64 * 768, 64 * 768 + 1]
SCAN_OVERRIDES = [(323, 1), (323, 2), (64 * 300, 5), (64 * 257 + 1, 3)]
SCAN_POINTS_ALL = ["zero", "one", "minus_one", "two", "random", "order64", "order128"]
SCAN_POINTS_LARGE = ["random", "minus_one", "order128"]
SCAN_POLYS = ["random", "all_minus_one", "top_only", "root"]


def scan_cases():
    """(m, per override or 0, point names)"""
    return [(m, 0, SCAN_POINTS_ALL if m <= 129 else SCAN_POINTS_LARGE) for m in SCAN_SIZES] + [(m, per, SCAN_POINTS_LARGE) for m, per in SCAN_OVERRIDES]


@functools.lru_cache(maxsize=None)
def scan_point(tag, name):
    r = CURVES[tag].r
    if name in ("order64", "order128"):
        a = 2
        while True:
            g = pow(a, (r - 1) // 128, r)
            if pow(g, 64, r) == r - 1: break
            a += 1
        z = g if name == "order128" else g * g % r
        assert pow(z, 64, r) == (r - 1 if name == "order128" else 1) and pow(z, 32, r) != 1
        return z
    return {"zero": 0, "one": 1, "minus_one": r - 1, "two": 2, "random": random.Random("fr_edges z " + tag).randrange(2, r - 1)}[name]


@functools.lru_cache(maxsize=None)
def _random_poly(tag, m):
    rnd = random.Random("fr_edges poly %s %d" % (tag, m))
    r = CURVES[tag].r
    return tuple(rnd.randrange(r) for _ in range(m))


def scan_poly(tag, m, kind, z):
    r = CURVES[tag].r
    if kind == "random": return list(_random_poly(tag, m))
    if kind == "all_minus_one": return [r - 1] * m
    if kind == "top_only": return [0] * (m - 1) + [_random_poly(tag, 1)[0] | 1]
    if m == 1: return [0]
    s = _random_poly(tag, m - 1)                                       # (X - z) s(X)
    return [((s[i - 1] if i else 0) - (z * s[i] if i < m - 1 else 0)) % r for i in range(m)]


def suffix_horner(p, z, r):
    """s[j] = sum_{k >= j} p[k] z^(k - j): the quotient of p by (X - z) is s[1:], p(z) = s[0]"""
    s, acc = [0] * len(p), 0
    for k in range(len(p) - 1, -1, -1):
        acc = (acc * z + p[k]) % r
        s[k] = acc
    return s


def scan_model(p, z, r, per=0):
    """k_kzg_chunk_sums, k_kzg_carry_scan, k_kzg_quotient (ripp_amd/csrc/msm_batch.hpp) restated lane by lane with the launch parameters of kzg_quotient_launch.
    Returns (h, cin, q, eval): q has m - 1 entries"""
    m = len(p)
    nchunk = (m + KZG_CHUNK - 1) // KZG_CHUNK
    per = per or (nchunk + KZG_SCAN_LANES - 1) // KZG_SCAN_LANES
    assert per * KZG_SCAN_LANES >= nchunk
    zT = pow(z, KZG_CHUNK, r); zTper = pow(zT, per, r)
    h = [0] * nchunk
    for c in range(nchunk):
        acc = 0
        for k in range(min(c * KZG_CHUNK + KZG_CHUNK, m) - 1, c * KZG_CHUNK - 1, -1): acc = (acc * z + p[k]) % r
        h[c] = acc
    rng = [(min(l * per, nchunk), min(l * per + per, nchunk)) for l in range(KZG_SCAN_LANES)]
    sh = []
    for lo, hi in rng:
        acc = 0
        for c in range(hi - 1, lo - 1, -1): acc = (acc * zT + h[c]) % r
        sh.append(acc)
    run = 0
    for t in range(KZG_SCAN_LANES - 1, -1, -1):
        own = sh[t]; sh[t] = run; run = (run * zTper + own) % r
    cin = [None] * nchunk
    for l, (lo, hi) in enumerate(rng):
        run = sh[l]
        for c in range(hi - 1, lo - 1, -1):
            cin[c] = run; run = (run * zT + h[c]) % r
    q, ev = [None] * (m - 1), None
    for c in range(nchunk):
        acc = cin[c]
        for k in range(min(c * KZG_CHUNK + KZG_CHUNK, m) - 1, c * KZG_CHUNK - 1, -1):
            acc = (acc * z + p[k]) % r
            if k: q[k - 1] = acc
            else: ev = acc
    return h, cin, q, ev
