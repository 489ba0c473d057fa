"""Limb-level models (Python integers) of the two device inversions of ripp_amd/csrc/bls12_381/fp_inv.hpp, for either prime the header is
compiled for (curve "381" / "377").

fp_inv_bingcd -- inv(), inv_trace(): binary GCD with K = 30 inner steps on 64-bit approximations, ITER = ceil((2 BITS - 1) / 30) = 26 outer iterations,
exact division by 2^30 of (a, b) and modular division of (u, v) per outer iteration (Pornin, eprint 2020/972, Alg. 2), on 14 limbs of 28 bits, followed by
the device's tail: v + 64 p, one float32 quotient estimate (numpy float32), r = V - q p, canonical.  Every step asserts what the device code relies on:
the window is one of its three forms and fits 64 bits, factor bounds, 64-bit columns, exact divisibility, int32 top limbs, |u|, |v| < 64 p, a = 0 and
b = 1 after ITER iterations, top limb < 2^24 before the float conversion, 0 <= r < 2p after the estimate.

fp_inv_kaliski -- kaliski(): the bit-serial almost-Montgomery inverse with its 13-limb r, s and the final reduction (asserts k <= 768, r < 2p).

Both return the PLAIN inverse of the integer the 12 input words hold; device_result() is what the routines store: that inverse times R^3 in one
Montgomery product, i.e. times 2^768."""
import random

import numpy as np

PRIMES = {
    "381": 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
    "377": 0x01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001,
}
W, NL, MASK = 28, 14, (1 << 28) - 1
K = 30
KMASK = (1 << K) - 1
RBITS = 384                                  # the radix of the 12 x 32-bit Montgomery form (fp.hpp)


class Curve:
    def __init__(self, tag):
        self.tag, self.P = tag, PRIMES[tag]
        self.BITS = self.P.bit_length()
        self.ITER = (2 * self.BITS - 1 + K - 1) // K
        self.MINV = (-pow(self.P, -1, 1 << K)) % (1 << K)
        self.PL = [(self.P >> (W * i)) & MASK for i in range(NL)]
        self.P_TOP = self.PL[NL - 1]                                   # p >> 364
        # constexpr float INV = (1.0f - 1.0f / 1048576.0f) / (float)(P_TOP + 1)
        self.QINV = (np.float32(1.0) - np.float32(1.0) / np.float32(1048576.0)) / np.float32(self.P_TOP + 1)


CURVES = {tag: Curve(tag) for tag in PRIMES}
P, ITER = CURVES["381"].P, CURVES["381"].ITER


def to_limbs(x): return [(x >> (W * i)) & MASK for i in range(NL)]
def val(l): return sum(v << (W * i) for i, v in enumerate(l))       # top limb may be negative


def carry_shr(col):
    """the device's carry_shr: a signed carry pass over 64-bit columns (the top word keeps the rest), then the exact division by 2^30"""
    assert all(-(1 << 63) <= c < (1 << 63) for c in col)
    l, c = [], 0
    for i in range(NL - 1):
        t = col[i] + c
        assert -(1 << 63) <= t < (1 << 63)
        l.append(t & MASK); c = t >> W
    T = col[NL - 1] + c
    assert -(1 << 63) <= T < (1 << 63)
    assert l[0] == 0 and (l[1] & 3) == 0, "not divisible by 2^30"
    out = [(l[j + 1] >> 2) | ((l[j + 2] & 3) << 26) for j in range(NL - 3)]
    out.append((l[NL - 2] >> 2) | ((T & 3) << 26))
    out.append((T >> 2) & MASK)
    out.append(T >> 30)
    assert -(1 << 31) <= out[NL - 1] < (1 << 31), "top limb leaves int32"
    assert val(out) << 30 == val(col)
    return out


def negate(l):
    r, c = [], 0
    for i in range(NL - 1):
        t = -l[i] + c; r.append(t & MASK); c = t >> W
    r.append(-l[NL - 1] + c)
    return r


def window(a, b):
    """the 64-bit approximations of the device loop and the form they took: "exact56" (no limb above the second is set), "exact64" (bit length <= 64:
    the values themselves), "top34" (low 30 bits + the 34 bits below the top bit of a | b)"""
    assert all(0 <= x <= MASK for x in a[:NL - 1] + b[:NL - 1]) and 0 <= a[NL - 1] < (1 << 28) and 0 <= b[NL - 1] < (1 << 28)
    lo_a, lo_b = a[0] | (a[1] << W), b[0] | (b[1] << W)
    w = next((i for i in range(NL - 1, 1, -1) if (a[i] | b[i]) != 0), None)
    if w is None:
        return lo_a, lo_b, "exact56"
    nb = (a[w] | b[w]).bit_length()                                   # 1..28
    if w == 2 and nb <= 8:
        a_, b_ = lo_a | (a[2] << 56), lo_b | (b[2] << 56)
        assert a_ == val(a) and b_ == val(b)
        return a_, b_, "exact64"
    ha = (a[w] << (34 - nb)) + (((a[w - 1] << W) | a[w - 2]) >> (nb + 22))
    hb = (b[w] << (34 - nb)) + (((b[w - 1] << W) | b[w - 2]) >> (nb + 22))
    assert max(ha, hb).bit_length() == 34
    n = W * w + nb                                                    # bit length of a | b
    assert ha == val(a) >> (n - 34) and hb == val(b) >> (n - 34) and n > 64
    return (lo_a & KMASK) | (ha << K), (lo_b & KMASK) | (hb << K), "top34"


def tail(C, v):
    """v (signed limbs, |v| < 64 p) -> (the canonical value, the estimate's remainder r, the top limb handed to the float conversion)"""
    B64 = to_limbs(64 * C.P)
    assert val(B64) == 64 * C.P
    l, c = [], 0
    for i in range(NL - 1):
        t = v[i] + B64[i] + c; l.append(t & MASK); c = t >> W
    top = v[NL - 1] + B64[NL - 1] + c
    assert 0 <= top < (1 << 24), "the top limb is not exact in float32"
    l.append(top)
    V = val(l)
    assert V == val(v) + 64 * C.P and 0 < V < 128 * C.P
    q = int(np.float32(top) * C.QINV)
    r = V - q * C.P
    assert 0 <= r < 2 * C.P, "the quotient estimate leaves [0, 2p)"
    return (r - C.P if r >= C.P else r), r, top


def inv_trace(y, curve="381", iters=None, stats=None):
    """-> (y^-1 mod p as fp_inv_bingcd computes it before its Montgomery product, the number of outer iterations after which a = 0).  iters: run that
    many outer iterations instead of ITER.  stats (a dict): collects the window forms met, max(|u|, |v|) / p at the end, r / p and the top limb."""
    C = CURVES[curve]
    assert 0 <= y < (1 << RBITS)                                       # whatever the 12 words hold; the engine passes canonical values
    a, b = to_limbs(y), to_limbs(C.P)
    u, v = to_limbs(1), to_limbs(0)
    needed = 0
    for it in range(C.ITER if iters is None else iters):
        if val(a) != 0: needed = it + 1
        a_, b_, form = window(a, b)
        assert a_ < (1 << 64) and b_ < (1 << 64)
        if stats is not None: stats.setdefault("forms", set()).add(form)
        f0, g0, f1, g1 = 1, 0, 0, 1
        for i in range(K):
            if a_ & 1:
                if a_ < b_: a_, b_ = b_, a_; f0, f1 = f1, f0; g0, g1 = g1, g0
                a_ -= b_; f0 -= f1; g0 -= g1
            a_ >>= 1; f1 *= 2; g1 *= 2
        assert max(abs(f0), abs(g0), abs(f1), abs(g1)) <= (1 << 30) and abs(f0) + abs(g0) <= (1 << 30) and abs(f1) + abs(g1) <= (1 << 30)
        na = carry_shr([f0 * a[i] + g0 * b[i] for i in range(NL)]); nb = carry_shr([f1 * a[i] + g1 * b[i] for i in range(NL)])
        if na[NL - 1] < 0: na = negate(na); f0, g0 = -f0, -g0
        if nb[NL - 1] < 0: nb = negate(nb); f1, g1 = -f1, -g1
        assert na[NL - 1] >= 0 and nb[NL - 1] >= 0
        a, b = na, nb
        nuv = []
        for ff, gg in ((f0, g0), (f1, g1)):
            col = [ff * u[i] + gg * v[i] for i in range(NL)]
            k = (((col[0] + (col[1] << W)) & 0xFFFFFFFF) * C.MINV) & KMASK
            nuv.append(carry_shr([col[i] + k * C.PL[i] for i in range(NL)]))
        u, v = nuv
        assert abs(val(u)) < 64 * C.P and abs(val(v)) < 64 * C.P
        assert (val(u) * y - val(a)) % C.P == 0 and (val(v) * y - val(b)) % C.P == 0
    if y == 0:
        assert val(a) == 0 and val(b) == C.P
        return 0, 0
    assert val(a) == 0 and val(b) == 1, "a != 0 after the outer iterations"
    x, r, top = tail(C, v)
    assert x * y % C.P == 1
    if stats is not None:
        stats["uv"] = max(stats.get("uv", 0.0), max(abs(val(u)), abs(val(v))) / C.P)
        stats["r"] = max(stats.get("r", 0.0), r / C.P); stats["top"] = max(stats.get("top", 0), top)
    return x, needed


def inv(y, curve="381"):
    return inv_trace(y, curve)[0]


def kaliski(y, curve="381"):
    """-> (k, y^-1 mod p) as fp_inv_kaliski computes them: phase 1 on 12-word u, v and 13-word r, s, the reduction of r, and 2^-k (which the device folds
    into the Montgomery product with KALISKI_FIX[k])"""
    C = CURVES[curve]
    assert 0 <= y < C.P
    if y == 0: return 0, 0                                             # no lane is live; the device overrides the result with zero
    u, v, r, s, k = C.P, y, 0, 1, 0
    while v != 0:
        assert k < 768, "more than 768 steps"
        if u % 2 == 0: u //= 2; s *= 2
        elif v % 2 == 0: v //= 2; r *= 2
        elif u > v: u = (u - v) // 2; r += s; s *= 2
        else: v = (v - u) // 2; s += r; r *= 2
        k += 1
        assert 0 <= u < (1 << 384) and 0 <= v < (1 << 384) and 0 <= r < (1 << 416) and 0 <= s < (1 << 416)
    assert u == 1 and C.BITS <= k <= 2 * C.BITS <= 768
    assert r < 2 * C.P
    w = r - C.P if r >= C.P else r
    x = C.P - w
    assert 0 < x < C.P
    return k, x * pow(2, -k, C.P) % C.P


def device_result(plain_inverse, curve="381"):
    """what both routines return for a plain inverse x: mul(x, KALISKI_FIX[0]) = x R^3 R^-1"""
    return plain_inverse * (1 << (2 * RBITS)) % CURVES[curve].P


def self_test(samples=3000):
    rnd = random.Random(2)
    for y in [1, 2, 3, P - 1, P - 2, (P + 1) // 2, 1 << 380, (1 << 381) - 1 - (1 << 300), 1 << 56, (1 << 57) + 1, 1 << 84, 5 << 100] + [rnd.randrange(1, P) for _ in range(samples)] + [rnd.randrange(1, 1 << rnd.randrange(1, 381)) for _ in range(samples)]:
        assert inv(y) * y % P == 1, hex(y)
    return ITER


if __name__ == "__main__":
    for tag, C in CURVES.items():
        rnd = random.Random(2)
        for y in [1, 2, 3, C.P - 1, C.P - 2] + [rnd.randrange(1, C.P) for _ in range(300)]:
            assert inv(y, tag) * y % C.P == 1 and kaliski(y, tag)[1] * y % C.P == 1, hex(y)
    print("ok", self_test(), hex(CURVES["381"].MINV), hex(CURVES["377"].MINV))
