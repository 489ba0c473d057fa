"""The scalars at the edges of the fold / scaling kernels' scalar splits, per curve (shared by tests/test_recoders_cpu.py, test_gpu_fold_edges.py and
test_gpu_scale_edges.py).  u = |x| and the GLV eigenvalue lambda are PARSED from the build's own parameter headers (RIPP_X_ABS_LIMBS, RIPP_GLV_LAMBDA in
ripp_amd/csrc/bls12_381/params.hpp and bls12_377/params.hpp), so the list sits where the engine's recoders (ripp_amd/csrc/recode.hpp) really cut."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADERS = {"381": os.path.join(ROOT, "ripp_amd", "csrc", "bls12_381", "params.hpp"), "377": os.path.join(ROOT, "ripp_amd", "csrc", "bls12_377", "params.hpp")}
_cache = {}


def _limbs(text, name):
    """the value of `#define NAME {0x..u, 0x..u, ...}`: little-endian 32-bit limbs"""
    m = re.search(r"^#define\s+" + name + r"\s+\{([^}]*)\}\s*$", text, re.M)
    assert m, name + " not found"
    words = [int(w.strip().rstrip("uU"), 16) for w in m.group(1).split(",")]
    assert words and all(0 <= w < 1 << 32 for w in words)
    return sum(w << (32 * i) for i, w in enumerate(words))


def params(curve):
    """(r, u, lam) of curve "381" / "377", with the relations the splits rest on"""
    if curve not in _cache:
        with open(_HEADERS[curve]) as f:
            text = f.read()
        r, u, lam = _limbs(text, "RIPP_FR_R"), _limbs(text, "RIPP_X_ABS_LIMBS"), _limbs(text, "RIPP_GLV_LAMBDA")
        assert r == u**4 - u**2 + 1, "r != u^4 - u^2 + 1"
        assert (lam * lam + lam + 1) % r == 0, "lambda is no primitive cube root of unity mod r"
        assert 1 << 63 <= u < 1 << 64 and lam < 1 << 128 and (r - 1) // lam < 1 << 128
        _cache[curve] = (r, u, lam)
    return _cache[curve]


WNAF_C = 0x7FFFFFFF_80000000          # the 128-bit challenge whose full-width inverse closes the list (GIPA's G2 folds take c^-1)


def scalars(curve):
    """S(curve): canonical integers below r, duplicates dropped, order stable"""
    r, u, lam = params(curve)
    s = [0, 1, 2, 3, r - 1, r - 2]                                                            # small values and the group order
    s += [lam - 1, lam, lam + 1, 2 * lam, r - lam, lam * lam % r]                             # GLV boundaries
    s += [(lam - 1) * lam + (lam - 1), 1 + lam]                                               # both halves at once
    s += [(r - 1) // lam * lam]                                                               # the largest quotient
    s += [u - 1, u, u + 1, u**2 - 1, u**2, u**2 + 1, u**3 - 1, u**3, u**3 + u - 1, (u - 1) * (1 + u + u**2 + u**3)]      # GLS boundaries
    s += [2**32 - 1, 2**32, 2**64 - 1, 2**64, 2**128 - 1, 2**128, 2**254, 2**254 + 2**127]    # cut points of the split forms
    # wNAF carries and empty strings in 128-bit challenges
    s += [0xFFFFFFFF_00000000_FFFFFFFF, 0xFFFFFFFF_FFFFFFFF_FFFFFFFF_FFFFFFFF, WNAF_C, 0xFFFF0000_FFFF0000_FFFF0000_FFFF]
    ks = [0x7FFF, 0x8000, 0xFFFF]
    s += [sum(((ks[(j + t) % 3]) << 16) * u**j for j in range(4)) for t in range(3)]          # 16-bit pieces of every base-u digit: each k at each digit
    s += [(u - 1) * u + (u >> 1) * u**3]                                                      # every second base-u digit zero
    s += [pow(WNAF_C, -1, r)]                                                                 # a 128-bit c (above) with its full-width inverse
    out = []
    for v in s:
        v %= r
        if v not in out:
            out.append(v)
    return out


def fused_pairs(curve):
    """(x0, x1), both below 2^128, for the fused round-0/1 recoders: the 128-bit members of S against each other"""
    small = [v for v in scalars(curve) if v < 1 << 128]
    edge = [1, 2**32 - 1, 2**64, 2**128 - 1, 0xFFFFFFFF_00000000_FFFFFFFF, WNAF_C]
    assert all(v in small for v in edge)
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(small[i], small[-1 - i]) for i in range(len(small))]
    return pairs
