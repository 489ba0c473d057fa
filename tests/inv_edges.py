"""The inputs the device inversion (ripp_amd/csrc/bls12_381/fp_inv.hpp) is tested on, per curve ("381" / "377"), shared by tests/test_inv_model_cpu.py
(the model of tools/inv_model.py, all assertions on) and tests/test_gpu_inv_edges.py (the device code through tests/device/inv_edges.hip).

Every value is a canonical integer 0 <= y < p: the raw 12 words handed to fp_inv_bingcd / fp_inv_kaliski, whatever they stand for."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import inv_model as IM  # noqa: E402

TAGS = ["381", "377"]
N_RANDOM = 1000
WINDOW_SWITCHES = (55, 56, 57, 63, 64, 65, 83, 84, 85)          # 2^k - 1: around the exact <= 56 bits / exact <= 64 bits / top 34 + low 30 bits switches


def _unique(seq):
    seen, out = set(), []
    for v in seq:
        if v not in seen:
            seen.add(v); out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def structured(tag):
    C = IM.CURVES[tag]
    p = C.P
    vals = [0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2, p // 3, 2 * p // 3]
    for k in range(C.BITS):
        for d in (-1, 0, 1):
            vals += [v for v in ((1 << k) + d, p - (1 << k) + d) if 0 < v < p]
    vals += [(1 << k) - 1 for k in WINDOW_SWITCHES]
    for s in list(range(1, 20)) + [p - 1, p - 2]:                 # the Montgomery images of small values in both radices (2^384: fp.hpp, 2^392: fq28.hpp)
        for e in (384, 392):
            vals += [s * pow(2, e, p) % p, s * pow(2, -e, p) % p]
    assert all(0 <= v < p for v in vals)
    return tuple(_unique(vals))


@functools.lru_cache(maxsize=None)
def randoms(tag):
    rnd = random.Random(0x1E5 + int(tag))
    return tuple(rnd.randrange(1, IM.CURVES[tag].P) for _ in range(N_RANDOM))


FULL_RUN_FROM = {"381": 370, "377": 374}


def full_run(tag):
    """the values of the list that keep fp_inv_bingcd busy through all of its outer iterations: 2^k and p - 2^k for the largest k (tests/test_inv_model_cpu.py
    checks that these, and no others of the list, need all ITER iterations of the model)"""
    C = IM.CURVES[tag]
    return tuple(v for k in range(FULL_RUN_FROM[tag], C.BITS) for v in (1 << k, C.P - (1 << k)))


def values(tag):
    """the whole list: structured values, then the seeded random ones"""
    return structured(tag) + randoms(tag)


@functools.lru_cache(maxsize=None)
def kaliski_steps(tag):
    """k of fp_inv_kaliski for every value of the list (0 for y = 0)"""
    return tuple(IM.kaliski(y, tag)[0] for y in values(tag))


@functools.lru_cache(maxsize=None)
def traces(tag):
    """(plain inverse, outer iterations needed) of the fp_inv_bingcd model for every value of the list, all model assertions on; plus the statistics"""
    stats = {}
    return tuple(IM.inv_trace(y, tag, stats=stats) for y in values(tag)), stats


def expected(tag, y):
    """what every form of the device inversion must return for the raw input y: y^-1 2^768 mod p (0 for 0)"""
    p = IM.CURVES[tag].P
    return 0 if y == 0 else pow(y, -1, p) * (1 << 768) % p
