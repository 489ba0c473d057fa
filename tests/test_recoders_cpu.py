"""CPU: the host scalar recoders of ripp_amd/csrc/recode.hpp (the digit strings every fold and scaling kernel walks) as pure host code.
tests/host/recoders.cpp is built stand-alone for each curve and fed S(curve) (tests/fold_edge_scalars.py: the boundaries of the GLV / GLS splits, the cut
points at bit 16 / 32 / 64 / 128, wNAF carries and empty strings) plus 2000 seeded random scalars; what it prints -- every digit string over the struct's
full capacity -- is checked with Python integers:
  value   the strings, weighted with the bases the kernels attach to them, reconstruct the scalar exactly
  shape   NAF: digits in {-1, 0, 1}, no two adjacent nonzeros; width-W wNAF: odd digits, |d| < 2^(W-1), at most one nonzero in any W consecutive positions
  bounds  len <= the maxd passed and <= capacity - 1, every entry at index >= len is zero, len > the index of the highest nonzero digit"""
import os
import random
import subprocess

import numpy as np
import pytest

import fold_edge_scalars as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")

# tag -> (strings, capacity of a string, the maxd its recoder passes, kind)
SPEC = {
    "naf_digits": (1, 260, 258, "naf"), "gls_digits": (4, 68, 66, "naf"), "glv_digits": (2, 132, 131, "naf"), "gls8_digits": (8, 36, 35, "naf"),
    "split_digits_g2": (8, 68, 35, "naf"), "split_digits_g1_glv": (8, 68, 67, "naf"), "split64_digits": (2, 132, 131, "naf"), "split_digits_g1": (8, 68, 67, "naf"),
    "wnaf4_recode": (1, 68, 66, "wnaf"), "gls16_wnaf": (16, 20, 19, "wnaf"), "gls_wnaf": (4, 68, 66, "wnaf"), "split32_wnaf": (4, 36, 35, "wnaf"),
    "fused_digits_g1": (16, 36, 35, "wnaf"), "fused_digits_g2": (48, 20, 19, "wnaf"),
}
WIDTHS = (4, 5)


def _inputs(curve):
    r, _, _ = FE.params(curve)
    rng = random.Random(0x5EED0000 + int(curve))
    return FE.scalars(curve) + [rng.randrange(r) for _ in range(1000)] + [rng.randrange(1 << 128) for _ in range(1000)]


def _run(curve, tmp):
    exe = os.path.join(tmp, "recoders_" + curve)
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-mbmi2", "-DRIPP_NO_B2S_ASM"] + (["-DRIPP_BLS12_377"] if curve == "377" else [])
                          + ["-I" + os.path.join(ROOT, "ripp_amd", "csrc"), os.path.join(ROOT, "tests", "host", "recoders.cpp"), "-o", exe])
    text = "".join("S %x\n" % s for s in _inputs(curve)) + "".join("P %x %x\n" % p for p in FE.fused_pairs(curve))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].split() == ["W"] + [str(w) for w in WIDTHS], out[0]          # tab_width(4), tab_width(FOLD_TAB_M)
    records = []
    for ln in out[1:]:
        w = ln.split()
        if w[0] in ("S", "P"):
            records.append((w[0], tuple(int(x, 16) for x in w[1:]), {}))
            continue
        rec = records[-1][2]
        assert w[0] not in rec, "printed twice: " + w[0]
        if w[0] in ("scalar_bits", "glv_split"): rec[w[0]] = w[1:]
        elif w[0] == "fits_128" or w[0].startswith("fused_digits_g2_lens"): rec[w[0]] = [int(x) for x in w[1:]]
        else:
            n, cap, _, _ = SPEC[w[0].split(".")[0]]
            assert len(w) == 2 + n and all(len(x) == cap for x in w[2:]), ("capacity", w[0])
            assert "?" not in ln, ("a digit outside [-32, 32)", w[0], records[-1][1])
            rec[w[0]] = (int(w[1]), [np.frombuffer(x.encode(), dtype=np.uint8).astype(np.int16) - ord("P") for x in w[2:]])
    return records


@pytest.fixture(scope="module", params=["381", "377"])
def run(request, tmp_path_factory):
    curve = request.param
    return curve, _run(curve, str(tmp_path_factory.mktemp("recoders")))


def _val(d):
    return sum(int(d[i]) << int(i) for i in np.nonzero(d)[0])


def _sum(strings, bases):
    assert len(strings) == len(bases)
    return sum(b * _val(d) for d, b in zip(strings, bases))


def _widths(tag):
    return [tag + ".%d" % w for w in WIDTHS]


def test_every_request_ran_every_recoder(run):
    curve, records = run
    ins, pairs = _inputs(curve), FE.fused_pairs(curve)
    assert [r[1] for r in records] == [(s,) for s in ins] + pairs
    assert len(FE.scalars(curve)) >= 30 and sum(s >= 1 << 128 for s in ins) > 1000 and sum(s < 1 << 128 for s in ins) > 1000
    for kind, req, rec in records:
        if kind == "S":
            s = req[0]
            assert rec["fits_128"] == [int(s < 1 << 128)], hex(s)                              # fits_128 IS the predicate s < 2^128
            want = {"scalar_bits", "fits_128", "glv_split", "naf_digits", "gls_digits", "glv_digits", "gls8_digits", "split_digits_g2", "split_digits_g1_glv"}
            want |= set(_widths("wnaf4_recode") + _widths("gls16_wnaf") + _widths("gls_wnaf"))
            if s < 1 << 128: want |= {"split64_digits", "split_digits_g1"} | set(_widths("split32_wnaf"))      # the 128-bit recoders: fed such scalars only
            assert set(rec) == want, hex(s)
        else:
            assert set(rec) == set(_widths("fused_digits_g1") + _widths("fused_digits_g2") + _widths("fused_digits_g2_lens")) and max(req) < 1 << 128


def test_strings_reconstruct_the_scalar(run):
    curve, records = run
    r, u, lam = FE.params(curve)
    U = [u**j for j in range(4)]
    gls16 = [(1 << (16 * b)) * U[j] for b in range(4) for j in range(4)]                       # string 4 b + j
    words = [1 << (32 * b) for b in range(4)]
    for kind, req, rec in records:
        if kind == "S":
            s = req[0]; h = hex(s)
            assert int(rec["scalar_bits"][0]) == s.bit_length() and int(rec["scalar_bits"][1], 16) == s, h
            rem, quo = (int(x, 16) for x in rec["glv_split"])
            assert rem + quo * lam == s and rem < lam and quo < 1 << 128, h
            assert _sum(rec["naf_digits"][1], [1]) == s, h
            assert _sum(rec["gls_digits"][1], U) == s, h
            g = rec["glv_digits"][1]
            assert _val(g[0]) == rem and _val(g[1]) == quo, h
            for tag in ("gls8_digits", "split_digits_g2"):
                assert _sum(rec[tag][1], U + [(1 << 32) * b for b in U]) == s, (tag, h)
            assert _sum(rec["split_digits_g1_glv"][1], [1, lam, 1 << 64, lam << 64, 0, 0, 0, 0]) == s, h
            g = rec["split_digits_g1_glv"][1]
            assert _val(g[0]) + (_val(g[2]) << 64) == rem and _val(g[1]) + (_val(g[3]) << 64) == quo and not any(x.any() for x in g[4:]), h
            for w in WIDTHS:
                assert _sum(rec["wnaf4_recode.%d" % w][1], [1]) == s & ((1 << 64) - 1), (w, h)
                assert _sum(rec["gls16_wnaf.%d" % w][1], gls16) == s, (w, h)
                assert _sum(rec["gls_wnaf.%d" % w][1], U) == s, (w, h)
                if s < 1 << 128: assert _sum(rec["split32_wnaf.%d" % w][1], words) == s, (w, h)
            if s < 1 << 128:
                assert _sum(rec["split64_digits"][1], [1, 1 << 64]) == s, h
                g = rec["split_digits_g1"][1]
                assert _sum(g, [1, 1 << 64, 0, 0, 0, 0, 0, 0]) == s and not any(x.any() for x in g[2:]), h
        else:
            x0, x1 = req; prod = x0 * x1 % r; h = (hex(x0), hex(x1))
            for w in WIDTHS:
                g = rec["fused_digits_g1.%d" % w][1]                                            # string 4 t + b = 32-bit word b of x0 | k1 | k2 | x1
                v = [_sum(g[4 * t:4 * t + 4], words) for t in range(4)]
                assert v[0] == x0 and v[3] == x1 and v[1] + v[2] * lam == prod and v[1] < lam and v[2] < 1 << 128, (w, h)
                g = rec["fused_digits_g2.%d" % w][1]                                            # sets x0 x1 | x0 | x1
                assert [_sum(g[16 * t:16 * t + 16], gls16) for t in range(3)] == [prod, x0, x1], (w, h)


def test_digit_shapes(run):
    _, records = run
    for _, req, rec in records:
        for tag, val in rec.items():
            name, _, w = tag.partition(".")
            if name not in SPEC: continue
            for d in val[1]:
                nz = d != 0
                if SPEC[name][3] == "naf":
                    assert np.abs(d).max() <= 1 and not (nz[1:] & nz[:-1]).any(), (tag, req)
                else:
                    W = int(w)
                    assert (d[nz] & 1).all() and np.abs(d).max() < 1 << (W - 1), (tag, req)
                    assert np.convolve(nz.astype(np.int32), np.ones(W, dtype=np.int32)).max() <= 1, (tag, req)      # every window of W consecutive positions


def test_lengths_and_padding(run):
    _, records = run
    for _, req, rec in records:
        for tag, val in rec.items():
            name, _, w = tag.partition(".")
            if name not in SPEC: continue
            _, cap, maxd, _ = SPEC[name]
            ln, strings = val
            assert 0 <= ln <= maxd and ln <= cap - 1, (tag, req, ln)
            tops = [int(np.nonzero(d)[0][-1]) if d.any() else -1 for d in strings]
            assert all(not d[ln:].any() for d in strings) and ln > max(tops), (tag, req, ln)
            if name == "fused_digits_g2":                                                       # Wnaf16x3: each set has its own len as well
                lens = rec["fused_digits_g2_lens." + w]
                assert ln == max(lens), (tag, req)
                for t in range(3):
                    assert 0 <= lens[t] <= maxd and lens[t] > max(tops[16 * t:16 * t + 16]) and all(not d[lens[t]:].any() for d in strings[16 * t:16 * t + 16]), (tag, req, t)
