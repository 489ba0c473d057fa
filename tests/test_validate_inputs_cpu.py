"""CPU: the inputs of the validation tests (tests/validate_inputs.py), the host side of the feature, and the six entry points without a device.

  inputs      every class carries the flag the DEFINITION gives it (range, curve equation, [r]P = O); the small-order points have the stated orders,
              the torsion points are killed by the cofactor, the facts the exactness argument of DESIGN.md section 3d rests on hold as integers
  host code   tests/host/validate.cpp, stand-alone per curve and once more under AddressSanitizer + UBSan: val_complete (the check the kernels redo their
              exceptional lanes with, and the criterion their fast chains evaluate) agrees with the definition on every input; wire.hpp's parse_g1 / parse_g2
              give the documented reason for every tampered image, and the single-element readers built on them accept exactly the valid ones
  C ABI       both libraries export the calls; argument errors are RIPP_ERR_ARG and n = 0 is RIPP_OK before any device is looked for; n = 1 needs a device"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import validate_inputs as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
SYMBOLS = ("ripp_validate_g1a", "ripp_validate_g2a", "ripp_vec_validate", "ripp_de_g1_vec", "ripp_de_g2_vec", "ripp_de_groth16_proofs")
EXPECT = {"subgroup": V.OK, "infinity": V.OK, "outside": V.SUBGROUP, "torsion": V.SUBGROUP, "mixed": V.SUBGROUP, "small": V.SUBGROUP, "offcurve": V.CURVE, "unreduced": V.RANGE}
CASES = [(t, g) for t in V.TAGS for g in (1, 2)]


def library(tag):
    if tag == "381":
        from ripp_amd._lib import lib
        return lib()
    import ripp_amd.bls12_377 as R7
    return R7.lib()


@pytest.mark.parametrize("tag,g", CASES)
def test_every_class_carries_the_flag_of_the_definition(tag, g):
    C, cls = V.curve(tag), V.classes(tag, g)
    assert set(cls) == set(EXPECT)
    for name, pts in cls.items():
        assert len(pts) <= 32 and (pts or (name == "small" and (tag, g) == ("377", 2))), name
        assert [f for _, f in pts] == [EXPECT[name]] * len(pts), name
    canon = lambda raw: [v * pow(V.RP, -1, C.P) % C.P for v in raw]
    point = lambda raw: (lambda c: (c[0], c[1]) if g == 1 else ((c[0], c[1]), (c[2], c[3])))(canon(raw))
    for raw, _ in cls["torsion"]:
        assert C.mul(g, C.h[g], point(raw)) is None and C.mul(g, C.R, point(raw)) is not None
    for raw, _ in cls["outside"]:
        assert C.mul(g, C.h[g] * C.R, point(raw)) is None                      # the cofactor formulas: h r is the group order
    zero = C.F[g].zero
    n3 = n2 = 0
    for raw, _ in cls["small"]:
        pt = point(raw)
        if pt[0] == zero: assert C.mul(g, 3, pt) is None; n3 += 1
        if pt[1] == zero: assert C.mul(g, 2, pt) is None; n2 += 1
    assert (n3, n2) == (V.SMALL_ORDER[(tag, g)]["x=0"], V.SMALL_ORDER[(tag, g)]["y=0"])
    if g == 1:
        want = {"381": [(0, 2), (0, C.P - 2)], "377": [(0, 1), (0, C.P - 1), (C.P - 1, 0)]}[tag]
        assert all(p in [point(raw) for raw, _ in cls["small"]] for p in want)


@pytest.mark.parametrize("tag", V.TAGS)
def test_the_integer_facts_behind_the_exactness_argument(tag):
    C = V.curve(tag); x = C.X; u = abs(x); lam = u * u - 1
    assert lam * lam + lam + 1 == C.R                                          # G1: phi^2 + phi + 1 = 0 and phi(P) = [lambda]P give [r]P = O
    assert C.P - x == C.R * C.h[1]                                             # G2: psi^2 - t psi + p = 0, t = x + 1 and psi(P) = [x]P give [p - x]P = O
    assert math.gcd(C.h[2], C.h[1]) == 1 and C.h[2] % C.R != 0 and C.h[1] % C.R != 0      # ... and the order of P divides h2 r: it divides r


def _compile(tmp, tag, flags):
    exe = os.path.join(tmp, "validate_" + tag + ("_san" if flags else ""))
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-mbmi2", "-DRIPP_NO_B2S_ASM", "-Wall", "-Werror"] + flags + (["-DRIPP_BLS12_377"] if tag == "377" else [])
                          + ["-I" + os.path.join(ROOT, "ripp_amd", "csrc"), os.path.join(ROOT, "tests", "host", "validate.cpp"), "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [tuple(int(w) for w in ln.split()) for ln in out]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
@pytest.mark.parametrize("tag", V.TAGS)
def test_host_check_and_parse_split_against_the_definition(tmp_path, tag, sanitize):
    """the stand-alone program itself is the (sanitized) binary: nothing is loaded into python, no device"""
    exe = _compile(str(tmp_path), tag, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
    L = library(tag)
    for g in (1, 2):
        m = V.mixed(tag, g)
        got = _run(exe, ["%d %s" % (g, " ".join("%x" % v for v in raw)) for raw, _ in m])
        assert got == [(f, f) for _, f in m], (tag, g)
        imgs = V.tampered_images(tag, g, L)
        got = _run(exe, ["W %d %d %s" % (g, c, bytes(img).hex()) for c, img, _, _ in imgs])
        assert got == [(p, a) for _, _, p, a in imgs], (tag, g)


@pytest.mark.parametrize("tag", V.TAGS)
def test_symbols_argument_errors_and_the_empty_call_need_no_device(tag):
    L = library(tag)
    assert all(hasattr(L, s) for s in SYMBOLS + ("ripp_validate_set_chunk",))
    sz = ctypes.c_size_t
    nb, fb = sz(7), sz(7)
    p1, p2, img = np.zeros((1, 12), dtype=np.uint64), np.zeros((1, 24), dtype=np.uint64), np.zeros(384, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    R = ctypes.byref
    ARG, DEVICE = 4, 3
    for fn, pts in ((L.ripp_validate_g1a, p1), (L.ripp_validate_g2a, p2)):
        assert fn(None, sz(1), None, R(nb), R(fb)) == ARG and fn(P(pts), sz(1), None, None, R(fb)) == ARG and fn(P(pts), sz(1), None, R(nb), None) == ARG
        assert fn(P(pts), sz(0), None, R(nb), R(fb)) == 0 and (nb.value, fb.value) == (0, 0)
    assert L.ripp_vec_validate(None, None, R(nb), R(fb)) == ARG
    for fn, pts, sizes in ((L.ripp_de_g1_vec, p1, (96, 48)), (L.ripp_de_g2_vec, p2, (192, 96))):
        for c in (0, 1):
            assert fn(P(img), sz(sizes[c] - 1), sz(1), c, P(pts), None, R(nb), R(fb)) == ARG            # stride below the image size
            assert fn(None, sz(sizes[c]), sz(1), c, P(pts), None, R(nb), R(fb)) == ARG and fn(P(img), sz(sizes[c]), sz(1), c, None, None, R(nb), R(fb)) == ARG
            assert fn(P(img), sz(sizes[c]), sz(1), c, P(pts), None, None, R(fb)) == ARG and fn(P(img), sz(sizes[c]), sz(1), c, P(pts), None, R(nb), None) == ARG
            nb.value = fb.value = 7
            assert fn(P(img), sz(sizes[c]), sz(0), c, P(pts), None, R(nb), R(fb)) == 0 and (nb.value, fb.value) == (0, 0)
    g = L.ripp_de_groth16_proofs
    for c, size in ((0, 384), (1, 192)):
        assert g(P(img), sz(size - 1), sz(1), c, P(p1), P(p2), P(p1), None, R(nb), R(fb)) == ARG
        assert g(None, sz(size), sz(1), c, P(p1), P(p2), P(p1), None, R(nb), R(fb)) == ARG and g(P(img), sz(size), sz(1), c, None, P(p2), P(p1), None, R(nb), R(fb)) == ARG
        assert g(P(img), sz(size), sz(1), c, P(p1), None, P(p1), None, R(nb), R(fb)) == ARG and g(P(img), sz(size), sz(1), c, P(p1), P(p2), None, None, R(nb), R(fb)) == ARG
        assert g(P(img), sz(size), sz(1), c, P(p1), P(p2), P(p1), None, None, R(fb)) == ARG and g(P(img), sz(size), sz(1), c, P(p1), P(p2), P(p1), None, R(nb), None) == ARG
        nb.value = fb.value = 7
        assert g(P(img), sz(size), sz(0), c, P(p1), P(p2), P(p1), None, R(nb), R(fb)) == 0 and (nb.value, fb.value) == (0, 0)
    # one point needs the device: no CPU fallback
    have = L.ripp_device_count() > 0
    for fn, pts in ((L.ripp_validate_g1a, p1), (L.ripp_validate_g2a, p2)):
        rc = fn(P(pts), sz(1), None, R(nb), R(fb))
        assert rc == (0 if have else DEVICE)
    assert L.ripp_de_g1_vec(P(img), sz(96), sz(1), 0, P(p1), None, R(nb), R(fb)) == (0 if have else DEVICE)
