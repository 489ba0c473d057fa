"""CPU: the native TIPA provers / verifiers for multiexponentiation products with a committed scalar vector and for scalar products (include/ripp_hip.h:
ripp_tipa_mexp_prove / _verify, ripp_tipa_scalar_prove / _verify) as far as they can be checked without a device -- both libraries export the four names,
argument errors come before the device is looked for, the calls refuse with RIPP_ERR_DEVICE when there is none and allocate nothing -- and the CPU model
tests/model/tipa_generic_oracle.py: pinned to the C oracle's TIPP prover member for member, and held to every input set tests/test_gpu_tipa_generic.py uses."""
import ctypes
import os
import re

import numpy as np
import pytest

import tipa_generic_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, POW2, DEVICE, ARG = 0, 2, 3, 4
NAMES = ("ripp_tipa_mexp_prove", "ripp_tipa_mexp_verify", "ripp_tipa_scalar_prove", "ripp_tipa_scalar_verify")


@pytest.fixture(scope="module")
def libs():
    from ripp_amd._lib import lib
    import ripp_amd.bls12_377 as R7
    return lib(), R7.lib()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sz(v):
    return ctypes.c_size_t(v)


def _args(n=4):
    """well-formed buffers for n <= 8.  -> (keep-alive, {name: argument list}); the size argument sits at index 5 of a prover's list and 7 of a verifier's.
    The SRS handle is opaque: a zero-filled block reads as an SRS of 0 powers, and its size check comes before anything else looks at it."""
    fr = np.zeros((8, 4), dtype=np.uint64); g1a = np.zeros((8, 12), dtype=np.uint64); g2a = np.zeros((8, 24), dtype=np.uint64)
    g1j = np.zeros((8, 18), dtype=np.uint64); g2j = np.zeros((8, 36), dtype=np.uint64); gt = np.zeros((8, 72), dtype=np.uint64)
    srs = np.zeros(64, dtype=np.uint64); vsrs = np.zeros(2 * 18 + 2 * 36, dtype=np.uint64)
    keep = (fr, g1a, g2a, g1j, g2j, gt, srs, vsrs)
    a = {
        #                        srs      m_a      m_b     ck_a     ck_b     n       r_shift com_gt  com_ped  com_ip   tr      base_a   base_b  f_ck_a   f_ck_b   open_a   open_b   kzg_c
        "ripp_tipa_mexp_prove": [_p(srs), _p(g1j), _p(fr), _p(g2a), _p(g1a), _sz(n), _p(fr), _p(gt), _p(g1j), _p(g1j), _p(fr), _p(g1j), _p(fr), _p(g2j), _p(g1j), _p(g2j), _p(g1j), _p(fr), None],
        #                          srs      m_a     m_b     ck_a     ck_b     n       r_shift com_g2   com_g1   com_fr  tr      base_a  base_b  f_ck_a   f_ck_b   open_a   open_b   kzg_c
        "ripp_tipa_scalar_prove": [_p(srs), _p(fr), _p(fr), _p(g2a), _p(g1a), _sz(n), _p(fr), _p(g2j), _p(g1j), _p(fr), _p(fr), _p(fr), _p(fr), _p(g2j), _p(g1j), _p(g2j), _p(g1j), _p(fr), None],
        #                         v_srs     com_a   com_b    com_t    com_gt  com_ped  com_ip   rounds  base_a   base_b  f_ck_a   f_ck_b   open_a   open_b   r_shift accept
        "ripp_tipa_mexp_verify": [_p(vsrs), _p(gt), _p(g1j), _p(g1j), _p(gt), _p(g1j), _p(g1j), _sz(2), _p(g1j), _p(fr), _p(g2j), _p(g1j), _p(g2j), _p(g1j), _p(fr), None],
        #                           v_srs     com_a    com_b    com_t   com_g2   com_g1   com_fr  rounds  base_a  base_b  f_ck_a   f_ck_b   open_a   open_b   r_shift accept
        "ripp_tipa_scalar_verify": [_p(vsrs), _p(g2j), _p(g1j), _p(fr), _p(g2j), _p(g1j), _p(fr), _sz(2), _p(fr), _p(fr), _p(g2j), _p(g1j), _p(g2j), _p(g1j), _p(fr), None],
    }
    return keep, a


def test_header_declares_and_both_libraries_export_the_four_names(libs):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ripp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ripp_[a-z0-9_]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ripp_hip.h"
        assert hasattr(libs[0], name), f"{name} is not exported by libripp_hip.so"
        assert hasattr(libs[1], name), f"{name} is not exported by libripp_hip_377.so"
    assert "#define RIPP_ABI_VERSION 7" in src
    assert libs[0].ripp_abi_version() == 7 and libs[1].ripp_abi_version() == 7


@pytest.mark.parametrize("which", [0, 1])
def test_null_in_each_pointer_position_is_an_argument_error(libs, which):
    L = libs[which]
    keep, args = _args()
    for name in NAMES:
        a = args[name]
        acc = ctypes.c_int32(-1)
        size_at = 5 if name.endswith("prove") else 7
        if name.endswith("verify"): a = a[:-1] + [ctypes.byref(acc)]
        tested = 0
        for i in range(len(a)):
            if i == size_at or (name.endswith("prove") and i == len(a) - 1): continue            # the size; stats may be NULL
            b = list(a); b[i] = None
            assert getattr(L, name)(*b) == ARG, f"{name}, pointer {i}"
            tested += 1
        assert tested == (17 if name.endswith("prove") else 15)
        assert acc.value == -1
    assert L.ripp_device_bytes() == 0 or L.ripp_device_count() > 0


@pytest.mark.parametrize("which", [0, 1])
def test_lengths_that_are_no_power_of_two_from_2_on(libs, which):
    L = libs[which]
    for n in (0, 1, 3, 6):
        keep, args = _args(n)
        assert L.ripp_tipa_mexp_prove(*args["ripp_tipa_mexp_prove"]) == POW2, n
        assert L.ripp_tipa_scalar_prove(*args["ripp_tipa_scalar_prove"]) == POW2, n
    assert L.ripp_device_bytes() == 0 or L.ripp_device_count() > 0


@pytest.mark.parametrize("which", [0, 1])
def test_srs_size_mismatch_is_an_argument_error(libs, which):
    L = libs[which]
    for n in (2, 4, 8):
        keep, args = _args(n)                                                                     # the handle holds 0 powers, never 2n - 1
        for name in ("ripp_tipa_mexp_prove", "ripp_tipa_scalar_prove"):
            assert getattr(L, name)(*args[name]) == ARG, (name, n)
            assert f"need 2n-1 = {2 * n - 1}" in L.ripp_last_error().decode()
    assert L.ripp_device_bytes() == 0 or L.ripp_device_count() > 0


def test_no_device_means_status_3_and_no_memory(libs):
    if libs[0].ripp_device_count() > 0:
        pytest.skip("a HIP device is present; the refusal path is exercised on the CPU-only builder")
    import ripp_amd as R
    import ripp_amd.bls12_377 as R7
    for L in libs:
        keep, args = _args(4)
        keep[6][6] = 7                                                                            # `num` of the zero-filled SRS block (two buffers of three words, then the count): 2n - 1
        acc = ctypes.c_int32(-1)
        for name in NAMES:
            a = args[name]
            if name.endswith("verify"): a = a[:-1] + [ctypes.byref(acc)]
            assert getattr(L, name)(*a) == DEVICE, name
        assert acc.value == -1
        assert L.ripp_device_bytes() == 0
    for mod in (R, R7):
        assert hasattr(mod, "TIPA_MEXP") and hasattr(mod, "TIPA_SCALAR")
        for cls in (mod.TIPA_MEXP, mod.TIPA_SCALAR):
            for fn in ("prove", "prove_with_srs_shift", "verify", "verify_with_srs_shift"):
                assert callable(getattr(cls, fn))
    assert libs[0].ripp_device_bytes() == 0 and libs[1].ripp_device_bytes() == 0


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("shift", [1, I.SHIFT])
def test_model_equals_the_c_oracle_on_the_pairing_instantiation(orc, n, shift):
    """TIPA<PairingInnerProduct, AFGHO-G1, AFGHO-G2, Identity<GT>>: the model's proof equals orclib.tipa_tipp_prove's member for member and
    orclib.tipa_tipp_verify accepts it -- this pins the model's KZG half (challenge, key polynomial, quotient, openings) to the C oracle."""
    import gipa_generic_oracle as G
    import helpers as h
    import tipa_generic_oracle as T
    s = I.srs(orc, n); ck_a, ck_b = I.keys(s)
    m_a, m_b = orc.blind_g1(orc.gen_g1(11, n), 1), orc.blind_g2(orc.gen_g2(22, n), 2)
    if shift != 1:
        ck_a, m_a = I.shift_keys(orc, ck_a, shift), I.shift_points(orc, m_a, shift)
    rs = orc.fr_array([shift])[0]
    rc, ref = orc.tipa_tipp_prove(s[0], s[1], m_a, m_b, ck_a, ck_b, rs); assert rc == 0
    got = T.prove(I.INST_PAIR, s, m_a, m_b, ck_a, ck_b, shift)
    rounds = n.bit_length() - 1
    assert len(got["steps"]) == rounds
    for k in range(rounds):
        for side in range(2):
            for j in range(3):
                assert np.array_equal(got["steps"][k][side][j], ref["steps"][6 * k + 3 * side + j]), (k, side, j)
    assert orc.fr_array(got["tr"]).tobytes() == ref["tr"].tobytes()
    assert G.same("G1", got["base"][0], ref["base_a"]) and G.same("G2", got["base"][1], ref["base_b"])
    assert G.same("G2", got["final_ck"][0], ref["final_ck_a"]) and G.same("G1", got["final_ck"][1], ref["final_ck_b"])
    assert G.same("G2", got["opening_a"], ref["opening_a"]) and G.same("G1", got["opening_b"], ref["opening_b"])
    assert got["kzg_c"] == orc.limbs_to_fr(ref["kzg_c"])
    com = T.commit(I.INST_PAIR, m_a, m_b, ck_a, ck_b)
    as_oracle = dict(steps=np.stack([x for st in got["steps"] for side in st for x in side]), base_a=got["base"][0], base_b=got["base"][1],
                     final_ck_a=got["final_ck"][0], final_ck_b=got["final_ck"][1], opening_a=got["opening_a"], opening_b=got["opening_b"])
    assert orc.tipa_tipp_verify(*h.verifier_srs(s), com, as_oracle, rs) == 1
    assert T.verify(I.INST_PAIR, h.verifier_srs(s), com, got, shift)
    if shift != 1:
        assert not T.verify(I.INST_PAIR, h.verifier_srs(s), com, got, 1)


def _model_holds(inst, case, shift=1):
    import gipa_generic_oracle as G
    import tipa_generic_oracle as T
    v = I.verifier_srs(case)
    assert T.verify(inst, v, case["com"], case["model"], shift)
    t = inst[3]
    wrong = [case["com"][0], case["com"][1], G.plus(t, case["com"][2], case["com"][2])]
    assert not T.verify(inst, v, wrong, case["model"], shift)


@pytest.mark.parametrize("n", I.SIZES_MEXP)
def test_model_proves_the_multiexponentiation_statements(orc, n):
    _model_holds(I.INST_MEXP, I.mexp_case(n))


@pytest.mark.parametrize("n", I.SIZES_SCAL)
def test_model_proves_the_scalar_statements(orc, n):
    _model_holds(I.INST_SCAL, I.scalar_case(n))


def test_model_proves_the_shifted_statements(orc):
    import tipa_generic_oracle as T
    for inst, case in ((I.INST_MEXP, I.mexp_case(8, I.SHIFT)), (I.INST_SCAL, I.scalar_case(8, I.SHIFT))):
        _model_holds(inst, case, I.SHIFT)
        assert not T.verify(inst, I.verifier_srs(case), case["com"], case["model"], 1)


@pytest.mark.parametrize("trapdoors", sorted(I.TRAPDOORS))
@pytest.mark.parametrize("which", [0, 1])
def test_model_proves_the_scalar_edge_sets(orc, trapdoors, which):
    """Precondition of test_gpu_tipa_generic.py::test_scalar_edges: the edge values are what the docstring of scalar_edges says, every key is +-generator, and
    the model proves the statement."""
    ma, mb = I.scalar_edges(orc, which)
    R, X = orc.R, I.X_ABS
    assert len(ma) == len(mb) == 8 and X ** 4 > R > X ** 3 and X.bit_length() == 64
    both = set(ma) | set(mb)
    if which == 0:
        assert {0, 1, R - 1, X - 1, X, X + 1, X * X, X ** 3} == set(ma) and {I.LAMBDA, I.LAMBDA + 1, (1 << 128) - 1, 1 << 128} <= set(mb)
    else:
        assert {(1 << 64) - 1, 1 << 64} <= set(ma) and {0, 1, R - 1, X - 1, X, X + 1, X * X, X ** 3} == set(mb)
        assert (X - 1) * (1 + X + X * X) in both                                              # digits (|x| - 1, |x| - 1, |x| - 1, 0)
    case = I.scalar_edge_case(trapdoors, which)
    gen1, gen2 = orc.g1_generator(), orc.g2_generator()
    for k in case["ck_a"]: assert np.array_equal(orc.g2_to_affine(k), gen2)
    for k in case["ck_b"]: assert np.array_equal(orc.g1_to_affine(k), gen1)
    neg1 = orc.g1_mul_a(gen1, orc.fr_array([R - 1])[0])
    odd = orc.g1_to_affine(case["srs"][0][1])
    assert np.array_equal(odd, gen1 if trapdoors == "one" else neg1)                           # the odd powers of the SRS: generator or its negative
    _model_holds(I.INST_SCAL, case)
