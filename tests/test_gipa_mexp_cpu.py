"""CPU: the fused GIPA prover / verifier for multiexponentiation products with a committed scalar vector (include/ripp_hip.h: ripp_gipa_mexp_prove,
ripp_gipa_mexp_verify; gipa_mexp_api.inc) as far as it can be checked without a device: both libraries export the two names, argument errors come before the
device is looked for, both calls refuse with RIPP_ERR_DEVICE when there is none and allocate nothing -- and the CPU model accepts the edge-case inputs
that tests/test_gpu_gipa_mexp.py compares the device with."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, POW2, DEVICE, ARG = 0, 2, 3, 4


@pytest.fixture(scope="module")
def libs():
    from ripp_amd._lib import lib
    import ripp_amd.bls12_377 as R7
    return lib(), R7.lib()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sz(v):
    return ctypes.c_size_t(v)


def _args():
    """well-formed buffers for n <= 8: (prove arguments without n and stats, verify arguments without n and accept)"""
    fr = np.zeros((8, 4), dtype=np.uint64); g1a = np.zeros((8, 12), dtype=np.uint64); g2a = np.zeros((8, 24), dtype=np.uint64)
    g1j = np.zeros((8, 18), dtype=np.uint64); g2j = np.zeros((8, 36), dtype=np.uint64); gt = np.zeros((8, 72), dtype=np.uint64)
    keep = (fr, g1a, g2a, g1j, g2j, gt)
    #         m_a      m_b     ck_a     ck_b     com_gt  com_ped  com_ip   transcript base_a  base_b  ck_base_a ck_base_b
    prove = [_p(g1j), _p(fr), _p(g2a), _p(g1a), _p(gt), _p(g1j), _p(g1j), _p(fr), _p(g1j), _p(fr), _p(g2j), _p(g1j)]
    #          ck_a     ck_b     com_a   com_b    com_t    com_gt  com_ped  com_ip   base_a   base_b
    verify = [_p(g2a), _p(g1a), _p(gt), _p(g1j), _p(g1j), _p(gt), _p(g1j), _p(g1j), _p(g1j), _p(fr)]
    return keep, prove, verify


def _prove(L, a, n, stats=None):
    return L.ripp_gipa_mexp_prove(*a[:4], _sz(n), *a[4:], stats)


def _verify(L, a, n, acc):
    return L.ripp_gipa_mexp_verify(*a[:2], _sz(n), *a[2:], None if acc is None else ctypes.byref(acc))


def test_header_declares_and_both_libraries_export_the_two_names(libs):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ripp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ripp_[a-z0-9_]+)\s*\(", src))
    for name in ("ripp_gipa_mexp_prove", "ripp_gipa_mexp_verify"):
        assert name in declared, f"{name} is not declared in include/ripp_hip.h"
        assert hasattr(libs[0], name), f"{name} is not exported by libripp_hip.so"
        assert hasattr(libs[1], name), f"{name} is not exported by libripp_hip_377.so"
    assert "#define RIPP_ABI_VERSION 7" in src
    assert libs[0].ripp_abi_version() == 7 and libs[1].ripp_abi_version() == 7


@pytest.mark.parametrize("which", [0, 1])
def test_null_in_each_pointer_position_is_an_argument_error(libs, which):
    L = libs[which]
    keep, prove, verify = _args()
    assert len(prove) == 12 and len(verify) == 10
    for i in range(len(prove)):
        a = list(prove); a[i] = None
        assert _prove(L, a, 4) == ARG, f"ripp_gipa_mexp_prove, pointer {i}"
    acc = ctypes.c_int32(-1)
    for i in range(len(verify)):
        a = list(verify); a[i] = None
        assert _verify(L, a, 4, acc) == ARG, f"ripp_gipa_mexp_verify, pointer {i}"
    assert _verify(L, verify, 4, None) == ARG
    assert acc.value == -1
    assert L.ripp_device_bytes() == 0 or L.ripp_device_count() > 0


@pytest.mark.parametrize("which", [0, 1])
def test_lengths_that_are_no_power_of_two_from_2_on(libs, which):
    L = libs[which]
    keep, prove, verify = _args()
    acc = ctypes.c_int32(-1)
    for n in (0, 1, 3, 6):
        assert _prove(L, prove, n) == POW2, n
        assert _verify(L, verify, n, acc) == POW2, n
    assert acc.value == -1
    assert L.ripp_device_bytes() == 0 or L.ripp_device_count() > 0


def test_no_device_means_status_3_and_no_memory(libs):
    if libs[0].ripp_device_count() > 0:
        pytest.skip("a HIP device is present; the refusal path is exercised on the CPU-only builder")
    import ripp_amd as R
    import ripp_amd.bls12_377 as R7
    keep, prove, verify = _args()
    for L in libs:
        acc = ctypes.c_int32(-1)
        assert _prove(L, prove, 4) == DEVICE
        assert _verify(L, verify, 4, acc) == DEVICE
        assert acc.value == -1
        assert L.ripp_device_bytes() == 0
    fr, g1a, g2a, g1j = keep[0], keep[1], keep[2], keep[3]
    for mod in (R, R7):
        with pytest.raises(mod.DeviceError):
            mod.GIPA_MEXP.prove_with_aux(g1j[:4], fr[:4], g2a[:4], g1a[:4])
    assert libs[0].ripp_device_bytes() == 0 and libs[1].ripp_device_bytes() == 0


def test_model_accepts_the_edge_inputs(orc):
    """Precondition of test_gpu_gipa_mexp.py::test_edges: tests/model/gipa_generic_oracle.py proves the edge inputs at n = 8 -- scalars 0, 1, r - 1, lambda,
    lambda + 1, 2^128 - 1, 2^128; repeated points in m_a and ck_b; the identity in m_a -- and its verifier accepts the proof."""
    import gipa_generic_oracle as M
    import gipa_mexp_inputs as I
    m_a, m_b, ck_a, ck_b = I.edges(orc)
    assert len(m_a) == 8 and not m_a[6, 12:18].any()                                       # the identity is in
    assert [orc.limbs_to_fr(x) for x in m_b[:7]] == [0, 1, orc.R - 1, I.LAMBDA, I.LAMBDA + 1, (1 << 128) - 1, 1 << 128]
    assert (I.LAMBDA * I.LAMBDA + I.LAMBDA + 1) % orc.R == 0                               # lambda is the eigenvalue of the endomorphism: a primitive cube root of unity mod r
    steps, tr, base, ck_base, com = I.model_prove(orc, m_a, m_b, ck_a, ck_b)
    assert len(steps) == 3 and len(tr) == 3
    assert I.model_verify(orc, ck_a, ck_b, com, steps, base)
    wrong = [com[0], com[1], M.plus("G1", com[2], com[2])]
    assert not I.model_verify(orc, ck_a, ck_b, wrong, steps, base)
