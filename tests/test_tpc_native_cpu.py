"""CPU: the transparent polynomial-commitment surface of the C ABI (include/ripp_hip.h section "transparent polynomial commitments", tpc_api.inc) as far as
it can be checked without a device: the exports exist in both libraries, `ripp_tpc_univariate_degrees` is the reference's split (transparent.rs:221-227),
argument errors are reported before the device is looked for, every compute entry point refuses with RIPP_ERR_DEVICE when there is none, and none of that
allocates device memory."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_EXPORTS = ("ripp_tpc_univariate_degrees", "ripp_tpc_ck_setup", "ripp_tpc_ck_create", "ripp_tpc_ck_destroy", "ripp_tpc_ck_degrees", "ripp_tpc_ck_keys",
               "ripp_tpc_commit", "ripp_tpc_open", "ripp_tpc_verify", "ripp_tpc_commit_univariate", "ripp_tpc_open_univariate", "ripp_tpc_verify_univariate",
               "ripp_gipa_ssm_scalar_prove", "ripp_gipa_ssm_scalar_verify", "ripp_gipa_ssm_mexp_prove", "ripp_gipa_ssm_mexp_verify", "ripp_tpc_round_ms")
OK, POW2, DEVICE, ARG = 0, 2, 3, 4


@pytest.fixture(scope="module")
def hiplib():
    from ripp_amd._lib import lib
    return lib()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sz(v):
    return ctypes.c_size_t(v)


def test_header_declares_and_both_libraries_export_the_new_names(hiplib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ripp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ripp_[a-z0-9_]+)\s*\(", src))
    import ripp_amd.bls12_377 as R7
    L7 = R7.lib()
    for name in NEW_EXPORTS:
        assert name in declared, f"{name} is not declared in include/ripp_hip.h"
        assert hasattr(hiplib, name), f"{name} is not exported by libripp_hip.so"
        assert hasattr(L7, name), f"{name} is not exported by libripp_hip_377.so"
    assert "typedef struct ripp_tpc_ck ripp_tpc_ck;" in src and re.search(r"\}\s*ripp_tpc_opening\s*;", src)
    assert "#define RIPP_ABI_VERSION 7" in src


def _degrees(L, degree):
    x, y = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = L.ripp_tpc_univariate_degrees(_sz(degree), ctypes.byref(x), ctypes.byref(y))
    return rc, x.value, y.value


def test_univariate_degrees_equal_the_python_split(hiplib):
    """transparent.rs:221-227 against UnivariatePolynomialCommitment.bivariate_degrees of ripp_amd.poly_commit.transparent"""
    from ripp_amd.poly_commit.transparent import UnivariatePolynomialCommitment as U
    for degree in list(range(1, 4097)) + [65535, (1 << 20) - 1, (1 << 24) - 1]:
        rc, x, y = _degrees(hiplib, degree)
        assert rc == OK and (x, y) == U.bivariate_degrees(degree), degree
        assert (x + 1) * (y + 1) >= degree + 1 and (x + 1) & x == 0 and (y + 1) & y == 0
    assert _degrees(hiplib, 65535) == (OK, 63, 1023) and _degrees(hiplib, (1 << 20) - 1) == (OK, 255, 4095)
    with pytest.raises(ZeroDivisionError):                     # the reference divides by the zero skew factor
        U.bivariate_degrees(0)
    assert _degrees(hiplib, 0)[0] == ARG
    assert hiplib.ripp_tpc_univariate_degrees(_sz(100), None, None) == ARG
    from ripp_amd.poly_commit import native as N
    assert N.transparent.univariate_degrees(65535) == (63, 1023) and N.transparent.UnivariatePolynomialCommitment.bivariate_degrees(56) == U.bivariate_degrees(56)


def _opening(N):
    return N.transparent.Opening(1, 2)


def test_argument_errors_come_before_the_device(hiplib):
    """NULL pointers and stride < cols are RIPP_ERR_ARG, degrees / lengths that are no power of two >= 2 RIPP_ERR_POW2 -- with or without a device"""
    from ripp_amd.poly_commit import native as N
    L = hiplib
    fr = np.zeros((8, 4), dtype=np.uint64); g1 = np.zeros((8, 12), dtype=np.uint64); g2 = np.zeros((8, 24), dtype=np.uint64)
    out = np.zeros((8, 18), dtype=np.uint64); gt = np.zeros((8, 72), dtype=np.uint64); h = ctypes.c_void_p(); acc = ctypes.c_int32(-1)
    fake = np.zeros(64, dtype=np.uint64)                       # stands in for a handle where the call must fail before it reads one
    o = _opening(N)
    assert L.ripp_tpc_ck_setup(ctypes.c_uint64(1), ctypes.c_uint64(2), _sz(1), _sz(3), None) == ARG
    for xd, yd in ((2, 3), (1, 4), (0, 3), (1, 0), (5, 5)):
        assert L.ripp_tpc_ck_setup(ctypes.c_uint64(1), ctypes.c_uint64(2), _sz(xd), _sz(yd), ctypes.byref(h)) == POW2 and not h.value, (xd, yd)
        assert L.ripp_tpc_ck_create(_p(g1), _sz(yd), _p(g2), _sz(xd), ctypes.byref(h)) == POW2 and not h.value, (xd, yd)
    assert b"powers of two" in L.ripp_last_error()
    assert L.ripp_tpc_ck_create(None, _sz(3), _p(g2), _sz(1), ctypes.byref(h)) == ARG
    assert L.ripp_tpc_ck_create(_p(g1), _sz(3), None, _sz(1), ctypes.byref(h)) == ARG
    assert L.ripp_tpc_ck_create(_p(g1), _sz(3), _p(g2), _sz(1), None) == ARG
    for fn, args in (("ripp_tpc_ck_degrees", (None, None, None)), ("ripp_tpc_ck_keys", (None, _p(g1), _p(g2))), ("ripp_tpc_ck_keys", (_p(fake), None, _p(g2))),
                     ("ripp_tpc_commit", (None, _p(fr), _sz(1), _sz(4), _sz(4), _p(gt), _p(out))),
                     ("ripp_tpc_commit", (_p(fake), None, _sz(1), _sz(4), _sz(4), _p(gt), _p(out))),
                     ("ripp_tpc_commit", (_p(fake), _p(fr), _sz(1), _sz(4), _sz(4), None, _p(out))),
                     ("ripp_tpc_commit", (_p(fake), _p(fr), _sz(2), _sz(4), _sz(3), _p(gt), _p(out))),                                 # stride < cols
                     ("ripp_tpc_open", (_p(fake), _p(fr), _sz(2), _sz(4), _sz(3), _p(out), _p(fr), _p(fr), ctypes.byref(o.s), None, None)),      # stride < cols
                     ("ripp_tpc_open", (_p(fake), _p(fr), _sz(2), _sz(4), _sz(4), _p(out), _p(fr), _p(fr), None, None, None)),
                     ("ripp_tpc_open", (None, _p(fr), _sz(2), _sz(4), _sz(4), _p(out), _p(fr), _p(fr), ctypes.byref(o.s), None, None)),
                     ("ripp_tpc_verify", (None, _p(gt), _p(fr), _p(fr), _p(fr), ctypes.byref(o.s), ctypes.byref(acc))),
                     ("ripp_tpc_verify", (_p(fake), _p(gt), _p(fr), _p(fr), _p(fr), ctypes.byref(o.s), None)),
                     ("ripp_tpc_commit_univariate", (None, _p(fr), _sz(4), _p(gt), _p(out))), ("ripp_tpc_commit_univariate", (_p(fake), None, _sz(4), _p(gt), _p(out))),
                     ("ripp_tpc_open_univariate", (None, _p(fr), _sz(4), _p(out), _p(fr), ctypes.byref(o.s), None, None)),
                     ("ripp_tpc_open_univariate", (_p(fake), _p(fr), _sz(4), _p(out), _p(fr), None, None, None)),
                     ("ripp_tpc_verify_univariate", (None, _p(gt), _p(fr), _p(fr), ctypes.byref(o.s), ctypes.byref(acc))),
                     ("ripp_gipa_ssm_scalar_prove", (None, _p(fr), _p(g1), _sz(4), _p(out), _p(fr), _p(fr), _p(fr), _p(fr), None)),
                     ("ripp_gipa_ssm_scalar_prove", (_p(fr), _p(fr), None, _sz(4), _p(out), _p(fr), _p(fr), _p(fr), _p(fr), None)),
                     ("ripp_gipa_ssm_scalar_verify", (_p(g1), _sz(4), _p(out), _p(fr), None, _p(out), _p(fr), _p(fr), _p(fr), ctypes.byref(acc))),
                     ("ripp_gipa_ssm_mexp_prove", (_p(out), None, _p(g2), _sz(4), _p(gt), _p(out), _p(fr), _p(out), _p(fr), None)),
                     ("ripp_gipa_ssm_mexp_verify", (_p(g2), _sz(4), None, _p(out), _p(fr), _p(gt), _p(out), _p(out), _p(fr), ctypes.byref(acc)))):
        assert getattr(L, fn)(*args) == ARG, fn
    # an opening with a missing step array is an argument error too
    broken = _opening(N); broken.s.f_com_fr = None
    assert L.ripp_tpc_verify(_p(fake), _p(gt), _p(fr), _p(fr), _p(fr), ctypes.byref(broken.s), ctypes.byref(acc)) == ARG
    for n in (0, 1, 3, 6):
        assert L.ripp_gipa_ssm_scalar_prove(_p(fr), _p(fr), _p(g1), _sz(n), _p(out), _p(fr), _p(fr), _p(fr), _p(fr), None) == POW2, n
        assert L.ripp_gipa_ssm_scalar_verify(_p(g1), _sz(n), _p(out), _p(fr), _p(fr), _p(out), _p(fr), _p(fr), _p(fr), ctypes.byref(acc)) == POW2, n
        assert L.ripp_gipa_ssm_mexp_prove(_p(out), _p(fr), _p(g2), _sz(n), _p(gt), _p(out), _p(fr), _p(out), _p(fr), None) == POW2, n
        assert L.ripp_gipa_ssm_mexp_verify(_p(g2), _sz(n), _p(gt), _p(out), _p(fr), _p(gt), _p(out), _p(out), _p(fr), ctypes.byref(acc)) == POW2, n
    assert acc.value == -1
    L.ripp_tpc_ck_destroy.restype = None; L.ripp_tpc_ck_destroy.argtypes = [ctypes.c_void_p]
    L.ripp_tpc_ck_destroy(None)                                                                                  # a no-op, like the other destroyers
    assert L.ripp_device_bytes() == 0 or L.ripp_device_count() > 0


def test_no_device_means_status_3_and_no_memory(hiplib):
    if hiplib.ripp_device_count() > 0:
        pytest.skip("a HIP device is present; the refusal path is exercised on the CPU-only builder")
    from ripp_amd.poly_commit import native as N
    import ripp_amd as R
    L = hiplib; T = N.transparent
    fr = np.zeros((8, 4), dtype=np.uint64); fr[:, 0] = 1; g1 = np.zeros((8, 12), dtype=np.uint64); g2 = np.zeros((8, 24), dtype=np.uint64)
    out = np.zeros((8, 18), dtype=np.uint64); gt = np.zeros((8, 72), dtype=np.uint64); h = ctypes.c_void_p(); acc = ctypes.c_int32(-1)
    fake = np.zeros(64, dtype=np.uint64)                       # no handle can exist without a device; every call below must refuse before it reads one
    o = _opening(N)
    assert L.ripp_tpc_ck_setup(ctypes.c_uint64(700), ctypes.c_uint64(900), _sz(1), _sz(3), ctypes.byref(h)) == DEVICE and not h.value
    assert L.ripp_tpc_ck_create(_p(g1), _sz(3), _p(g2), _sz(1), ctypes.byref(h)) == DEVICE and not h.value
    assert L.ripp_tpc_ck_keys(_p(fake), _p(g1), _p(g2)) == DEVICE
    assert L.ripp_tpc_commit(_p(fake), _p(fr), _sz(2), _sz(4), _sz(4), _p(gt), _p(out)) == DEVICE
    assert L.ripp_tpc_open(_p(fake), _p(fr), _sz(2), _sz(4), _sz(4), _p(out), _p(fr), _p(fr), ctypes.byref(o.s), None, None) == DEVICE
    assert L.ripp_tpc_verify(_p(fake), _p(gt), _p(fr), _p(fr), _p(fr), ctypes.byref(o.s), ctypes.byref(acc)) == DEVICE
    assert L.ripp_tpc_commit_univariate(_p(fake), _p(fr), _sz(8), _p(gt), _p(out)) == DEVICE
    assert L.ripp_tpc_open_univariate(_p(fake), _p(fr), _sz(8), _p(out), _p(fr), ctypes.byref(o.s), None, None) == DEVICE
    assert L.ripp_tpc_verify_univariate(_p(fake), _p(gt), _p(fr), _p(fr), ctypes.byref(o.s), ctypes.byref(acc)) == DEVICE
    assert L.ripp_gipa_ssm_scalar_prove(_p(fr), _p(fr), _p(g1), _sz(4), _p(out), _p(fr), _p(fr), _p(fr), _p(fr), None) == DEVICE
    assert L.ripp_gipa_ssm_scalar_verify(_p(g1), _sz(4), _p(out), _p(fr), _p(fr), _p(out), _p(fr), _p(fr), _p(fr), ctypes.byref(acc)) == DEVICE
    assert L.ripp_gipa_ssm_mexp_prove(_p(out), _p(fr), _p(g2), _sz(4), _p(gt), _p(out), _p(fr), _p(out), _p(fr), None) == DEVICE
    assert L.ripp_gipa_ssm_mexp_verify(_p(g2), _sz(4), _p(gt), _p(out), _p(fr), _p(gt), _p(out), _p(out), _p(fr), ctypes.byref(acc)) == DEVICE
    assert acc.value == -1
    with pytest.raises(R.DeviceError):
        T.CK.setup(700, 900, 1, 3)
    with pytest.raises(R.DeviceError):
        T.UnivariatePolynomialCommitment.setup(700, 900, 56)
    with pytest.raises(R.DeviceError):
        T.scalar_prove(fr[:4], fr[:4], g1[:4])
    assert L.ripp_tpc_round_ms(None, _sz(0)) == 0
    assert L.ripp_device_bytes() == 0
