"""CPU: the native polynomial-commitment surface of the C ABI (include/ripp_hip.h section "polynomial commitments", poly_commit_api.inc) as far as it
can be checked without a device: the exports exist in both libraries, `ripp_pc_univariate_degrees` is the reference's sqrt split (mod.rs:299-306),
argument errors are reported before the device is looked for, every compute entry point refuses with RIPP_ERR_DEVICE when there is none, and none of
that allocates device memory.

(The one argument error that needs a live handle -- more coefficients than the SRS has powers -- is in tests/test_gpu_poly_commit_native.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_EXPORTS = ("ripp_pc_univariate_degrees", "ripp_pc_srs_setup", "ripp_pc_srs_create", "ripp_pc_srs_destroy", "ripp_pc_srs_degrees", "ripp_pc_srs_verifier_key",
               "ripp_pc_srs_kzg_powers", "ripp_msm_g1_batch_a", "ripp_msm_batch_chunks", "ripp_kzg_commit", "ripp_kzg_open", "ripp_kzg_verify", "ripp_pc_commit", "ripp_pc_open",
               "ripp_pc_verify", "ripp_pc_commit_univariate", "ripp_pc_open_univariate", "ripp_pc_verify_univariate")


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
    assert "typedef struct ripp_pc_srs ripp_pc_srs;" in src and re.search(r"\}\s*ripp_pc_opening\s*;", src)
    # the ABI guard did not move: no member was added to ripp_config / ripp_stats for this surface
    assert "#define RIPP_ABI_VERSION 7" in src


def _degrees(L, degree):
    x, y = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = L.ripp_pc_univariate_degrees(_sz(degree), ctypes.byref(x), ctypes.byref(y))
    return rc, x.value, y.value


def test_univariate_degrees_equal_the_python_split(hiplib):
    """mod.rs:299-306 against UnivariatePolynomialCommitment.bivariate_degrees of the Python implementation"""
    from ripp_amd.poly_commit import UnivariatePolynomialCommitment as U
    for degree in list(range(1, 5001)) + [(1 << k) - 1 for k in range(1, 27)] + [(1 << k) for k in range(1, 27)]:
        rc, x, y = _degrees(hiplib, degree)
        assert rc == 0 and (x, y) == U.bivariate_degrees(degree), degree
        assert (x + 1) * (y + 1) >= degree + 1 and (x + 1) & x == 0
    assert _degrees(hiplib, 65535) == (0, 15, 4095) and _degrees(hiplib, (1 << 20) - 1) == (0, 63, 16383)
    # degree 0: the reference's skew factor is sqrt / 2 = 0 and its division panics (the Python implementation raises ZeroDivisionError)
    with pytest.raises(ZeroDivisionError):
        U.bivariate_degrees(0)
    assert _degrees(hiplib, 0)[0] == 4
    assert hiplib.ripp_pc_univariate_degrees(_sz(100), None, None) == 4
    from ripp_amd.poly_commit import native as N
    assert N.univariate_degrees(65535) == (15, 4095) and N.UnivariatePolynomialCommitment.bivariate_degrees(56) == U.bivariate_degrees(56)


def test_argument_errors_come_before_the_device(hiplib):
    """RIPP_ERR_ARG = 4 for NULL pointers, cols > n, stride < cols and a second-tier length that is no power of two -- with or without a device"""
    fr = np.zeros((8, 4), dtype=np.uint64); g1 = np.zeros((8, 12), dtype=np.uint64); out = np.zeros((8, 18), dtype=np.uint64); h = ctypes.c_void_p()
    L = hiplib
    assert L.ripp_msm_g1_batch_a(_p(g1), _sz(4), _p(fr), _sz(1), _sz(5), _sz(5), _p(out)) == 4                 # cols > n
    assert b"cols" in L.ripp_last_error()
    assert L.ripp_msm_g1_batch_a(_p(g1), _sz(8), _p(fr), _sz(2), _sz(4), _sz(3), _p(out)) == 4                 # stride < cols
    assert b"stride" in L.ripp_last_error()
    assert L.ripp_msm_g1_batch_a(None, _sz(8), _p(fr), _sz(2), _sz(4), _sz(4), _p(out)) == 4
    assert L.ripp_msm_g1_batch_a(_p(g1), _sz(8), None, _sz(2), _sz(4), _sz(4), _p(out)) == 4
    assert L.ripp_msm_g1_batch_a(_p(g1), _sz(8), _p(fr), _sz(2), _sz(4), _sz(4), None) == 4
    assert L.ripp_msm_g1_batch_a(None, _sz(8), None, _sz(0), _sz(4), _sz(4), None) == 0                          # rows == 0: nothing to write
    assert L.ripp_pc_srs_setup(None, _p(fr), _sz(1), _sz(3), ctypes.byref(h)) == 4
    assert L.ripp_pc_srs_setup(_p(fr), _p(fr), _sz(1), _sz(3), None) == 4
    assert L.ripp_pc_srs_setup(_p(fr), _p(fr), _sz(2), _sz(3), ctypes.byref(h)) == 4 and not h.value          # x_degree + 1 = 3
    assert L.ripp_pc_srs_create(None, _sz(3), None, _sz(1), None, None, ctypes.byref(h)) == 4
    for fn, args in (("ripp_kzg_commit", (None, _p(fr), _sz(4), _p(out))), ("ripp_kzg_open", (None, _p(fr), _sz(4), _p(fr), _p(out), None)),
                     ("ripp_pc_commit", (None, _p(fr), _sz(1), _sz(4), _sz(4), _p(out), _p(out))), ("ripp_pc_commit_univariate", (None, _p(fr), _sz(4), _p(out), _p(out))),
                     ("ripp_pc_open", (None, _p(fr), _sz(1), _sz(4), _sz(4), _p(out), _p(fr), _p(fr), None, None, None)),
                     ("ripp_pc_open_univariate", (None, _p(fr), _sz(4), _p(out), _p(fr), None, None, None)),
                     ("ripp_kzg_verify", (None, _p(out), _p(fr), _p(fr), _p(out), None)), ("ripp_pc_verify", (None, None, _p(fr), _p(fr), _p(fr), None, _sz(1), None)),
                     ("ripp_pc_verify_univariate", (None, _sz(56), None, _p(fr), _p(fr), None, _sz(1), None)),
                     ("ripp_pc_srs_degrees", (None, None, None)), ("ripp_pc_srs_verifier_key", (None, None)), ("ripp_pc_srs_kzg_powers", (None, None))):
        assert getattr(L, fn)(*args) == 4, fn
    L.ripp_pc_srs_destroy.restype = None; L.ripp_pc_srs_destroy.argtypes = [ctypes.c_void_p]
    L.ripp_pc_srs_destroy(None)                                                                                  # a no-op, like the other destroyers
    assert L.ripp_device_bytes() == 0 or L.ripp_device_count() > 0


def test_no_device_means_status_3_and_no_memory(hiplib):
    if hiplib.ripp_device_count() > 0:
        pytest.skip("a HIP device is present; the refusal path is exercised on the CPU-only builder")
    from ripp_amd.poly_commit import native as N
    from ripp_amd._lib import VerifierSRSStruct
    import ripp_amd as R
    L = hiplib
    fr = np.zeros((8, 4), dtype=np.uint64); fr[:, 0] = 1; g1 = np.zeros((8, 12), dtype=np.uint64); g2 = np.zeros((3, 36), dtype=np.uint64)
    out = np.zeros((8, 18), dtype=np.uint64); gt = np.zeros(72, dtype=np.uint64); h = ctypes.c_void_p(); acc = ctypes.c_int32(-1)
    assert L.ripp_pc_srs_setup(_p(fr), _p(fr[1:]), _sz(1), _sz(3), ctypes.byref(h)) == 3 and not h.value
    assert L.ripp_pc_srs_create(_p(g1), _sz(3), _p(g2), _sz(1), _p(out), _p(g2), ctypes.byref(h)) == 3 and not h.value
    assert L.ripp_msm_g1_batch_a(_p(g1), _sz(8), _p(fr), _sz(2), _sz(4), _sz(4), _p(out)) == 3
    vs = VerifierSRSStruct(); o = N.Opening(1)
    assert L.ripp_kzg_verify(ctypes.byref(vs), _p(out), _p(fr), _p(fr), _p(out), ctypes.byref(acc)) == 3
    assert L.ripp_pc_verify(ctypes.byref(vs), _p(gt), _p(fr), _p(fr), _p(fr), ctypes.byref(o.s), _sz(1), ctypes.byref(acc)) == 3
    assert L.ripp_pc_verify_univariate(ctypes.byref(vs), _sz(56), _p(gt), _p(fr), _p(fr), ctypes.byref(o.s), _sz(1), ctypes.byref(acc)) == 3
    assert acc.value == -1
    # commit and open need a handle, and no handle can exist without a device: the bindings surface the refusal of setup
    with pytest.raises(R.DeviceError):
        N.KZG.setup(fr[0], fr[1], 7)
    with pytest.raises(R.DeviceError):
        N.UnivariatePolynomialCommitment.setup(fr[0], fr[1], 56)
    with pytest.raises(R.DeviceError):
        N.msm_g1_batch(g1, fr.reshape(2, 4, 4))
    assert L.ripp_msm_batch_chunks() == 0
    assert L.ripp_device_bytes() == 0


def test_import_is_lazy():
    """`import ripp_amd.poly_commit` behaves as before: the native module is a sub-module nobody imports for the caller"""
    import subprocess
    import sys
    code = "import sys; import ripp_amd.poly_commit as P; assert 'ripp_amd.poly_commit.native' not in sys.modules; assert hasattr(P, 'KZG') and hasattr(P, 'transparent')"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
