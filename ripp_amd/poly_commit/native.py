"""The polynomial commitments of ip_proofs/src/applications/poly_commit/mod.rs on the library's own entry points (`ripp_pc_*`, `ripp_kzg_*`,
`ripp_msm_g1_batch_a`: include/ripp_hip.h) -- the same class names as the package's Python implementation, which stays as the second
implementation the tests compare against.

Differences from `ripp_amd.poly_commit`:
  * field elements are Montgomery limb arrays -- a coefficient vector is (n, 4) uint64, a bivariate polynomial (rows, cols, 4), a point (4,) -- so no
    per-element Python conversion sits in the path (`ripp_amd.poly_commit.frs` converts lists of integers when a caller has those);
  * the SRS is ONE resident handle (`PCSRS`): KZG powers with their extended form, second-tier SRS and verifier key;
  * `commit` is one batched MSM over the shared powers; partial evaluation, quotient and evaluation run on the device, and `open` returns the
    evaluation it computed beside the proof.
Proofs are dicts of the same shape as the Python implementation's, so either `verify` takes either proof.

    from ripp_amd.poly_commit import native as N
    srs = N.UnivariatePolynomialCommitment.setup(alpha, beta, degree)
    com, y_coms = N.UnivariatePolynomialCommitment.commit(srs, coeffs)
    proof, value = N.UnivariatePolynomialCommitment.open(srs, coeffs, y_coms, z)
    assert N.UnivariatePolynomialCommitment.verify(srs.verifier_key(), degree, com, z, value, proof)

`bind(lib_getter)` gives the same names over another build of the library (BLS12-377: `bind(ripp_amd.bls12_377.lib)`).
"""
import ctypes
import types

import numpy as np

from .._lib import RIPP_ERR_DEVICE, RIPP_ERR_POW2, RIPP_OK, RippStats, VerifierSRSStruct
from .._lib import lib as _default_lib


def _u64(n):
    return ctypes.c_uint64 * n


class PCOpeningStruct(ctypes.Structure):
    """`ripp_pc_opening` of include/ripp_hip.h (OpeningProof, mod.rs:142-146)."""
    _fields_ = [("com_gt", ctypes.c_void_p), ("com_g1", ctypes.c_void_p), ("transcript", ctypes.c_void_p),
                ("base_a", _u64(18)), ("base_b", _u64(4)), ("final_ck_a", _u64(36)), ("opening_a", _u64(36)), ("kzg_challenge", _u64(4)),
                ("y_eval_comm", _u64(18)), ("kzg_proof", _u64(18))]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _a(x, n):
    return np.ascontiguousarray(x, dtype=np.uint64).reshape(n)


def _sz(v):
    return ctypes.c_size_t(int(v))


def _matrix(coeffs):
    """(rows, cols, 4) limbs, possibly a strided view of a wider matrix -> (array that owns the memory, rows, cols, stride in elements)"""
    c = np.asarray(coeffs, dtype=np.uint64)
    if c.ndim != 3 or c.shape[2] != 4:
        raise ValueError(f"expected (rows, cols, 4) Montgomery limbs, got {c.shape}")
    rows, cols = c.shape[0], c.shape[1]
    if rows and cols and c.strides[2] == 8 and c.strides[1] == 32 and c.strides[0] % 32 == 0 and c.strides[0] >= 32 * cols:
        return c, rows, cols, c.strides[0] // 32                 # rows of a wider row-major matrix: passed as they lie, no padded copy
    c = np.ascontiguousarray(c)
    return c, rows, cols, cols


def bind(lib=None):
    """The classes of this module over the library `lib()` returns (default: libripp_hip.so)."""
    lib = lib or _default_lib

    def last_error():
        return lib().ripp_last_error().decode()

    def check(rc):
        if rc == RIPP_OK:
            return
        if rc == RIPP_ERR_POW2:
            raise AssertionError("x_degree + 1 must be a power of two >= 2 for the second-tier argument")
        if rc == RIPP_ERR_DEVICE:
            from ..api import DeviceError
            raise DeviceError("HIP engine unavailable: " + last_error())
        raise ValueError(f"libripp_hip status {rc}: {last_error()}")

    def vsrs(v):
        s = VerifierSRSStruct()
        for k in ("g", "h", "g_beta", "h_alpha"):
            arr = np.ascontiguousarray(v[k], dtype=np.uint64).reshape(-1)
            ctypes.memmove(getattr(s, k), arr.ctypes.data, arr.nbytes)
        return s

    def univariate_degrees(degree):
        """mod.rs:299-306, computed by the library (needs no device)"""
        x, y = ctypes.c_size_t(0), ctypes.c_size_t(0)
        check(lib().ripp_pc_univariate_degrees(_sz(degree), ctypes.byref(x), ctypes.byref(y)))
        return x.value, y.value

    def msm_g1_batch(bases, scalars, n=None):
        """out[r] = sum_i scalars[r][i] * bases[i]: bases (n, 12) affine, scalars (rows, cols, 4) with cols <= n -> (rows, 18) projective"""
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 12)
        sc, rows, cols, stride = _matrix(scalars)
        out = np.zeros((rows, 18), dtype=np.uint64)
        check(lib().ripp_msm_g1_batch_a(_p(bases), _sz(len(bases) if n is None else n), _p(sc), _sz(rows), _sz(cols), _sz(stride), _p(out)))
        return out

    class PCSRS:
        """`ripp_pc_srs`: the resident SRS of all three schemes."""

        def __init__(self, handle):
            self._h = handle

        @staticmethod
        def setup(alpha, beta, x_degree, y_degree):
            h = ctypes.c_void_p()
            check(lib().ripp_pc_srs_setup(_p(_a(alpha, 4)), _p(_a(beta, 4)), _sz(x_degree), _sz(y_degree), ctypes.byref(h)))
            return PCSRS(h)

        @staticmethod
        def create(kzg_powers, h_beta_powers, g_beta, h_alpha):
            kp = np.ascontiguousarray(kzg_powers, dtype=np.uint64).reshape(-1, 12); hb = np.ascontiguousarray(h_beta_powers, dtype=np.uint64).reshape(-1, 36)
            h = ctypes.c_void_p()
            check(lib().ripp_pc_srs_create(_p(kp), _sz(len(kp) - 1), _p(hb), _sz((len(hb) - 1) // 2), _p(_a(g_beta, 18)), _p(_a(h_alpha, 36)), ctypes.byref(h)))
            return PCSRS(h)

        def degrees(self):
            x, y = ctypes.c_size_t(0), ctypes.c_size_t(0)
            check(lib().ripp_pc_srs_degrees(self._h, ctypes.byref(x), ctypes.byref(y))); return x.value, y.value

        def verifier_key(self):
            s = VerifierSRSStruct(); check(lib().ripp_pc_srs_verifier_key(self._h, ctypes.byref(s)))
            return {k: np.ctypeslib.as_array(getattr(s, k)).copy() for k in ("g", "h", "g_beta", "h_alpha")}

        def kzg_powers(self):
            out = np.zeros((self.degrees()[1] + 1, 12), dtype=np.uint64)
            check(lib().ripp_pc_srs_kzg_powers(self._h, _p(out))); return out

        def close(self):
            if self._h:
                lib().ripp_pc_srs_destroy(self._h); self._h = ctypes.c_void_p()

        def __del__(self):
            try:
                self.close()
            except Exception:
                pass

    class Opening:
        """Owner of a PCOpeningStruct and of its step arrays."""

        def __init__(self, rounds):
            self.rounds = rounds
            self.com_gt = np.zeros((rounds * 2, 72), dtype=np.uint64); self.com_g1 = np.zeros((rounds * 2, 18), dtype=np.uint64); self.tr = np.zeros((rounds, 4), dtype=np.uint64)
            self.s = PCOpeningStruct()
            self.s.com_gt, self.s.com_g1, self.s.transcript = self.com_gt.ctypes.data, self.com_g1.ctypes.data, self.tr.ctypes.data

        @staticmethod
        def from_proof(proof):
            ip = proof["ip_proof"]
            com_gt = np.ascontiguousarray(ip["com_gt"], dtype=np.uint64).reshape(-1, 72)
            o = Opening(len(com_gt) // 2)
            o.com_gt[:] = com_gt; o.com_g1[:] = np.asarray(ip["com_g1"], dtype=np.uint64).reshape(-1, 18)
            if "tr" in ip:
                o.tr[:] = np.asarray(ip["tr"], dtype=np.uint64).reshape(-1, 4)
            for name, key, n in (("base_a", "base_a", 18), ("final_ck_a", "final_ck_a", 36), ("opening_a", "opening_a", 36)):
                arr = _a(ip[key], n); ctypes.memmove(getattr(o.s, name), arr.ctypes.data, arr.nbytes)
            for name, val, n in (("y_eval_comm", proof["y_eval_comm"], 18), ("kzg_proof", proof["kzg_proof"], 18)):
                arr = _a(val, n); ctypes.memmove(getattr(o.s, name), arr.ctypes.data, arr.nbytes)
            return o

        def to_proof(self, stats=None):
            f = lambda name: np.ctypeslib.as_array(getattr(self.s, name)).copy()
            ip = dict(com_gt=self.com_gt, com_g1=self.com_g1, tr=self.tr, base_a=f("base_a"), base_b=f("base_b"), final_ck_a=f("final_ck_a"), opening_a=f("opening_a"),
                      kzg_c=f("kzg_challenge"))
            if stats is not None:
                ip["stats"] = stats
            return {"ip_proof": ip, "y_eval_comm": f("y_eval_comm"), "kzg_proof": f("kzg_proof")}

    def _rounds(srs):
        return max((srs.degrees()[0] + 1).bit_length() - 1, 1)

    class KZG:
        """mod.rs:50-119"""

        @staticmethod
        def setup(alpha, beta, degree):
            """mod.rs:56-76 with the trapdoors given: a KZG-only handle (x_degree 0)"""
            return PCSRS.setup(alpha, beta, 0, degree)

        @staticmethod
        def commit(srs, polynomial):
            c = np.ascontiguousarray(polynomial, dtype=np.uint64).reshape(-1, 4); out = np.zeros(18, dtype=np.uint64)
            check(lib().ripp_kzg_commit(srs._h, _p(c), _sz(len(c)), _p(out))); return out

        @staticmethod
        def open(srs, polynomial, point):
            """-> (proof (18,), p(point) (4,))"""
            c = np.ascontiguousarray(polynomial, dtype=np.uint64).reshape(-1, 4); proof = np.zeros(18, dtype=np.uint64); ev = np.zeros(4, dtype=np.uint64)
            check(lib().ripp_kzg_open(srs._h, _p(c), _sz(len(c)), _p(_a(point, 4)), _p(proof), _p(ev))); return proof, ev

        @staticmethod
        def verify(v_srs, com, point, eval, proof):
            vs = vsrs(v_srs); acc = ctypes.c_int32(0)
            check(lib().ripp_kzg_verify(ctypes.byref(vs), _p(_a(com, 18)), _p(_a(point, 4)), _p(_a(eval, 4)), _p(_a(proof, 18)), ctypes.byref(acc)))
            return bool(acc.value)

    class BivariatePolynomialCommitment:
        """mod.rs:142-296; a polynomial is its (rows, cols, 4) coefficient matrix, rows <= x_degree + 1, cols <= y_degree + 1"""

        @staticmethod
        def setup(alpha, beta, x_degree, y_degree):
            return PCSRS.setup(alpha, beta, x_degree, y_degree)

        @staticmethod
        def commit(srs, coeffs):
            """-> (AFGHO commitment (72,), KZG commitments of the y-polynomials (x_degree + 1, 18))"""
            c, rows, cols, stride = _matrix(coeffs)
            com = np.zeros(72, dtype=np.uint64); y_coms = np.zeros((srs.degrees()[0] + 1, 18), dtype=np.uint64)
            check(lib().ripp_pc_commit(srs._h, _p(c), _sz(rows), _sz(cols), _sz(stride), _p(com), _p(y_coms))); return com, y_coms

        @staticmethod
        def open(srs, coeffs, y_polynomial_comms, point):
            """-> (proof dict, p(x, y) (4,))"""
            c, rows, cols, stride = _matrix(coeffs)
            yc = np.ascontiguousarray(y_polynomial_comms, dtype=np.uint64).reshape(-1, 18)
            assert len(yc) == srs.degrees()[0] + 1
            o = Opening(_rounds(srs)); ev = np.zeros(4, dtype=np.uint64); st = RippStats()
            check(lib().ripp_pc_open(srs._h, _p(c), _sz(rows), _sz(cols), _sz(stride), _p(yc), _p(_a(point[0], 4)), _p(_a(point[1], 4)), ctypes.byref(o.s), _p(ev), ctypes.byref(st)))
            return o.to_proof(st.as_dict()), ev

        @staticmethod
        def verify(v_srs, com, point, eval, proof):
            vs = vsrs(v_srs); o = Opening.from_proof(proof); acc = ctypes.c_int32(0)
            check(lib().ripp_pc_verify(ctypes.byref(vs), _p(_a(com, 72)), _p(_a(point[0], 4)), _p(_a(point[1], 4)), _p(_a(eval, 4)), ctypes.byref(o.s), _sz(o.rounds), ctypes.byref(acc)))
            return bool(acc.value)

    class UnivariatePolynomialCommitment:
        """mod.rs:298-388; a polynomial is its flat (n, 4) coefficient array"""

        bivariate_degrees = staticmethod(univariate_degrees)

        @staticmethod
        def setup(alpha, beta, degree):
            return PCSRS.setup(alpha, beta, *univariate_degrees(degree))

        @staticmethod
        def commit(srs, polynomial):
            c = np.ascontiguousarray(polynomial, dtype=np.uint64).reshape(-1, 4)
            com = np.zeros(72, dtype=np.uint64); y_coms = np.zeros((srs.degrees()[0] + 1, 18), dtype=np.uint64)
            check(lib().ripp_pc_commit_univariate(srs._h, _p(c), _sz(len(c)), _p(com), _p(y_coms))); return com, y_coms

        @staticmethod
        def open(srs, polynomial, y_polynomial_comms, point):
            """-> (proof dict, p(point) (4,))"""
            c = np.ascontiguousarray(polynomial, dtype=np.uint64).reshape(-1, 4)
            yc = np.ascontiguousarray(y_polynomial_comms, dtype=np.uint64).reshape(-1, 18)
            assert len(yc) == srs.degrees()[0] + 1
            o = Opening(_rounds(srs)); ev = np.zeros(4, dtype=np.uint64); st = RippStats()
            check(lib().ripp_pc_open_univariate(srs._h, _p(c), _sz(len(c)), _p(yc), _p(_a(point, 4)), ctypes.byref(o.s), _p(ev), ctypes.byref(st)))
            return o.to_proof(st.as_dict()), ev

        @staticmethod
        def verify(v_srs, max_degree, com, point, eval, proof):
            vs = vsrs(v_srs); o = Opening.from_proof(proof); acc = ctypes.c_int32(0)
            check(lib().ripp_pc_verify_univariate(ctypes.byref(vs), _sz(max_degree), _p(_a(com, 72)), _p(_a(point, 4)), _p(_a(eval, 4)), ctypes.byref(o.s), _sz(o.rounds), ctypes.byref(acc)))
            return bool(acc.value)

    return types.SimpleNamespace(PCSRS=PCSRS, Opening=Opening, KZG=KZG, BivariatePolynomialCommitment=BivariatePolynomialCommitment,
                                 UnivariatePolynomialCommitment=UnivariatePolynomialCommitment, msm_g1_batch=msm_g1_batch, univariate_degrees=univariate_degrees,
                                 msm_batch_chunks=lambda: int(lib().ripp_msm_batch_chunks()))


_ns = bind()
PCSRS, Opening, KZG = _ns.PCSRS, _ns.Opening, _ns.KZG
BivariatePolynomialCommitment, UnivariatePolynomialCommitment = _ns.BivariatePolynomialCommitment, _ns.UnivariatePolynomialCommitment
msm_g1_batch, univariate_degrees, msm_batch_chunks = _ns.msm_g1_batch, _ns.univariate_degrees, _ns.msm_batch_chunks
