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

`transparent` (and `bind(..).transparent`) holds the transparent scheme of applications/poly_commit/transparent.rs on `ripp_tpc_*`: a resident `CK`
handle, `BivariatePolynomialCommitment`, `UnivariatePolynomialCommitment` and the two tier arguments (`scalar_prove` / `scalar_verify`,
`mexp_prove` / `mexp_verify`); its proofs have the shape of `ripp_amd.poly_commit.transparent`'s.

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


class TPCOpeningStruct(ctypes.Structure):
    """`ripp_tpc_opening` of include/ripp_hip.h (OpeningProof, transparent.rs:80-84)."""
    _fields_ = [("s_com_gt", ctypes.c_void_p), ("s_com_g1", ctypes.c_void_p), ("s_transcript", ctypes.c_void_p), ("s_base_a", _u64(18)), ("s_base_b", _u64(4)),
                ("y_eval_comm", _u64(18)),
                ("f_com_g1", ctypes.c_void_p), ("f_com_fr", ctypes.c_void_p), ("f_transcript", ctypes.c_void_p), ("f_base_a", _u64(4)), ("f_base_b", _u64(4))]


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


def _matrix_args(coeffs):
    """the coefficient arguments of a bivariate entry point: coeffs, rows, cols, stride"""
    c, rows, cols, stride = _matrix(coeffs)
    return [_p(c), _sz(rows), _sz(cols), _sz(stride)]


def _flat_args(polynomial):
    """the coefficient arguments of a univariate entry point: the flat (n, 4) coefficient array and its length"""
    c = np.ascontiguousarray(polynomial, dtype=np.uint64).reshape(-1, 4)
    return [_p(c), _sz(len(c))]


class _Handle:
    """Owner of a resident key handle of the library.  The subclasses that `bind` makes name the library getter, its status check and the two exports
    that read the degrees of a handle and free it."""
    _lib = _check = _degrees = _destroy = None

    def __init__(self, handle):
        self._h = handle

    def degrees(self):
        x, y = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._check(getattr(self._lib(), self._degrees)(self._h, ctypes.byref(x), ctypes.byref(y))); return x.value, y.value

    def close(self):
        if self._h:
            getattr(self._lib(), self._destroy)(self._h); self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _commit(fn, key, coeff_args):
    """`commit` of either scheme, bivariate or univariate -> (AFGHO commitment (72,), first-tier commitments of the y-polynomials (x_degree + 1, 18))"""
    com = np.zeros(72, dtype=np.uint64); y_coms = np.zeros((key.degrees()[0] + 1, 18), dtype=np.uint64)
    key._check(fn(key._h, *coeff_args, _p(com), _p(y_coms))); return com, y_coms


def _open(fn, key, coeff_args, y_polynomial_comms, points, o):
    """`open` of either scheme at (x, y) or (z,) into the opening `o` -> (proof dict, the value there (4,))"""
    yc = np.ascontiguousarray(y_polynomial_comms, dtype=np.uint64).reshape(-1, 18)
    assert len(yc) == key.degrees()[0] + 1
    ev = np.zeros(4, dtype=np.uint64); st = RippStats()
    key._check(fn(key._h, *coeff_args, _p(yc), *(_p(_a(q, 4)) for q in points), ctypes.byref(o.s), _p(ev), ctypes.byref(st)))
    return o.to_proof(st.as_dict()), ev


def _degrees_of(lib, check, export):
    def univariate_degrees(degree):
        """the sqrt split of a univariate degree (mod.rs:299-306, transparent.rs:221-227), computed by the library (needs no device)"""
        x, y = ctypes.c_size_t(0), ctypes.c_size_t(0)
        check(getattr(lib(), export)(_sz(degree), ctypes.byref(x), ctypes.byref(y)))
        return x.value, y.value
    return univariate_degrees


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

    univariate_degrees = _degrees_of(lib, check, "ripp_pc_univariate_degrees")

    def msm_g1_batch(bases, scalars, n=None):
        """out[r] = sum_i scalars[r][i] * bases[i]: bases (n, 12) affine, scalars (rows, cols, 4) with cols <= n -> (rows, 18) projective"""
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 12)
        sc, rows, cols, stride = _matrix(scalars)
        out = np.zeros((rows, 18), dtype=np.uint64)
        check(lib().ripp_msm_g1_batch_a(_p(bases), _sz(len(bases) if n is None else n), _p(sc), _sz(rows), _sz(cols), _sz(stride), _p(out)))
        return out

    class PCSRS(_Handle):
        """`ripp_pc_srs`: the resident SRS of all three schemes."""
        _lib, _check, _degrees, _destroy = staticmethod(lib), staticmethod(check), "ripp_pc_srs_degrees", "ripp_pc_srs_destroy"

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

        def verifier_key(self):
            s = VerifierSRSStruct(); check(lib().ripp_pc_srs_verifier_key(self._h, ctypes.byref(s)))
            return {k: np.ctypeslib.as_array(getattr(s, k)).copy() for k in ("g", "h", "g_beta", "h_alpha")}

        def kzg_powers(self):
            out = np.zeros((self.degrees()[1] + 1, 12), dtype=np.uint64)
            check(lib().ripp_pc_srs_kzg_powers(self._h, _p(out))); return out

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
            return _commit(lib().ripp_pc_commit, srs, _matrix_args(coeffs))

        @staticmethod
        def open(srs, coeffs, y_polynomial_comms, point):
            """-> (proof dict, p(x, y) (4,))"""
            return _open(lib().ripp_pc_open, srs, _matrix_args(coeffs), y_polynomial_comms, point[:2], Opening(_rounds(srs)))

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
            return _commit(lib().ripp_pc_commit_univariate, srs, _flat_args(polynomial))

        @staticmethod
        def open(srs, polynomial, y_polynomial_comms, point):
            """-> (proof dict, p(point) (4,))"""
            return _open(lib().ripp_pc_open_univariate, srs, _flat_args(polynomial), y_polynomial_comms, [point], Opening(_rounds(srs)))

        @staticmethod
        def verify(v_srs, max_degree, com, point, eval, proof):
            vs = vsrs(v_srs); o = Opening.from_proof(proof); acc = ctypes.c_int32(0)
            check(lib().ripp_pc_verify_univariate(ctypes.byref(vs), _sz(max_degree), _p(_a(com, 72)), _p(_a(point, 4)), _p(_a(eval, 4)), ctypes.byref(o.s), _sz(o.rounds), ctypes.byref(acc)))
            return bool(acc.value)

    transparent = _bind_transparent(lib, check)
    return types.SimpleNamespace(transparent=transparent, PCSRS=PCSRS, Opening=Opening, KZG=KZG, BivariatePolynomialCommitment=BivariatePolynomialCommitment,
                                 UnivariatePolynomialCommitment=UnivariatePolynomialCommitment, msm_g1_batch=msm_g1_batch, univariate_degrees=univariate_degrees,
                                 msm_batch_chunks=lambda: int(lib().ripp_msm_batch_chunks()))


def _steps_to_dict(left, inner, base_a, base_b):
    """step arrays in ROUND order -> the GIPAProof dict of ripp_amd.gipa: r_commitment_steps reversed, each side (LMC output, Fr::zero(), [inner product])"""
    zero = np.zeros(4, dtype=np.uint64)
    steps = [((left[2 * r], zero, [inner[2 * r]]), (left[2 * r + 1], zero, [inner[2 * r + 1]])) for r in range(len(left) // 2)]
    return {"r_commitment_steps": steps[::-1], "r_base": (base_a, base_b)}


def _steps_from_dict(proof, left_cols, inner_cols):
    """the inverse: (left (2 r, left_cols), inner (2 r, inner_cols), base_a, base_b), ROUND order"""
    steps = proof["r_commitment_steps"][::-1]
    left = np.zeros((2 * len(steps), left_cols), dtype=np.uint64); inner = np.zeros((2 * len(steps), inner_cols), dtype=np.uint64)
    for r, sides in enumerate(steps):
        for k, side in enumerate(sides):
            left[2 * r + k] = np.asarray(side[0], dtype=np.uint64).reshape(left_cols); inner[2 * r + k] = np.asarray(side[2][0], dtype=np.uint64).reshape(inner_cols)
    return left, inner, proof["r_base"][0], proof["r_base"][1]


def _bind_transparent(lib, check):
    """The transparent scheme (applications/poly_commit/transparent.rs) on `ripp_tpc_*` / `ripp_gipa_ssm_*`: the class names of
    ripp_amd.poly_commit.transparent, limb arrays in, `open` returns (proof, value); proofs have that module's shape, so either `verify` takes either proof."""

    def log2(n):
        return n.bit_length() - 1

    univariate_degrees = _degrees_of(lib, check, "ripp_tpc_univariate_degrees")

    class CK(_Handle):
        """`ripp_tpc_ck`: the resident commitment key (first-tier G1 keys with their extended form, second-tier G2 keys)."""
        _lib, _check, _degrees, _destroy = staticmethod(lib), staticmethod(check), "ripp_tpc_ck_degrees", "ripp_tpc_ck_destroy"

        @staticmethod
        def setup(seed_g1, seed_g2, x_degree, y_degree):
            h = ctypes.c_void_p()
            check(lib().ripp_tpc_ck_setup(ctypes.c_uint64(seed_g1), ctypes.c_uint64(seed_g2), _sz(x_degree), _sz(y_degree), ctypes.byref(h)))
            return CK(h)

        @staticmethod
        def create(first_tier_ck, second_tier_ck):
            """affine keys: (y_degree + 1, 12) and (x_degree + 1, 24)"""
            k1 = np.ascontiguousarray(first_tier_ck, dtype=np.uint64).reshape(-1, 12); k2 = np.ascontiguousarray(second_tier_ck, dtype=np.uint64).reshape(-1, 24)
            h = ctypes.c_void_p()
            check(lib().ripp_tpc_ck_create(_p(k1), _sz(len(k1) - 1), _p(k2), _sz(len(k2) - 1), ctypes.byref(h)))
            return CK(h)

        def keys(self):
            """-> (first_tier_ck (y_degree + 1, 12), second_tier_ck (x_degree + 1, 24)), affine"""
            xd, yd = self.degrees()
            k1 = np.zeros((yd + 1, 12), dtype=np.uint64); k2 = np.zeros((xd + 1, 24), dtype=np.uint64)
            check(lib().ripp_tpc_ck_keys(self._h, _p(k1), _p(k2))); return k1, k2

    class Opening:
        """Owner of a TPCOpeningStruct and of its step arrays."""

        def __init__(self, r2, r1):
            self.s_gt = np.zeros((2 * r2, 72), dtype=np.uint64); self.s_g1 = np.zeros((2 * r2, 18), dtype=np.uint64); self.s_tr = np.zeros((r2, 4), dtype=np.uint64)
            self.f_g1 = np.zeros((2 * r1, 18), dtype=np.uint64); self.f_fr = np.zeros((2 * r1, 4), dtype=np.uint64); self.f_tr = np.zeros((r1, 4), dtype=np.uint64)
            self.s = TPCOpeningStruct()
            self.s.s_com_gt, self.s.s_com_g1, self.s.s_transcript = self.s_gt.ctypes.data, self.s_g1.ctypes.data, self.s_tr.ctypes.data
            self.s.f_com_g1, self.s.f_com_fr, self.s.f_transcript = self.f_g1.ctypes.data, self.f_fr.ctypes.data, self.f_tr.ctypes.data

        def _set(self, name, val, n):
            arr = _a(val, n); ctypes.memmove(getattr(self.s, name), arr.ctypes.data, arr.nbytes)

        def _get(self, name):
            return np.ctypeslib.as_array(getattr(self.s, name)).copy()

        @staticmethod
        def from_proof(proof):
            s_gt, s_g1, sa, sb = _steps_from_dict(proof["second_tier_ip_proof"], 72, 18)
            f_g1, f_fr, fa, fb = _steps_from_dict(proof["first_tier_ip_proof"], 18, 4)
            o = Opening(len(s_gt) // 2, len(f_g1) // 2)
            o.s_gt[:] = s_gt; o.s_g1[:] = s_g1; o.f_g1[:] = f_g1; o.f_fr[:] = f_fr
            o._set("s_base_a", sa, 18); o._set("s_base_b", sb, 4); o._set("f_base_a", fa, 4); o._set("f_base_b", fb, 4); o._set("y_eval_comm", proof["y_eval_comm"], 18)
            return o

        def to_proof(self, stats=None):
            proof = {"second_tier_ip_proof": _steps_to_dict(self.s_gt, self.s_g1, self._get("s_base_a"), self._get("s_base_b")),
                     "y_eval_comm": self._get("y_eval_comm"),
                     "first_tier_ip_proof": _steps_to_dict(self.f_g1, self.f_fr, self._get("f_base_a"), self._get("f_base_b")),
                     "second_tier_transcript": self.s_tr, "first_tier_transcript": self.f_tr}
            if stats is not None:
                proof["stats"] = stats
            return proof

    def scalar_prove(m, b, ck):
        """first tier from host slices: m, b (n, 4), ck (n, 12) affine -> (GIPAProof dict, transcript (r, 4) in round order)"""
        m = np.ascontiguousarray(m, dtype=np.uint64).reshape(-1, 4); b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4); ck = np.ascontiguousarray(ck, dtype=np.uint64).reshape(-1, 12)
        n = len(m); assert len(b) == n and len(ck) == n
        r = max(log2(n), 0)
        g1 = np.zeros((2 * r, 18), dtype=np.uint64); fr = np.zeros((2 * r, 4), dtype=np.uint64); tr = np.zeros((r, 4), dtype=np.uint64)
        a_base = np.zeros(4, dtype=np.uint64); b_base = np.zeros(4, dtype=np.uint64)
        check(lib().ripp_gipa_ssm_scalar_prove(_p(m), _p(b), _p(ck), _sz(n), _p(g1), _p(fr), _p(tr), _p(a_base), _p(b_base), None))
        return _steps_to_dict(g1, fr, a_base, b_base), tr

    def scalar_verify(ck, com, scalar_b, proof):
        """com = (Pedersen commitment (18,), inner product (4,))"""
        ck = np.ascontiguousarray(ck, dtype=np.uint64).reshape(-1, 12)
        g1, fr, a_base, b_base = _steps_from_dict(proof, 18, 4); acc = ctypes.c_int32(0)
        check(lib().ripp_gipa_ssm_scalar_verify(_p(ck), _sz(len(ck)), _p(_a(com[0], 18)), _p(_a(com[1], 4)), _p(_a(scalar_b, 4)), _p(g1), _p(fr), _p(_a(a_base, 4)), _p(_a(b_base, 4)),
                                                ctypes.byref(acc)))
        return bool(acc.value)

    def mexp_prove(m, b, ck):
        """second tier from host slices: m (n, 18) projective, b (n, 4), ck (n, 24) affine -> (GIPAProof dict, transcript)"""
        m = np.ascontiguousarray(m, dtype=np.uint64).reshape(-1, 18); b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4); ck = np.ascontiguousarray(ck, dtype=np.uint64).reshape(-1, 24)
        n = len(m); assert len(b) == n and len(ck) == n
        r = max(log2(n), 0)
        gt = np.zeros((2 * r, 72), dtype=np.uint64); g1 = np.zeros((2 * r, 18), dtype=np.uint64); tr = np.zeros((r, 4), dtype=np.uint64)
        a_base = np.zeros(18, dtype=np.uint64); b_base = np.zeros(4, dtype=np.uint64)
        check(lib().ripp_gipa_ssm_mexp_prove(_p(m), _p(b), _p(ck), _sz(n), _p(gt), _p(g1), _p(tr), _p(a_base), _p(b_base), None))
        return _steps_to_dict(gt, g1, a_base, b_base), tr

    def mexp_verify(ck, com, scalar_b, proof):
        """com = (AFGHO commitment (72,), inner product (18,))"""
        ck = np.ascontiguousarray(ck, dtype=np.uint64).reshape(-1, 24)
        gt, g1, a_base, b_base = _steps_from_dict(proof, 72, 18); acc = ctypes.c_int32(0)
        check(lib().ripp_gipa_ssm_mexp_verify(_p(ck), _sz(len(ck)), _p(_a(com[0], 72)), _p(_a(com[1], 18)), _p(_a(scalar_b, 4)), _p(gt), _p(g1), _p(_a(a_base, 18)), _p(_a(b_base, 4)),
                                              ctypes.byref(acc)))
        return bool(acc.value)

    def round_ms():
        """milliseconds of the commitment + inner-product phase of every round of the last first-tier prover (key lengths n, n / 2, .. 2)"""
        out = (ctypes.c_double * 64)(); k = lib().ripp_tpc_round_ms(out, _sz(64)); return list(out[:k])

    def _opening(ck):
        xd, yd = ck.degrees(); return Opening(log2(xd + 1), log2(yd + 1))

    class BivariatePolynomialCommitment:
        """transparent.rs:86-212; a polynomial is its (rows, cols, 4) coefficient matrix, rows <= x_degree + 1, cols <= y_degree + 1"""

        @staticmethod
        def setup(seed_g1, seed_g2, x_degree, y_degree):
            return CK.setup(seed_g1, seed_g2, x_degree, y_degree)

        @staticmethod
        def commit(ck, coeffs):
            """-> (AFGHO commitment (72,), Pedersen commitments of the y-polynomials (x_degree + 1, 18))"""
            return _commit(lib().ripp_tpc_commit, ck, _matrix_args(coeffs))

        @staticmethod
        def open(ck, coeffs, y_polynomial_comms, point):
            """-> (proof dict, p(x, y) (4,))"""
            return _open(lib().ripp_tpc_open, ck, _matrix_args(coeffs), y_polynomial_comms, point[:2], _opening(ck))

        @staticmethod
        def verify(ck, com, point, eval, proof):
            o = Opening.from_proof(proof); acc = ctypes.c_int32(0)
            check(lib().ripp_tpc_verify(ck._h, _p(_a(com, 72)), _p(_a(point[0], 4)), _p(_a(point[1], 4)), _p(_a(eval, 4)), ctypes.byref(o.s), ctypes.byref(acc)))
            return bool(acc.value)

    class UnivariatePolynomialCommitment:
        """transparent.rs:214-330; a polynomial is its flat (n, 4) coefficient array"""

        bivariate_degrees = staticmethod(univariate_degrees)

        @staticmethod
        def setup(seed_g1, seed_g2, degree):
            return CK.setup(seed_g1, seed_g2, *univariate_degrees(degree))

        @staticmethod
        def commit(ck, polynomial):
            return _commit(lib().ripp_tpc_commit_univariate, ck, _flat_args(polynomial))

        @staticmethod
        def open(ck, polynomial, y_polynomial_comms, point):
            """-> (proof dict, p(point) (4,))"""
            return _open(lib().ripp_tpc_open_univariate, ck, _flat_args(polynomial), y_polynomial_comms, [point], _opening(ck))

        @staticmethod
        def verify(ck, com, point, eval, proof):
            o = Opening.from_proof(proof); acc = ctypes.c_int32(0)
            check(lib().ripp_tpc_verify_univariate(ck._h, _p(_a(com, 72)), _p(_a(point, 4)), _p(_a(eval, 4)), ctypes.byref(o.s), ctypes.byref(acc)))
            return bool(acc.value)

    return types.SimpleNamespace(CK=CK, Opening=Opening, BivariatePolynomialCommitment=BivariatePolynomialCommitment,
                                 UnivariatePolynomialCommitment=UnivariatePolynomialCommitment, univariate_degrees=univariate_degrees,
                                 scalar_prove=scalar_prove, scalar_verify=scalar_verify, mexp_prove=mexp_prove, mexp_verify=mexp_verify, round_ms=round_ms)


_ns = bind()
transparent = _ns.transparent
PCSRS, Opening, KZG = _ns.PCSRS, _ns.Opening, _ns.KZG
BivariatePolynomialCommitment, UnivariatePolynomialCommitment = _ns.BivariatePolynomialCommitment, _ns.UnivariatePolynomialCommitment
msm_g1_batch, univariate_degrees, msm_batch_chunks = _ns.msm_g1_batch, _ns.univariate_degrees, _ns.msm_batch_chunks
