"""GPU (-m gpu): representation invariance through the shipping library, both curves.  The same G1 / G2 points are fed in Jacobian form with
Z in {1, p - 1, 2, (p + 1) / 2, random} and with Z chosen so that X = p - 1 (a square root of -1/x, where one exists), each as a whole vector and mixed
per element.  normalize_batch_g1 / g2, the Jacobian folds, msm_g1_j / msm_g2_j and pairing_product_j must give what they give for Z = 1, and what the
CPU oracle gives."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 64


def _sqrt(a, P):
    """a square root of a mod P (Tonelli-Shanks), or None"""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 2, P) != 1:
        return None
    q, s = P - 1, 0
    while q % 2 == 0:
        q //= 2; s += 1
    z = 2
    while pow(z, (P - 1) // 2, P) != P - 1:
        z += 1
    m, c, t, r = s, pow(z, q, P), pow(a, q, P), pow(a, (q + 1) // 2, P)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % P; i += 1
        b = pow(c, 1 << (m - i - 1), P)
        m, c, t, r = i, b * b % P, t * b * b % P, r * b % P
    assert r * r % P == a
    return r


@pytest.fixture(scope="module", params=["381", "377"])
def curve(request, engine, orc):
    if request.param == "381":
        return engine, orc
    import orclib377
    import ripp_amd.bls12_377 as R377
    orclib377.lib()
    R377.init(0)
    return R377, orclib377


def _z_choices(o, xs, rng):
    """per point: the Z of each kind; 'xm1' makes X = x Z^2 = p - 1 (falls back to a random Z where -1/x is not a square)"""
    P = o.P
    kinds = {"one": [1] * len(xs), "pm1": [P - 1] * len(xs), "two": [2] * len(xs), "half": [(P + 1) // 2] * len(xs),
             "rand": [rng.randrange(1, P) for _ in xs]}
    xm1, solved = [], 0
    for x in xs:
        z = _sqrt(-pow(x, -1, P), P)
        solved += z is not None and z != 0
        xm1.append(z if z else rng.randrange(1, P))
    kinds["xm1"] = xm1
    assert solved > 0
    kinds["mixed"] = [kinds[k][i] for i, k in zip(range(len(xs)), ["pm1", "two", "half", "rand", "xm1"] * len(xs))]
    return kinds


def _jac_g1(o, a, zs):
    P = o.P
    out = np.zeros((len(a), 18), dtype=np.uint64)
    for i, (row, z) in enumerate(zip(a, zs)):
        x, y = o.limbs_to_fp(row[:6]), o.limbs_to_fp(row[6:12])
        z2 = z * z % P
        out[i, 0:6] = o.fp_to_limbs(x * z2 % P); out[i, 6:12] = o.fp_to_limbs(y * z2 * z % P); out[i, 12:18] = o.fp_to_limbs(z)
    return out


def _jac_g2(o, b, zs):
    """Z = (z, 0): X = x z^2, Y = y z^3 componentwise"""
    P = o.P
    out = np.zeros((len(b), 36), dtype=np.uint64)
    for i, (row, z) in enumerate(zip(b, zs)):
        z2, z3 = z * z % P, z * z * z % P
        for c, f in ((0, z2), (1, z2), (2, z3), (3, z3)):
            out[i, 6 * c:6 * c + 6] = o.fp_to_limbs(o.limbs_to_fp(row[6 * c:6 * c + 6]) * f % P)
        out[i, 24:30] = o.fp_to_limbs(z)
    return out


def test_jacobian_representation_invariance(curve):
    R, o = curve
    rng = random.Random(23)
    a, b, r = o.gen_g1(300, N), o.gen_g2(400, N), o.gen_scalars(5, N)
    s = o.gen_scalars(6, 1)[0]
    kinds_a = _z_choices(o, [o.limbs_to_fp(row[:6]) for row in a], rng)
    kinds_b = _z_choices(o, [o.limbs_to_fp(row[:6]) for row in b], rng)
    h = N // 2
    ref = None
    for kind in kinds_a:
        ja, jb = _jac_g1(o, a, kinds_a[kind]), _jac_g2(o, b, kinds_b[kind])
        if kind == "xm1":                                  # the lifted X really is p - 1 where the root exists
            assert any(o.limbs_to_fp(row[:6]) == o.P - 1 for row in ja) and any(o.limbs_to_fp(row[:6]) == o.P - 1 for row in jb)
        got = {
            "norm_g1": R.normalize_batch_g1(ja), "norm_g2": R.normalize_batch_g2(jb),
            "fold_g1": R.normalize_batch_g1(R.fold_g1(ja[:h], ja[h:], s)), "fold_g2": R.normalize_batch_g2(R.fold_g2(jb[:h], jb[h:], s)),
            "msm_g1": R.normalize_batch_g1(R.MultiexponentiationInnerProductG1.inner_product(ja, r)),
            "msm_g2": R.normalize_batch_g2(R.MultiexponentiationInnerProductG2.inner_product(jb, r)),
            "pairing": R.PairingInnerProduct.inner_product(ja, jb),
        }
        if ref is None:                                    # Z = 1 (the first kind): the inputs themselves, and the oracle's results
            assert kind == "one"
            ref = got
            assert np.array_equal(ref["norm_g1"], a) and np.array_equal(ref["norm_g2"], b)
            assert np.array_equal(ref["fold_g1"], o.normalize_g1(o.fold_g1_j(ja[:h], ja[h:], s)))
            assert np.array_equal(ref["fold_g2"], o.normalize_g2(o.fold_g2_j(jb[:h], jb[h:], s)))
            rc, m1 = o.msm_g1_j(ja, r); assert rc == 0 and np.array_equal(ref["msm_g1"], o.normalize_g1(m1.reshape(1, 18)))
            rc, m2 = o.msm_g2_j(jb, r); assert rc == 0 and np.array_equal(ref["msm_g2"], o.normalize_g2(m2.reshape(1, 36)))
            rc, pp = o.pairing_product_j(ja, jb); assert rc == 0 and np.array_equal(ref["pairing"], pp)
            continue
        for k in got:
            assert np.array_equal(got[k], ref[k]), (kind, k)
    # the oracle agrees on a lifted representation as well
    ja, jb = _jac_g1(o, a, kinds_a["mixed"]), _jac_g2(o, b, kinds_b["mixed"])
    rc, pp = o.pairing_product_j(ja, jb)
    assert rc == 0 and np.array_equal(pp, ref["pairing"])
