"""Inputs shared by tests/test_gipa_mexp_cpu.py and tests/test_gpu_gipa_mexp.py: the vectors of the reference's
multiexponentiation_inner_product_test (gipa.rs:499-530) as tests/test_gpu_gipa_generic.py draws them, and the edge case at n = 8."""
import numpy as np

INST = ("MEXP1", "AFGHO1", "PED1", "G1")
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF          # the GLV eigenvalue of BLS12-381's G1 (z^2 - 1): scalars are split as k = q * LAMBDA + rem on the device


def regular(orc, n):
    """-> m_a (n,18) projective, m_b (n,4), ck_a (n,24) affine, ck_b (n,12) affine"""
    return orc.blind_g1(orc.gen_g1(11, n), 1), orc.gen_scalars(5, n), orc.gen_g2(33, n), orc.gen_g1(44, n)


def edges(orc):
    """n = 8.  m_b: zero, one, r - 1, lambda (remainder 0), lambda + 1, 2^128 - 1 (every digit of the remainder at its maximum, quotient 0), 2^128, a random value.
    m_a: a repeated point in each half (the two meet in one bucket when their scalars share a digit: the exceptional additions of the gather) and the
    identity.  ck_b: a repeated point."""
    n = 8
    rnd = orc.limbs_to_fr(orc.gen_scalars(77, 1)[0])
    m_b = orc.fr_array([0, 1, orc.R - 1, LAMBDA, LAMBDA + 1, (1 << 128) - 1, 1 << 128, rnd])
    a = orc.gen_g1(11, n).copy(); a[1] = a[0]; a[5] = a[4]
    m_a = orc.blind_g1(a, 1)
    m_a[6] = orc.to_jac_g1(np.zeros((1, 12), dtype=np.uint64))[0]                        # the identity, (1, 1, 0)
    ck_b = orc.gen_g1(44, n).copy(); ck_b[3] = ck_b[2]
    return m_a, m_b, orc.gen_g2(33, n), ck_b


def model_prove(orc, m_a, m_b, ck_a, ck_b):
    """tests/model/gipa_generic_oracle.py on the same inputs -> (steps, transcript, base, ck_base, com): round order, scalars as integers"""
    import gipa_generic_oracle as M
    mb = [orc.limbs_to_fr(x) for x in m_b]
    ka, kb = orc.to_jac_g2(ck_a), orc.to_jac_g1(ck_b)
    steps, tr, base, ck_base = M.prove(INST, m_a, mb, ka, kb)
    com = [M.COMMIT["AFGHO1"][3](ka, m_a), M.COMMIT["PED1"][3](kb, mb), M.inner_product("MEXP1", m_a, mb)]
    return steps, tr, base, ck_base, com


def model_verify(orc, ck_a, ck_b, com, steps, base):
    import gipa_generic_oracle as M
    return M.verify(INST, orc.to_jac_g2(ck_a), orc.to_jac_g1(ck_b), com, steps, base)
