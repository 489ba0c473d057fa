"""Inputs shared by tests/test_tipa_generic_cpu.py and tests/test_gpu_tipa_generic.py: the statements of the reference's
multiexponentiation_inner_product_test and scalar_inner_product_test of TIPA (tipa/mod.rs:473-526), their shifted forms (mod.rs:545-561) and the edge
sets of the scalar-product prover at n = 8, with the model proofs (tests/model/tipa_generic_oracle.py) computed once per input set."""
import functools

import numpy as np

INST_PAIR = ("PAIR", "AFGHO1", "AFGHO2", "GT")
INST_MEXP = ("MEXP1", "AFGHO1", "PED1", "G1")
INST_SCAL = ("SCAL", "PED2", "PED1", "FR")
X_ABS = 0xD201000000010000                           # |x| of BLS12-381: G2 scalars are written in base |x| on the device (four 64-bit digits)
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF          # the GLV eigenvalue of G1: k = q * LAMBDA + rem on the device
SIZES_MEXP = (2, 4, 8, 16)
SIZES_SCAL = (2, 4, 8, 16, 64, 512)
SHIFT = 0x1D5A2F8B6C4E9071                           # the r_shift != 1 of the shifted statements
TRAPDOORS = {"one": (1, 1), "minus_one": (-1, -1)}   # (alpha, beta) of the two edge SRS sets, mod r: every power is +-generator


def srs(orc, n, alpha=None, beta=None):
    """(g_alpha_powers, h_beta_powers, g_beta, h_alpha) projective, 2n-1 powers (tests/helpers.py make_srs)"""
    import helpers as h
    return h.make_srs(n, (0x1234567 + n if alpha is None else alpha) % orc.R, (0x89ABCDEF + n if beta is None else beta) % orc.R, o=orc)


def keys(srs_):
    """(ck_a in G2, ck_b in G1): the even powers (tipa/mod.rs:114-118), projective"""
    import helpers as h
    return h.commitment_keys(srs_)


def mexp_messages(orc, n):
    return orc.blind_g1(orc.gen_g1(11, n), 1), orc.gen_scalars(5, n)


def scalar_messages(orc, n):
    return orc.gen_scalars(5, n), orc.gen_scalars(6, n)


def ints(orc, fr_rows):
    return [orc.limbs_to_fr(x) for x in fr_rows]


def shift_keys(orc, ck_a, r):
    """ck_a[i] * r^-i (tipa/mod.rs:545-553)"""
    return np.stack([orc.to_jac_g2(orc.g2_mul_a(orc.g2_to_affine(ck_a[i]), orc.fr_array([pow(r, -i, orc.R)])[0]))[0] for i in range(len(ck_a))])


def shift_points(orc, m_a, r):
    """m_a[i] * r^i for a G1 message (tipa/mod.rs:554-561)"""
    return np.stack([orc.to_jac_g1(orc.g1_mul_a(orc.g1_to_affine(m_a[i]), orc.fr_array([pow(r, i, orc.R)])[0]))[0] for i in range(len(m_a))])


def shift_scalars(orc, m_a, r):
    return orc.fr_array([v * pow(r, i, orc.R) % orc.R for i, v in enumerate(ints(orc, m_a))])


def scalar_edges(orc, which):
    """n = 8, integers.  which = 0: m_a holds the edges of the base-|x| split of the G2 digit pass -- zero, one, r - 1, |x| - 1 (quotient 0, the largest remainder),
    |x| (remainder 0), |x| + 1, |x|^2 and |x|^3 (one digit 1, all others 0) -- and m_b the lambda edges of the G1 digit pass (tests/gipa_mexp_inputs.py).
    which = 1: m_a holds 2^64 - 1 and 2^64 (just above |x|: quotient 1), |x|^4 - 1 reduced (every digit at its maximum) and values next to the first set; m_b
    holds the base-|x| edges, so both vectors meet them."""
    R, X = orc.R, X_ABS
    base_x = [0, 1, R - 1, X - 1, X, X + 1, X * X, X ** 3]
    lam = [0, 1, R - 1, LAMBDA, LAMBDA + 1, (1 << 128) - 1, 1 << 128, orc.limbs_to_fr(orc.gen_scalars(77, 1)[0])]
    if which == 0:
        return base_x, lam
    second = [(1 << 64) - 1, 1 << 64, (X - 1) * (1 + X + X * X), X * X - 1, X ** 3 + X - 1, R - 2, 0, (1 << 128) + (1 << 64)]
    return second, base_x[::-1]


# ---- model proofs, once per input set -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mexp_case(n, shift=1):
    """-> dict(srs, m_a, m_b, ck_a (shifted), ck_b, com, model): the statement of length n and the model's proof of it"""
    import orclib as orc
    import tipa_generic_oracle as T
    s = srs(orc, n); ck_a, ck_b = keys(s); m_a, m_b = mexp_messages(orc, n)
    if shift != 1:
        ck_a, m_a = shift_keys(orc, ck_a, shift), shift_points(orc, m_a, shift)
    mb = ints(orc, m_b)
    return dict(srs=s, m_a=m_a, m_b=m_b, ck_a=ck_a, ck_b=ck_b, com=T.commit(INST_MEXP, m_a, mb, ck_a, ck_b),
                model=T.prove(INST_MEXP, s, m_a, mb, ck_a, ck_b, shift))


def _scalar(orc, s, ma, mb, shift):
    import tipa_generic_oracle as T
    ck_a, ck_b = keys(s)
    if shift != 1:
        ck_a = shift_keys(orc, ck_a, shift); ma = [v * pow(shift, i, orc.R) % orc.R for i, v in enumerate(ma)]
    return dict(srs=s, m_a=orc.fr_array(ma), m_b=orc.fr_array(mb), ck_a=ck_a, ck_b=ck_b, com=T.commit(INST_SCAL, ma, mb, ck_a, ck_b),
                model=T.prove(INST_SCAL, s, ma, mb, ck_a, ck_b, shift))


@functools.lru_cache(maxsize=None)
def scalar_case(n, shift=1):
    import orclib as orc
    m_a, m_b = scalar_messages(orc, n)
    return _scalar(orc, srs(orc, n), ints(orc, m_a), ints(orc, m_b), shift)


@functools.lru_cache(maxsize=None)
def scalar_edge_case(trapdoors, which):
    import orclib as orc
    alpha, beta = TRAPDOORS[trapdoors]
    return _scalar(orc, srs(orc, 8, alpha, beta), *scalar_edges(orc, which), 1)


def verifier_srs(case):
    import helpers as h
    return h.verifier_srs(case["srs"])
