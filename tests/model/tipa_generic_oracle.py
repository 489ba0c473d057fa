"""CPU restatement of the GENERIC TIPA prover / verifier (ip_proofs/src/tipa/mod.rs:176-301) over the C oracle's primitives -- test infrastructure, the
checker for ripp_tipa_mexp_* and ripp_tipa_scalar_*.  The GIPA half is tests/model/gipa_generic_oracle.py (prove / the verifier's replay); the KZG half is
written here from mod.rs:186-223 (prover), 242-301 (verifier) and 304-422 (the key polynomial, its quotient and the two opening checks), with the
polynomial helpers of tests/model/tipa_model.py.  Scalars are Python integers, points the oracle's projective rows; small sizes only.

Instantiations are the tag tuples of gipa_generic_oracle with a G2 key on the left and a G1 key on the right:
    ("PAIR",  "AFGHO1", "AFGHO2", "GT")   pairing_inner_product_test             tipa/mod.rs:450-471
    ("MEXP1", "AFGHO1", "PED1",   "G1")   multiexponentiation_inner_product_test tipa/mod.rs:473-497
    ("SCAL",  "PED2",   "PED1",   "FR")   scalar_inner_product_test              tipa/mod.rs:499-526
"""
import hashlib

import numpy as np
import orclib as o

import gipa_generic_oracle as G
from tipa_model import ck_poly_coeffs, fr_from_random_bytes, kzg_quotient, poly_eval  # noqa: F401  (ck_poly_coeffs: what kzg_quotient divides)

R = o.R


def kzg_challenge(first, ck_a_final, ck_b_final):
    """mod.rs:194-209 / 257-272: nonce || r_transcript.first() || ck_a_final || ck_b_final -> Blake2b -> Fr::from_random_bytes"""
    nonce = 0
    while True:
        h = nonce.to_bytes(8, "big") + G.ser("FR", first) + G.ser("G2", ck_a_final) + G.ser("G1", ck_b_final)
        c = fr_from_random_bytes(hashlib.blake2b(h).digest())
        if c is not None:
            return c
        nonce += 1


def prove(inst, srs, m_a, m_b, ck_a, ck_b, r_shift=1):
    """TIPA::prove_with_srs_shift.  srs = (g_alpha_powers (2n-1,18), h_beta_powers (2n-1,36)); ck_a is the SHIFTED key when r_shift != 1.
    -> dict(steps, tr: ROUND order; base, final_ck, opening_a, opening_b, kzg_c)"""
    steps, tr, base, ck_base = G.prove(inst, m_a, m_b, ck_a, ck_b)
    rev = tr[::-1]; rev_inv = [pow(x, -1, R) for x in rev]                                   # r_transcript and its inverses, :190-191
    c = kzg_challenge(rev[0], ck_base[0], ck_base[1])
    qa = kzg_quotient(rev_inv, pow(r_shift, -1, R), c); qb = kzg_quotient(rev, 1, c)
    assert len(qa) == len(srs[1]) and len(qb) == len(srs[0])
    opening_a = o.msm_g2_j(np.ascontiguousarray(srs[1]), G.frs(qa))[1]                        # :212-217
    opening_b = o.msm_g1_j(np.ascontiguousarray(srs[0]), G.frs(qb))[1]                        # :218-223
    return dict(steps=steps, tr=tr, base=base, final_ck=ck_base, opening_a=opening_a, opening_b=opening_b, kzg_c=c)


def replay(inst, com, steps):
    """_compute_recursive_challenges (gipa.rs:322-363): -> (folded commitments, transcript in ROUND order)"""
    ip, lmc, rmc, t = inst
    outs = (G.COMMIT[lmc][2], G.COMMIT[rmc][2], t)
    cur = list(com); tr = []
    for com_1, com_2 in steps:
        c, c_inv = G.challenge(inst, tr[-1] if tr else None, com_1, com_2)
        cur = [G.plus(o_, G.plus(o_, G.scale(o_, x1, c), cu), G.scale(o_, x2, c_inv)) for o_, x1, cu, x2 in zip(outs, com_1, cur, com_2)]
        tr.append(c)
    return cur, tr


def _neg(tag, v): return G.scale(tag, v, R - 1)


def _gt_is_one(v): return np.array_equal(v, o.gt_one())


def verify(inst, v_srs, com, proof, r_shift=1):
    """TIPA::verify_with_srs_shift.  v_srs = (g, h, g_beta, h_alpha) projective; proof: dict of prove (steps in ROUND order)."""
    ip, lmc, rmc, t = inst
    g, h, g_beta, h_alpha = v_srs
    cur, tr = replay(inst, com, proof["steps"])
    rev = tr[::-1]; rev_inv = [pow(x, -1, R) for x in rev]
    ka, kb = proof["final_ck"]
    c = kzg_challenge(rev[0], ka, kb)
    # verify_commitment_key_g2_kzg_opening (:340-354): e(g, ck_a - h * eval) == e(g_beta - g * c, opening_a)
    ev = poly_eval(rev_inv, c, pow(r_shift, -1, R))
    l2 = G.plus("G2", ka, _neg("G2", G.scale("G2", h, ev))); r1 = G.plus("G1", g_beta, _neg("G1", G.scale("G1", g, c)))
    ok_a = _gt_is_one(o.pairing_product_j(np.stack([g, _neg("G1", r1)]), np.stack([l2, proof["opening_a"]]))[1])
    # verify_commitment_key_g1_kzg_opening (:356-370): e(ck_b - g * eval, h) == e(opening_b, h_alpha - h * c)
    ev = poly_eval(rev, c, 1)
    l1 = G.plus("G1", kb, _neg("G1", G.scale("G1", g, ev))); r2 = G.plus("G2", h_alpha, _neg("G2", G.scale("G2", h, c)))
    ok_b = _gt_is_one(o.pairing_product_j(np.stack([l1, _neg("G1", proof["opening_b"])]), np.stack([h, r2]))[1])
    # base check (:291-298)
    a_base, b_base = proof["base"]
    outs = (G.COMMIT[lmc][2], G.COMMIT[rmc][2], t)
    def wrap(tag, x): return [x] if tag == "FR" else x[None]
    ok = G.same(outs[0], G.COMMIT[lmc][3](ka[None], wrap(G.COMMIT[lmc][0], a_base)), cur[0])
    ok &= G.same(outs[1], G.COMMIT[rmc][3](kb[None], wrap(G.COMMIT[rmc][0], b_base)), cur[1])
    ok &= G.same(outs[2], G.inner_product(ip, wrap(G.IP_TYPES[ip][0], a_base), wrap(G.IP_TYPES[ip][1], b_base)), cur[2])
    return bool(ok_a and ok_b and ok)


def commit(inst, m_a, m_b, ck_a, ck_b):
    """(com_a, com_b, com_t) of the statement"""
    ip, lmc, rmc, t = inst
    return [G.COMMIT[lmc][3](ck_a, m_a), G.COMMIT[rmc][3](ck_b, m_b), G.inner_product(ip, m_a, m_b)]
