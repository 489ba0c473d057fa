"""CPU: the reference and the point sets of tests/miller_edges.py, before tests/test_gpu_miller_edges.py holds the stage-1 kernels against them.
The step-by-step reference lines, combined by the recurrence of miller_combine and exponentiated, must give the pairing of the independent model
(affine slopes, untwisted lines) and the oracle's value; the edge points must be curve points with usable chains; the comparison rule must reject what
it is there to reject."""
import random

import numpy as np
import pytest

import miller_edges as E

CURVES = ["381", "377"]


def _orc(tag):
    if tag == "381":
        import orclib as o
    else:
        import orclib377 as o
    o.lib()
    return o


@pytest.mark.parametrize("tag", CURVES)
def test_reference_lines_give_the_model_pairing(tag):
    C = E.CURVES[tag]
    ps, qs = E.subgroup_points(tag, 6)
    for Pt, Q in ((ps[0], qs[0]), (ps[5], qs[2])):
        lines = E.ref_lines(tag, Pt, Q)
        assert len(lines) == C.n_lines
        assert C.m.final_exponentiation(E.combine(C, lines)) == E.model_pairing(tag, Pt, Q)


@pytest.mark.parametrize("tag", CURVES)
def test_reference_lines_give_the_oracle_value(tag):
    """sets (a) and (b): the oracle's Miller value and the combined reference lines agree after the oracle's final exponentiation, also for the edge
    points outside the prime-order subgroups"""
    o, C = _orc(tag), E.CURVES[tag]
    ps, qs = E.subgroup_points(tag, 4)
    eg1, (eg2, _) = E.edge_g1(tag), E.edge_g2(tag)
    pairs = list(zip(ps, qs)) + [(Pt, Q) for Pt in eg1 for Q in eg2] + [(ps[1], Q) for Q in eg2] + [(Pt, qs[1]) for Pt in eg1]
    for Pt, Q in pairs:
        ours = o.final_exp(o.gt_from_model(E.combine(C, E.ref_lines(tag, Pt, Q))))
        theirs = o.final_exp(o.miller_product_a(o.g1_array([Pt]), o.g2_array([Q])))
        assert np.array_equal(ours, theirs), (tag, Pt, Q)


@pytest.mark.parametrize("tag", CURVES)
def test_reference_steps_are_vmgen_s_formulas_up_to_scale(tag):
    from vm_model import vmgen
    C = E.CURVES[tag]
    ps, qs = E.subgroup_points(tag, 3)
    Pt, Q = ps[2], qs[1]
    T = (Q[0], Q[1], (1, 0))
    six = lambda d: (d["L0"][0], d["L0"][1], d["L1"][0], d["L1"][1], d["L2"][0], d["L2"][1])
    ours = E.ref_lines(tag, Pt, Q)
    vmgen.set_curve("bls12_" + tag)
    try:
        d = vmgen.ref_line_double(T[0], T[1], T[2], Pt[0], Pt[1])
        assert E.scale_equal(C.P, six(d), ours[0])
        s = 0
        for bit in C.bits:                                                 # walk to the first addition step
            T, _ = E.step_double(C, T); s += 1
            if bit == "1": break
        a = vmgen.ref_line_add(T[0], T[1], T[2], Q[0], Q[1], Pt[0], Pt[1])
        assert E.scale_equal(C.P, six(a), ours[s])
    finally:
        vmgen.set_curve("bls12_381")


@pytest.mark.parametrize("tag", CURVES)
def test_edge_points(tag):
    C = E.CURVES[tag]
    eg1, (eg2, skipped) = E.edge_g1(tag), E.edge_g2(tag)
    assert len(eg1) >= 4 and len(set(eg1)) == len(eg1) and len(eg2) >= 4 and len(set(eg2)) == len(eg2), (len(eg1), len(eg2), skipped)
    for Pt in eg1:
        assert E.g1_on_curve(C, Pt) and 0 <= Pt[0] < C.P and 0 <= Pt[1] < C.P and Pt != (0, 0)
    assert any(Pt[0] == 0 for Pt in eg1) and any(Pt[0] >= C.P - 3 for Pt in eg1)
    for Q in eg2:
        assert E.g2_on_curve(C, Q) and Q != ((0, 0), (0, 0)) and not E.chain(tag, Q)[1]
    assert any(Q[0][1] == 0 and Q[0][0] < E.EDGE_SEARCH for Q in eg2) and any(Q[0][0] == Q[0][1] >= C.P - 1 - E.EDGE_SEARCH for Q in eg2)
    # the square roots the search rests on
    rng = random.Random(5)
    for _ in range(8):
        r = (rng.randrange(C.P), rng.randrange(C.P))
        s = E.f2_sqrt(C, C.m.f2mul(r, r))
        assert s in (r, C.m.f2neg(r))
        x = rng.randrange(C.P)
        assert E.fp_sqrt(C.P, x * x) in (x, C.P - x)


@pytest.mark.parametrize("tag", CURVES)
def test_chain_flags_a_degenerate_point(tag):
    """Y = 0 (a 2-torsion point's shape; the formulas do not ask for a curve point) reaches Z = 0 in its first doubling"""
    assert E.chain(tag, ((5, 7), (0, 0)))[1]                               # Y = 0: b = 0, Z3 = b h = 0


@pytest.mark.parametrize("tag", CURVES)
def test_scale_rule(tag):
    C = E.CURVES[tag]
    P = C.P
    ps, qs = E.subgroup_points(tag, 2)
    ref = E.ref_lines(tag, ps[0], qs[1])[3]
    k = 0xC0FFEE
    assert E.scale_equal(P, tuple(v * k % P for v in ref), ref) and E.scale_equal(P, ref, ref)
    assert E.scale_equal(P, tuple(v * (P - 1) % P * 256 % P for v in ref), ref)                       # -2^8, as k_miller_lines_q scales an addition line
    assert not E.scale_equal(P, tuple([0] * 6), ref)
    for i in range(6):
        bad = list(v * k % P for v in ref); bad[i] = (bad[i] + 1) % P
        assert not E.scale_equal(P, bad, ref), i
    z = (3, 5)                                                                                        # an Fp2 factor outside Fp
    pairs = [C.m.f2mul((ref[2 * j], ref[2 * j + 1]), z) for j in range(3)]
    assert not E.scale_equal(P, tuple(c for pr in pairs for c in pr), ref)
    assert E.decode(C, C.one_m) == 1 and E.unit_words(tag)[12:] == [0] * 60
