"""GPU parity (-m gpu): the native transparent polynomial commitments (`ripp_tpc_*`, `ripp_gipa_ssm_*`; ripp_amd/poly_commit/native.py `transparent`) against
the CPU oracle (tests/model/gipa_generic_oracle.py, tests/model/poly_commit_oracle.py) and the package's Python path (ripp_amd/poly_commit/transparent.py).
Group elements are compared after normalisation, GT and Fr values byte for byte; these are exact values, nothing is tolerated.

The timing condition at the end (native commit / open / verify against the Python path's at degree 65 535, same process, same device, medians of 5 after a
warm-up) is a condition on where the work runs, not a tuned number."""
import ctypes
import os
import random
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "model"))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P(engine):
    import ripp_amd.poly_commit as pc
    return pc


@pytest.fixture(scope="module")
def T(engine):
    from ripp_amd.poly_commit import native
    return native.transparent


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _same_g1(orc, a, b):
    a, b = np.asarray(a).reshape(-1, 18), np.asarray(b).reshape(-1, 18)
    return np.array_equal(orc.normalize_g1(np.ascontiguousarray(a)), orc.normalize_g1(np.ascontiguousarray(b)))


def _ints(orc, limbs):
    """(n, 4) Montgomery limbs -> integers"""
    rinv = pow(1 << 256, -1, orc.R)
    raw = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") * rinv % orc.R for i in range(len(raw) // 32)]


def _int(orc, limbs):
    return _ints(orc, limbs)[0]


def _horner(orc, coeffs, z):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % orc.R
    return acc


def _eq(orc, tag, got, exp):
    """one proof member: tag GT (bytes), G1 (normalised), FR (integer; either side limbs or an integer)"""
    if tag == "FR":
        g = got if isinstance(got, int) else _int(orc, got); e = exp if isinstance(exp, int) else _int(orc, exp)
        return g % orc.R == e % orc.R
    if tag == "G1":
        return _same_g1(orc, got, exp)
    return np.array_equal(np.asarray(got).reshape(-1), np.asarray(exp).reshape(-1))


def _cmp_model(orc, left, inner, base_a, proof, tr, model):
    """native GIPAProof dict (+ transcript in round order) against the oracle's (steps, transcript, base, ck_base), every member"""
    steps, etr, base, _ = model
    got = proof["r_commitment_steps"][::-1]
    assert len(got) == len(steps) == len(tr)
    for k in range(len(steps)):
        for side in range(2):
            assert _eq(orc, left, got[k][side][0], steps[k][side][0]), (k, side, "commitment")
            assert not np.asarray(got[k][side][1]).any()
            assert _eq(orc, inner, got[k][side][2][0], steps[k][side][2]), (k, side, "inner product")
        assert _int(orc, tr[k]) == etr[k], (k, "transcript")
    assert _eq(orc, base_a, proof["r_base"][0], base[0]) and _eq(orc, "FR", proof["r_base"][1], base[1])


def _cmp_dicts(orc, left, inner, base_a, got, exp):
    """two GIPAProof dicts of the shape of ripp_amd.gipa (native against the Python path), every member"""
    assert len(got["r_commitment_steps"]) == len(exp["r_commitment_steps"])
    for g, e in zip(got["r_commitment_steps"], exp["r_commitment_steps"]):
        for side in range(2):
            assert _eq(orc, left, g[side][0], e[side][0]) and _eq(orc, inner, g[side][2][0], e[side][2][0])
    assert _eq(orc, base_a, got["r_base"][0], exp["r_base"][0]) and _eq(orc, "FR", got["r_base"][1], exp["r_base"][1])


def _altered(proof, step=0, side=0, member=0):
    """a copy of a GIPAProof dict with one step member replaced by the one of the other side"""
    steps = [tuple(tuple(x for x in s) for s in st) for st in proof["r_commitment_steps"]]
    st = [list(s) for s in steps[step]]
    if member == 0:
        st[side][0] = steps[step][1 - side][0]
    else:
        st[side][2] = steps[step][1 - side][2]
    steps[step] = tuple(tuple(s) for s in st)
    return {"r_commitment_steps": steps, "r_base": proof["r_base"]}


# ---------------------------------------------------------------------------------------------------------------- keys
def test_keys_and_memory(engine, orc, P, T):
    """setup gives the keys of the Python path's setup, ck_create from the downloaded keys commits to the same value, destroy returns the memory"""
    from ripp_amd._lib import lib
    PT = P.transparent.BivariatePolynomialCommitment
    x_degree, y_degree = 3, 15
    # one opening first: the engine's flag word of the VM folds (4 bytes) is allocated by the first fold of a process and lives until ripp_shutdown
    warm = T.CK.setup(1, 2, 1, 1); z = engine.synth_fr(8, 2)
    T.BivariatePolynomialCommitment.open(warm, z.reshape(1, 2, 4), T.BivariatePolynomialCommitment.commit(warm, z.reshape(1, 2, 4))[1], (z[0], z[1]))
    engine.release_scratch()
    before = engine.device_bytes()

    def live():
        """handles alive, from the refusal of ripp_init(another ordinal): it names their number and touches nothing while there is one (`warm` stays alive for this)"""
        assert lib().ripp_init(ctypes.c_int32(engine.device_count() + 7)) == 4
        msg = lib().ripp_last_error().decode(); assert "alive" in msg, msg
        return int(msg.split("ripp_init: ")[1].split()[0])

    live0 = live()
    ck = T.CK.setup(700, 900, x_degree, y_degree)
    assert live() == live0 + 1
    assert engine.device_bytes() > before
    assert ck.degrees() == (x_degree, y_degree)
    k1, k2 = ck.keys(); pck = PT.setup(700, 900, x_degree, y_degree)
    assert np.array_equal(k1, pck[0][:, :12]) and np.array_equal(k2, pck[1][:, :24])
    assert np.array_equal(k1, engine.synth_g1(700, y_degree + 1)) and np.array_equal(k2, engine.synth_g2(900, x_degree + 1))
    coeffs = engine.synth_fr(3, (x_degree + 1) * (y_degree + 1)).reshape(x_degree + 1, y_degree + 1, 4)
    com, coms = T.BivariatePolynomialCommitment.commit(ck, coeffs)
    ck2 = T.CK.create(k1, k2)
    com2, coms2 = T.BivariatePolynomialCommitment.commit(ck2, coeffs)
    assert np.array_equal(com, com2) and _same_g1(orc, coms, coms2)
    with pytest.raises(ValueError):
        T.BivariatePolynomialCommitment.commit(ck, np.zeros((x_degree + 2, y_degree + 1, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        T.BivariatePolynomialCommitment.commit(ck, np.zeros((1, y_degree + 2, 4), dtype=np.uint64))
    with pytest.raises(AssertionError):
        T.CK.setup(700, 900, 2, 15)
    proof, _ = T.BivariatePolynomialCommitment.open(ck, coeffs, coms, (engine.synth_fr(8, 1)[0], engine.synth_fr(9, 1)[0]))
    assert live() == live0 + 2
    ck.close(); ck2.close(); engine.release_scratch()
    assert engine.device_bytes() == before and live() == live0
    warm.close()
    assert engine.device_bytes() < before


# ---------------------------------------------------------------------------------------------------------------- the tier provers
def _neg_g1_affine(orc, a):
    import gipa_generic_oracle as M
    return orc.g1_to_affine(M.scale("G1", orc.to_jac_g1(a)[0], orc.R - 1))


def _first_tier_case(engine, orc, n, variant):
    rng = random.Random(1000 * n + sum(map(ord, variant)))
    m = [rng.randrange(orc.R) for _ in range(n)]
    s = rng.randrange(2, orc.R)
    ck = engine.synth_g1(4242 + n, n)
    if variant == "zero":
        m = [0] * n                                            # identity commitments, zero products
    elif variant == "last":
        m = [0] * (n - 1) + [orc.R - 1]
    elif variant == "b0":
        s = 0                                                  # b = (1, 0, 0, ..)
    elif variant == "b1":
        s = 1
    elif variant == "keys":                                    # the MSM's exceptional additions: P + (-P) and P + P inside one bucket
        ck[1] = _neg_g1_affine(orc, ck[0])
        if n >= 4:
            ck[3] = ck[2]
        m = [m[0]] * n                                         # equal scalars, so that the equal / opposite keys meet in one bucket
    b = [pow(s, i, orc.R) for i in range(n)]
    return m, b, s, ck


@pytest.mark.parametrize("variant", ["random", "zero", "last", "b0", "b1", "keys"])
@pytest.mark.parametrize("n", [2, 4, 64, 512])
def test_first_tier_against_the_oracle(engine, orc, P, T, n, variant):
    """GIPAWithSSM<ScalarInnerProduct, PedersenCommitment<G1>, IdentityCommitment<Fr>> (transparent.rs:43-48) against prove(FIRST_TIER, ..)"""
    import gipa_generic_oracle as M
    import poly_commit_oracle as PC
    m, b, s, ck = _first_tier_case(engine, orc, n, variant)
    ckj = orc.to_jac_g1(ck)
    proof, tr = T.scalar_prove(P.frs(m), P.frs(b), ck)
    model = M.prove(PC.FIRST_TIER, m, b, ckj, [None] * n)
    _cmp_model(orc, "G1", "FR", "FR", proof, tr, model)
    if variant == "zero":
        assert all(not orc.normalize_g1(np.ascontiguousarray(side[0]).reshape(1, 18)).any() and _int(orc, side[2][0]) == 0
                   for st in proof["r_commitment_steps"] for side in st)
    com = (M.COMMIT["PED1"][3](ckj, m), M.inner_product("SCAL", m, b))
    fcom = (com[0], P.frs([com[1]])[0]); fs = P.frs([s])[0]
    assert T.scalar_verify(ck, fcom, fs, proof)
    if n <= 64:
        steps = [tuple((np.asarray(side[0]), 0, _int(orc, side[2][0])) for side in st) for st in proof["r_commitment_steps"][::-1]]
        assert M.verify(PC.FIRST_TIER, ckj, [None] * n, [com[0], 0, com[1]], steps, (_int(orc, proof["r_base"][0]), _int(orc, proof["r_base"][1])), scalar_b=s)
    # rejections: a changed step (commitment and inner product), a changed base, a changed commitment; with a non-zero message also a changed scalar_b and a
    # changed r_base.1 (the all-zero message has a_base = 0, and 0 * b = 0 for every b)
    last = len(proof["r_commitment_steps"]) - 1
    moved = [tuple((M.plus("G1", np.asarray(side[0]), ckj[0]) if (i, j) == (0, 0) else side[0], side[1], side[2]) for j, side in enumerate(st))
             for i, st in enumerate(proof["r_commitment_steps"])]
    bumped = [tuple((side[0], side[1], [P.frs([_int(orc, side[2][0]) + 1])[0]] if (i, j) == (last, 1) else side[2]) for j, side in enumerate(st))
              for i, st in enumerate(proof["r_commitment_steps"])]
    assert not T.scalar_verify(ck, fcom, fs, dict(proof, r_commitment_steps=moved))
    assert not T.scalar_verify(ck, fcom, fs, dict(proof, r_commitment_steps=bumped))
    a_base, b_base = proof["r_base"]
    assert not T.scalar_verify(ck, fcom, fs, dict(proof, r_base=(P.frs([_int(orc, a_base) + 1])[0], b_base)))
    assert not T.scalar_verify(ck, (fcom[0], P.frs([com[1] + 1])[0]), fs, proof)
    if variant != "zero":
        assert not T.scalar_verify(ck, fcom, P.frs([s + 1])[0], proof)
        assert not T.scalar_verify(ck, fcom, fs, dict(proof, r_base=(a_base, P.frs([_int(orc, b_base) + 1])[0])))


@pytest.mark.parametrize("n", [2, 4, 512])
def test_first_tier_forms_agree(engine, orc, P, T, monkeypatch, n):
    """the crossed two-row commitments and the two single MSMs give the same proof at every round length (down to the degenerate 2 and 4), as do the
    legacy MSM switches and RIPP_NO_MSM_BATCH, which select the two single MSMs whatever the bound says"""
    m, b, s, ck = _first_tier_case(engine, orc, n, "random")
    fm, fb = P.frs(m), P.frs(b)
    monkeypatch.setenv("RIPP_TPC_CROSS_MIN", "2")
    crossed, tr = T.scalar_prove(fm, fb, ck)
    assert len(T.round_ms()) == n.bit_length() - 1
    monkeypatch.setenv("RIPP_TPC_CROSS_MIN", str(1 << 40))
    single, tr2 = T.scalar_prove(fm, fb, ck)
    monkeypatch.setenv("RIPP_TPC_CROSS_MIN", "64")
    mixed, tr3 = T.scalar_prove(fm, fb, ck)
    assert np.array_equal(tr, tr2) and np.array_equal(tr, tr3)
    _cmp_dicts(orc, "G1", "FR", "FR", crossed, single); _cmp_dicts(orc, "G1", "FR", "FR", crossed, mixed)
    monkeypatch.setenv("RIPP_TPC_CROSS_MIN", "2")                                           # the legacy forms win over the bound
    monkeypatch.setenv("RIPP_NO_MSM_BATCH", "1")
    nobatch, tr5 = T.scalar_prove(fm, fb, ck)
    monkeypatch.delenv("RIPP_NO_MSM_BATCH")
    assert np.array_equal(tr, tr5)
    _cmp_dicts(orc, "G1", "FR", "FR", crossed, nobatch)
    for switch in ("no_msm_glv", "no_fq", "no_vm"):
        try:
            engine.configure(**{switch: 1})
            legacy, tr4 = T.scalar_prove(fm, fb, ck)
        finally:
            engine.configure()
        assert np.array_equal(tr, tr4), switch
        _cmp_dicts(orc, "G1", "FR", "FR", crossed, legacy)
    monkeypatch.delenv("RIPP_TPC_CROSS_MIN")
    default, tr6 = T.scalar_prove(fm, fb, ck)
    assert np.array_equal(tr, tr6)
    _cmp_dicts(orc, "G1", "FR", "FR", crossed, default)


@pytest.mark.parametrize("variant", ["random", "infinity"])
@pytest.mark.parametrize("n", [2, 4, 32])
def test_second_tier_against_the_oracle(engine, orc, P, T, n, variant):
    """GIPAWithSSM<MultiexponentiationInnerProduct<G1>, AFGHOCommitmentG1, IdentityCommitment<G1>> (transparent.rs:28-33) against prove(SECOND_TIER, ..)"""
    import gipa_generic_oracle as M
    import poly_commit_oracle as PC
    rng = random.Random(77 * n + len(variant))
    msg = orc.to_jac_g1(engine.synth_g1(31 + n, n))
    if variant == "infinity":
        msg[0] = 0
        if n > 2:
            msg[n - 1] = 0
    s = rng.randrange(2, orc.R); b = [pow(s, i, orc.R) for i in range(n)]
    ck = engine.synth_g2(555 + n, n); ckj = orc.to_jac_g2(ck)
    proof, tr = T.mexp_prove(msg, P.frs(b), ck)
    model = M.prove(PC.SECOND_TIER, msg, b, ckj, [None] * n)
    _cmp_model(orc, "GT", "G1", "G1", proof, tr, model)
    com = (M.COMMIT["AFGHO1"][3](ckj, msg), M.inner_product("MEXP1", msg, b)); fs = P.frs([s])[0]
    assert T.mexp_verify(ck, com, fs, proof)
    steps = [tuple((np.asarray(side[0]), 0, np.asarray(side[2][0])) for side in st) for st in proof["r_commitment_steps"][::-1]]
    assert M.verify(PC.SECOND_TIER, ckj, [None] * n, [com[0], 0, com[1]], steps, (np.asarray(proof["r_base"][0]), _int(orc, proof["r_base"][1])), scalar_b=s)
    assert not T.mexp_verify(ck, com, P.frs([s + 1])[0], proof)
    assert not T.mexp_verify(ck, com, fs, _altered(proof, step=0, side=0, member=0))
    assert not T.mexp_verify(ck, com, fs, _altered(proof, step=len(steps) - 1, side=1, member=1))
    a_base, b_base = proof["r_base"]
    assert not T.mexp_verify(ck, com, fs, dict(proof, r_base=(a_base, P.frs([_int(orc, b_base) + 1])[0])))
    assert not T.mexp_verify(ck, com, fs, dict(proof, r_base=(orc.to_jac_g1(engine.synth_g1(5, 1))[0], b_base)))
    assert not T.mexp_verify(ck, (com[0], orc.to_jac_g1(engine.synth_g1(6, 1))[0]), fs, proof)


def _in_cyclotomic(orc, gt):
    """x^(p^4 - p^2 + 1) == 1 for a (72,) limb GT value, in the big-integer model (tests/model/bls381_model.py)"""
    import bls381_model as M
    import tipa_model as TM
    x = TM.gt_from_tower([orc.limbs_to_fp(gt[6 * i:6 * i + 6]) for i in range(12)])
    return M.f12pow(x, M.P ** 4 - M.P ** 2 + 1) == M.F12_ONE


@pytest.mark.parametrize("n", [2, 4])
def test_second_tier_rounds_are_one_function_for_both_callers(engine, orc, P, T, n):
    """ripp_gipa_ssm_mexp_prove (the transparent scheme's second tier) and ripp_tipa_ssm_prove (TIPAWithSSM) run the same rounds on the same loaded message: on one
    message, one structured scalar vector and one G2 key (the even powers of an SRS of 2 n - 1 powers, as ripp_amd.api builds for TIPAWithSSM) they return identical
    com_gt, com_g1, transcript, base_a and base_b bytes, n = 2 (one round, no previous challenge) and n = 4 (the chained challenge).  Both verifiers replay the
    transcript with one function: both accept, and both reject a GT step member outside the cyclotomic subgroup."""
    import helpers as h
    osrs = h.make_srs(n, 0x5eed + n, 0xfeed + n); srs = engine.SRS(osrs[0], osrs[1])
    ck_j, _ = h.commitment_keys(osrs); ck = engine.normalize_batch_g2(ck_j)
    msg = orc.blind_g1(orc.gen_g1(13, n), 3)
    s = 0x5eed5eed5eed5eed5eed5eed5eed5eed5eed % orc.R; fs = P.frs([s])[0]
    b = P.frs([pow(s, i, orc.R) for i in range(n)])
    proof, tr = T.mexp_prove(msg, b, ck)
    tipa = engine.TIPAWithSSM.prove_with_structured_scalar_message(srs, (msg, b), (ck_j,))
    steps = proof["r_commitment_steps"][::-1]                                              # ROUND order, as the TIPAWithSSM arrays
    gt = np.stack([side[0] for st in steps for side in st]); g1 = np.stack([side[2][0] for st in steps for side in st])
    assert len(tr) == n.bit_length() - 1
    assert gt.tobytes() == tipa["com_gt"].tobytes() and g1.tobytes() == tipa["com_g1"].tobytes() and tr.tobytes() == tipa["tr"].tobytes()
    assert np.asarray(proof["r_base"][0]).tobytes() == tipa["base_a"].tobytes() and np.asarray(proof["r_base"][1]).tobytes() == tipa["base_b"].tobytes()
    com = (engine.AFGHOCommitmentG1.commit(ck_j, msg), engine.MultiexponentiationInnerProductG1.inner_product(msg, b))
    g, hh, g_beta, _ = h.verifier_srs(osrs); vk = {"g": g, "h": hh, "g_beta": g_beta, "h_alpha": osrs[3]}
    assert T.mexp_verify(ck, com, fs, proof)
    assert engine.TIPAWithSSM.verify_with_structured_scalar_message(vk, com, fs, tipa)
    # a GT member with one limb incremented: the model shows that it has left the cyclotomic subgroup (and that the honest member is in it)
    k = 2 * len(steps) - 1
    off = tipa["com_gt"].copy(); off[k, 0] += np.uint64(1)
    assert _in_cyclotomic(orc, tipa["com_gt"][k]) and not _in_cyclotomic(orc, off[k])
    assert not engine.TIPAWithSSM.verify_with_structured_scalar_message(vk, com, fs, dict(tipa, com_gt=off))
    zero = np.zeros(4, dtype=np.uint64)
    bad = [((off[2 * r], zero, [g1[2 * r]]), (off[2 * r + 1], zero, [g1[2 * r + 1]])) for r in range(len(steps))][::-1]
    assert not T.mexp_verify(ck, com, fs, {"r_commitment_steps": bad, "r_base": proof["r_base"]})
    srs.close()


# ---------------------------------------------------------------------------------------------------------------- bivariate
def _cmp_opening(orc, proof, eproof):
    """native opening against the oracle's tr_open, every member"""
    assert _same_g1(orc, proof["y_eval_comm"], eproof["y_eval_comm"])
    _cmp_model(orc, "GT", "G1", "G1", proof["second_tier_ip_proof"], proof["second_tier_transcript"], eproof["second"])
    _cmp_model(orc, "G1", "FR", "FR", proof["first_tier_ip_proof"], proof["first_tier_transcript"], eproof["first"])


def _cmp_python(orc, proof, pproof):
    """native opening against the Python path's, every member"""
    assert _same_g1(orc, proof["y_eval_comm"], pproof["y_eval_comm"])
    _cmp_dicts(orc, "GT", "G1", "G1", proof["second_tier_ip_proof"], pproof["second_tier_ip_proof"])
    _cmp_dicts(orc, "G1", "FR", "FR", proof["first_tier_ip_proof"], pproof["first_tier_ip_proof"])


def _py_ck(orc, ck):
    k1, k2 = ck.keys()
    return orc.to_jac_g1(k1), orc.to_jac_g2(k2)


@pytest.mark.parametrize("x_degree,y_degree,rows,cols", [(1, 1, 2, 2), (1, 3, 2, 4), (7, 7, 8, 8), (3, 15, 3, 11), (1, 1023, 2, 1000)])
def test_bivariate_against_the_oracle(engine, orc, P, T, x_degree, y_degree, rows, cols):
    """transparent.rs:86-212 against tr_commit / tr_open / tr_verify; rows < x_degree + 1 and cols < y_degree + 1 exercise the zero padding"""
    import poly_commit_oracle as PC
    B = T.BivariatePolynomialCommitment; PB = P.transparent.BivariatePolynomialCommitment
    rng = random.Random(x_degree * 1000 + y_degree)
    ck = B.setup(700, 900, x_degree, y_degree); pck = _py_ck(orc, ck)
    ys = [[rng.randrange(orc.R) for _ in range(cols)] for _ in range(rows)]
    coeffs = np.stack([P.frs(r) for r in ys])
    com, coms = B.commit(ck, coeffs); ecom, ecoms = PC.tr_commit(pck[0], pck[1], ys)
    assert np.array_equal(com, ecom) and _same_g1(orc, coms, ecoms)
    if (x_degree, y_degree) == (3, 15):                                                    # stride > cols: the tail of every row is never read
        wide = np.zeros((rows, cols + 5, 4), dtype=np.uint64); wide[:, :cols] = coeffs; wide[:, cols:] = 0xABCDEF
        coeffs = wide[:, :cols]
        com2, coms2 = B.commit(ck, coeffs); assert np.array_equal(com2, com) and _same_g1(orc, coms2, coms)
    point = (rng.randrange(orc.R), rng.randrange(orc.R)); fpoint = (P.frs([point[0]])[0], P.frs([point[1]])[0])
    proof, val = B.open(ck, coeffs, coms, fpoint); eproof = PC.tr_open(pck[0], pck[1], ys, ecoms, point)
    _cmp_opening(orc, proof, eproof)
    ival = _int(orc, val)
    assert ival == P.BivariatePolynomial(ys).evaluate(point) == PC.bi_evaluate(ys, point)
    assert B.verify(ck, com, fpoint, val, proof)
    assert PB.verify(pck, com, point, ival, proof)                                          # the Python-path verifier accepts the native proof
    pproof = PB.open(pck, P.BivariatePolynomial(ys), coms, point)
    _cmp_python(orc, proof, pproof)
    assert B.verify(ck, com, fpoint, val, pproof)                                           # and the native verifier the Python path's
    if y_degree <= 15:
        oproof = dict(second=(eproof["second"][0], None, eproof["second"][2], None), y_eval_comm=proof["y_eval_comm"], first=(eproof["first"][0], None, eproof["first"][2], None))
        assert PC.tr_verify(pck[0], pck[1], com, point, ival, oproof)
    assert not B.verify(ck, com, fpoint, P.frs([ival + 1])[0], proof)
    assert not B.verify(ck, com, (P.frs([point[0] + 1])[0], fpoint[1]), val, proof)
    assert not B.verify(ck, com, (fpoint[0], P.frs([point[1] + 1])[0]), val, proof)
    assert not B.verify(ck, com, fpoint, val, dict(proof, second_tier_ip_proof=_altered(proof["second_tier_ip_proof"], 0, 0, 0)))
    assert not B.verify(ck, com, fpoint, val, dict(proof, first_tier_ip_proof=_altered(proof["first_tier_ip_proof"], 0, 1, 1)))
    ck.close()


# ---------------------------------------------------------------------------------------------------------------- univariate
@pytest.mark.parametrize("degree", [3, 15, 56, 255, 1023])
def test_univariate_against_the_oracle(engine, orc, P, T, degree):
    import poly_commit_oracle as PC
    U = T.UnivariatePolynomialCommitment; PU = P.transparent.UnivariatePolynomialCommitment
    rng = random.Random(degree)
    xd, yd = U.bivariate_degrees(degree); assert (xd, yd) == PU.bivariate_degrees(degree)
    ck = U.setup(700, 900, degree); pck = _py_ck(orc, ck)
    assert ck.degrees() == (xd, yd)
    p = [rng.randrange(orc.R) for _ in range(degree + 1)]; c = P.frs(p)
    com, coms = U.commit(ck, c)
    z = rng.randrange(orc.R); fz = P.frs([z])[0]
    proof, val = U.open(ck, c, coms, fz)
    ival = _int(orc, val); assert ival == PC.horner(p, z)
    ys = PC.split(p, xd, yd); ecom, ecoms = PC.tr_commit(pck[0], pck[1], ys)
    assert np.array_equal(com, ecom) and _same_g1(orc, coms, ecoms)
    _cmp_opening(orc, proof, PC.tr_open(pck[0], pck[1], ys, ecoms, (pow(z, yd + 1, orc.R), z)))
    assert U.verify(ck, com, fz, val, proof) and not U.verify(ck, com, fz, P.frs([ival + 1])[0], proof)
    assert PU.verify(pck, com, z, ival, proof)
    com0, _ = U.commit(ck, np.concatenate([c, np.zeros((9, 4), dtype=np.uint64)])); assert np.array_equal(com0, com)      # trailing zeros are stripped
    with pytest.raises(ValueError):
        U.commit(ck, P.frs([1] * ((xd + 1) * (yd + 1) + 1)))
    ck.close()


@pytest.mark.parametrize("degree", [16383, 65535])
def test_univariate_equals_the_python_path_member_for_member(engine, orc, P, T, degree):
    U, PU = T.UnivariatePolynomialCommitment, P.transparent.UnivariatePolynomialCommitment
    rng = random.Random(degree)
    ck = U.setup(700, 900, degree); pck = PU.setup(700, 900, degree)
    k1, k2 = ck.keys(); assert np.array_equal(k1, pck[0][:, :12]) and np.array_equal(k2, pck[1][:, :24])
    c = engine.synth_fr(17, degree + 1); p = _ints(orc, c)
    com, coms = U.commit(ck, c); pcom, pcoms = PU.commit(pck, p)
    assert np.array_equal(com, pcom) and _same_g1(orc, coms, pcoms)
    z = rng.randrange(orc.R); fz = P.frs([z])[0]
    proof, val = U.open(ck, c, coms, fz); pproof = PU.open(pck, p, pcoms, z)
    _cmp_python(orc, proof, pproof)
    ival = _int(orc, val); assert ival == _horner(orc, p, z)
    assert U.verify(ck, com, fz, val, proof) and PU.verify(pck, com, z, ival, proof) and U.verify(ck, com, fz, val, pproof)
    assert not U.verify(ck, com, fz, P.frs([ival + 1])[0], proof)
    ck.close()


def test_univariate_2p20(engine, orc, P, T):
    """degree 2^20 - 1 (x_degree 255, y_degree 4095), the inputs of test_univariate_2p20_commit_and_open"""
    from ripp_amd._lib import lib
    degree = (1 << 20) - 1
    U, PU = T.UnivariatePolynomialCommitment, P.transparent.UnivariatePolynomialCommitment
    assert U.bivariate_degrees(degree) == (255, 4095)
    ck = U.setup(700, 900, degree)
    c = engine.synth_fr(29, degree + 1)
    com, coms = U.commit(ck, c)
    k1, _ = ck.keys()
    for row in (0, 100, 255):
        exp = np.zeros(18, dtype=np.uint64); sc = np.ascontiguousarray(c[row * 4096:(row + 1) * 4096])
        assert lib().ripp_msm_g1_a(_p(k1), _p(sc), ctypes.c_size_t(4096), _p(exp)) == 0
        assert _same_g1(orc, coms[row], exp), row
    z = 0x1234567890ABCDEF1234567890ABCDEF % orc.R; fz = P.frs([z])[0]
    proof, val = U.open(ck, c, coms, fz)
    ival = _int(orc, val)
    assert ival == _horner(orc, _ints(orc, c), z)
    assert U.verify(ck, com, fz, val, proof) and not U.verify(ck, com, fz, P.frs([ival + 1])[0], proof)
    pck = _py_ck(orc, ck)
    assert PU.verify(pck, com, z, ival, proof)                                             # the Python-path verifier accepts
    ck.close(); engine.release_scratch()


# ---------------------------------------------------------------------------------------------------------------- BLS12-377
def test_bls12_377_bivariate_is_self_consistent(engine):
    """bivariate (7, 7) on libripp_hip_377.so.  There is no second implementation of the two tier arguments on this curve, so this is a SELF-CONSISTENCY
    check: the Pedersen commitments against per-row ripp_msm_g1_a, the commitment against AFGHOCommitmentG1.commit, the value against Python integers, and
    the native verifier accepts its own proof and rejects eval + 1."""
    import ripp_amd.bls12_377 as R7
    from ripp_amd.poly_commit import native
    R7.init(0)
    T7 = native.bind(R7.lib).transparent; L = R7.lib(); r = R7.R_MOD
    B = T7.BivariatePolynomialCommitment
    x = 0x8508C00000000001; p377 = (x - 1) ** 2 * (x ** 4 - x ** 2 + 1) // 3 + x
    fp_one = np.array([(((1 << 384) % p377) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)], dtype=np.uint64)

    def fr(v):
        m = (v % r) * (1 << 256) % r
        return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)

    def frs(vals): return np.stack([fr(v) for v in vals])
    def same_g1(a, b): return np.array_equal(R7.normalize_batch_g1(np.asarray(a).reshape(-1, 18)), R7.normalize_batch_g1(np.asarray(b).reshape(-1, 18)))

    x_degree = y_degree = 7
    rng = random.Random(377)
    ck = B.setup(700, 900, x_degree, y_degree)
    k1, k2 = ck.keys()
    assert np.array_equal(k1, R7.synth_g1(700, y_degree + 1)) and np.array_equal(k2, R7.synth_g2(900, x_degree + 1))
    ys = [[rng.randrange(r) for _ in range(y_degree + 1)] for _ in range(x_degree + 1)]
    coeffs = np.stack([frs(row) for row in ys])
    com, coms = B.commit(ck, coeffs)
    pcoms = np.zeros((x_degree + 1, 18), dtype=np.uint64)
    for i, row in enumerate(ys):
        assert L.ripp_msm_g1_a(_p(k1), _p(frs(row)), ctypes.c_size_t(y_degree + 1), _p(pcoms[i])) == 0
    assert same_g1(coms, pcoms)
    k2j = np.zeros((x_degree + 1, 36), dtype=np.uint64); k2j[:, :24] = k2; k2j[:, 24:30] = fp_one
    assert np.array_equal(np.asarray(com).reshape(-1), np.asarray(R7.AFGHOCommitmentG1.commit(k2j, pcoms)).reshape(-1))
    px, py = rng.randrange(r), rng.randrange(r)
    proof, val = B.open(ck, coeffs, coms, (fr(px), fr(py)))
    acc = sum(pow(px, i, r) * sum(cf * pow(py, j, r) for j, cf in enumerate(row)) for i, row in enumerate(ys)) % r
    assert np.array_equal(val, fr(acc))
    assert B.verify(ck, com, (fr(px), fr(py)), val, proof)
    assert not B.verify(ck, com, (fr(px), fr(py)), fr(acc + 1), proof)
    ck.close()


# ---------------------------------------------------------------------------------------------------------------- the timing condition
def test_native_is_not_slower_than_the_python_path(engine, orc, P, T):
    """degree 65 535 (x_degree 63, y_degree 1023): native commit, open and verify against the Python path's, same process and device, medians of 5 after a
    warm-up"""
    degree = 65535
    U, PU = T.UnivariatePolynomialCommitment, P.transparent.UnivariatePolynomialCommitment
    ck = U.setup(700, 900, degree); pck = PU.setup(700, 900, degree)
    c = engine.synth_fr(23, degree + 1); p = _ints(orc, c)
    z = 0xFEDCBA9876543210 % orc.R; fz = P.frs([z])[0]
    com, coms = U.commit(ck, c); proof, val = U.open(ck, c, coms, fz); ival = _int(orc, val)

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(5):
            t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
        return sorted(ts)[2]

    pairs = {"commit": (lambda: U.commit(ck, c), lambda: PU.commit(pck, p)),
             "open": (lambda: U.open(ck, c, coms, fz), lambda: PU.open(pck, p, coms, z)),
             "verify": (lambda: U.verify(ck, com, fz, val, proof), lambda: PU.verify(pck, com, z, ival, proof))}
    times = {k: (median_ms(a), median_ms(b)) for k, (a, b) in pairs.items()}
    for k, (tn, tp) in times.items():
        print(f"\ntransparent {k} at degree {degree}: native {tn:.2f} ms, Python path {tp:.2f} ms, ratio {tp / tn:.2f}")
    for k, (tn, tp) in times.items():
        assert tn <= tp, (k, tn, tp)
    ck.close()
