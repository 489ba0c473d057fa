"""GPU parity (-m gpu): the fused GIPA prover / verifier for multiexponentiation products with a committed scalar vector (ripp_gipa_mexp_prove /
ripp_gipa_mexp_verify; ripp_amd.api.GIPA_MEXP) against the CPU model tests/model/gipa_generic_oracle.py and the generic trait-level path ripp_amd/gipa.py.

RIPP_GIPA_MEXP_BATCH_MIN moves the vector length from which a round's four G1 MSMs run as ONE four-row pass of the batched MSM pipeline (gipa_mexp.hpp):
2 = every round, 64 = the long rounds only, 1 << 40 = never (four single MSMs).  All forms compute the same group elements, so every output is compared
exactly: GT values and scalars as bytes, projective points after normalisation."""
import functools
import os

import numpy as np
import pytest

import gipa_mexp_inputs as I

pytestmark = pytest.mark.gpu

BOUNDS = ("2", "64", str(1 << 40))
ENV = "RIPP_GIPA_MEXP_BATCH_MIN"


def _prove(mod, bound, *inputs, env=None):
    """one native proof with the bound (None: the library's default) and further environment switches set for the call"""
    changes = dict(env or {})
    if bound is not None: changes[ENV] = bound
    saved = {k: os.environ.get(k) for k in changes}
    os.environ.update(changes)
    try:
        return mod.GIPA_MEXP.prove_with_aux(*inputs)
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _reference(n):
    """the model's proof of the regular inputs of length n, computed once per size and shared"""
    import orclib as orc
    inputs = I.regular(orc, n)
    return inputs, I.model_prove(orc, *inputs)


def _flat(orc, engine, proof, aux, extra):
    """every output of a native proof in a form that compares exactly: bytes of the GT values and scalars, affine points"""
    pts = np.concatenate([extra["round_order_com_ped"], extra["round_order_com_ip"], proof["r_base"][0][None], aux["ck_base"][1][None]])
    return (extra["round_order_com_gt"].tobytes(), extra["round_order_transcript"].tobytes(), np.asarray(proof["r_base"][1]).tobytes(),
            orc.g1_to_affine(pts).tobytes(), orc.g2_to_affine(aux["ck_base"][0][None]).tobytes())


def _assert_equals_model(orc, proof, aux, extra, model):
    import gipa_generic_oracle as M
    steps, tr, base, ck_base, _ = model
    rounds = len(steps)
    gt, ped, ip = extra["round_order_com_gt"], extra["round_order_com_ped"], extra["round_order_com_ip"]
    assert len(gt) == len(ped) == len(ip) == 2 * rounds and len(proof["r_commitment_steps"]) == rounds
    for k in range(rounds):
        for side in range(2):
            assert np.array_equal(gt[2 * k + side], steps[k][side][0]), (k, side)
            assert M.same("G1", ped[2 * k + side], steps[k][side][1]), (k, side)
            assert M.same("G1", ip[2 * k + side], steps[k][side][2]), (k, side)
            got = proof["r_commitment_steps"][rounds - 1 - k][side]                                 # the dict holds the same values, reversed
            assert np.array_equal(got[0], gt[2 * k + side]) and np.array_equal(got[1], ped[2 * k + side]) and len(got[2]) == 1 and np.array_equal(got[2][0], ip[2 * k + side])
    assert extra["round_order_transcript"].tobytes() == orc.fr_array(tr).tobytes()
    assert np.array_equal(aux["r_transcript"], extra["round_order_transcript"][::-1])
    assert M.same("G1", proof["r_base"][0], base[0]) and orc.limbs_to_fr(proof["r_base"][1]) == base[1] % orc.R
    assert M.same("G2", aux["ck_base"][0], ck_base[0]) and M.same("G1", aux["ck_base"][1], ck_base[1])


def _round_order(proof):
    return [(tuple(s[0][:2]) + (s[0][2][0],), tuple(s[1][:2]) + (s[1][2][0],)) for s in proof["r_commitment_steps"][::-1]]


@pytest.mark.parametrize("n", [2, 4, 8, 64, 256])
def test_parity_with_the_model(engine, orc, n):
    """n = 2: h = 1, one term per row; n = 4: the first round whose folded X = (ck_b | m_a) feeds a batch; n = 256: X holds 512 bases, so the digit pass runs
    more than one block and the sort more than one tile.  Bound 64 mixes the two forms inside one proof."""
    inputs, model = _reference(n)
    outs = []
    for bound in BOUNDS:
        proof, aux, extra = _prove(engine, bound, *inputs)
        _assert_equals_model(orc, proof, aux, extra, model)
        outs.append(_flat(orc, engine, proof, aux, extra))
    assert outs[0] == outs[1] == outs[2]
    steps, tr, base, ck_base, com = model
    assert I.model_verify(orc, inputs[2], inputs[3], com, _round_order(proof), proof["r_base"][:1] + (orc.limbs_to_fr(proof["r_base"][1]),))
    assert engine.GIPA_MEXP.verify((inputs[2], inputs[3], None), (com[0], com[1], [com[2]]), proof)
    st = extra["stats"]
    assert st["total_ms"] > 0 and st["miller_products_ms"] > 0 and st["fold_ms"] > 0 and st["host_ms"] > 0


@pytest.mark.parametrize("n", [2, 8, 64])
def test_cross_acceptance_with_the_generic_path(engine, orc, n):
    """the generic verifier of ripp_amd/gipa.py accepts the native proof and ripp_gipa_mexp_verify the generic prover's"""
    import ripp_amd.gipa as G
    (m_a, m_b, ck_a, ck_b), model = _reference(n)
    gipa = G.GIPA(G.MultiexpIPG1, G.AFGHOCommitmentG1, G.PedersenCommitmentG1, G.IdentityCommitment(G.G1))
    ka, kb = orc.to_jac_g2(ck_a), orc.to_jac_g1(ck_b)                                              # the trait-level path takes projective keys
    com = (G.AFGHOCommitmentG1.commit(ka, m_a), G.PedersenCommitmentG1.commit(kb, m_b), [G.MultiexpIPG1.inner_product(m_a, m_b)])
    native, _, _ = _prove(engine, "2", m_a, m_b, ck_a, ck_b)
    assert gipa.verify((ka, kb, None), com, native)
    generic, _ = gipa.prove_with_aux((m_a, m_b), (ka, kb, [None]))
    assert engine.GIPA_MEXP.verify((ck_a, ck_b, None), com, generic)
    assert engine.GIPA_MEXP.verify((ka, kb, None), com, generic)                                   # projective keys are normalised by the binding
    wrong = (com[0], com[1], [G.G1.add(com[2][0], com[2][0])])
    assert not engine.GIPA_MEXP.verify((ck_a, ck_b, None), wrong, generic)


def test_edges(engine, orc):
    """n = 8 with every round in the one-pass form: scalars 0, 1, r - 1, lambda, lambda + 1, 2^128 - 1, 2^128 (a zero remainder, a zero quotient, the extreme
    digits), a repeated point in each half of m_a and the identity in it, a repeated point in ck_b (exceptional additions in the gather and their fix-up).
    tests/test_gipa_mexp_cpu.py::test_model_accepts_the_edge_inputs holds the model to these inputs."""
    inputs = I.edges(orc)
    model = I.model_prove(orc, *inputs)
    proof, aux, extra = _prove(engine, "2", *inputs)
    _assert_equals_model(orc, proof, aux, extra, model)
    proof2, aux2, extra2 = _prove(engine, str(1 << 40), *inputs)
    assert _flat(orc, engine, proof, aux, extra) == _flat(orc, engine, proof2, aux2, extra2)
    com = model[4]
    assert engine.GIPA_MEXP.verify((inputs[2], inputs[3], None), (com[0], com[1], [com[2]]), proof)


def _dbl(orc, p):
    return orc.fold_g1_j(np.asarray(p)[None], np.asarray(p)[None], orc.fr_array([1])[0])[0]


def test_verifier_rejects(engine, orc):
    """every tampered proof is refused with RIPP_OK and accept = 0 (GIPA_MEXP.verify raises on any other status)"""
    n = 8
    (m_a, m_b, ck_a, ck_b), model = _reference(n)
    c = model[4]; com = (c[0], c[1], [c[2]]); ck = (ck_a, ck_b, None)
    proof, _, _ = _prove(engine, "2", m_a, m_b, ck_a, ck_b)
    V = engine.GIPA_MEXP.verify
    assert V(ck, com, proof)
    other_g1 = orc.to_jac_g1(orc.gen_g1(999, 1))[0]

    def with_step(k, fn):
        steps = list(proof["r_commitment_steps"]); steps[k] = fn(steps[k]); return {"r_commitment_steps": steps, "r_base": proof["r_base"]}

    assert not V(ck, com, with_step(1, lambda s: (s[1], s[0])))                                                           # com_1 and com_2 swapped in one round
    assert not V(ck, com, with_step(0, lambda s: ((orc.gt_mul(s[0][0], s[0][0]), s[0][1], s[0][2]), s[1])))              # one element of com_gt
    assert not V(ck, com, with_step(2, lambda s: (s[0], (s[1][0], other_g1, s[1][2]))))                                   # ... of com_ped
    assert not V(ck, com, with_step(1, lambda s: ((s[0][0], s[0][1], [other_g1]), s[1])))                                 # ... of com_ip
    not_gt = np.asarray(proof["r_commitment_steps"][0][0][0]).copy(); not_gt[0] ^= 1                                      # no element of GT at all: refused, not an error
    assert not V(ck, com, with_step(0, lambda s: ((not_gt, s[0][1], s[0][2]), s[1])))
    ba, bb = proof["r_base"]
    assert not V(ck, com, {"r_commitment_steps": proof["r_commitment_steps"], "r_base": (_dbl(orc, ba), bb)})             # base_a doubled
    bb1 = orc.fr_array([orc.limbs_to_fr(bb) + 1])[0]
    assert not V(ck, com, {"r_commitment_steps": proof["r_commitment_steps"], "r_base": (ba, bb1)})                       # base_b + 1
    assert not V(ck, (com[0], com[1], [_dbl(orc, com[2][0])]), proof)                                                     # com_t doubled
    assert not V(ck, (com[0], other_g1, com[2]), proof)                                                                   # com_b replaced
    assert V(ck, com, proof)


@pytest.mark.parametrize("switch", ["no_msm_glv", "no_fq", "no_vm", "RIPP_NO_MSM_BATCH"])
def test_legacy_switches_take_the_fallback(engine, orc, switch):
    """under the legacy MSM switches the bound is ignored (msm_batch_legacy()): n = 64 with the bound at 2 gives the proof of the default path"""
    inputs, model = _reference(64)
    default = _flat(orc, engine, *_prove(engine, None, *inputs))
    try:
        if switch.startswith("RIPP_"):
            got = _prove(engine, "2", *inputs, env={switch: "1"})
        else:
            engine.configure(**{switch: 1})
            got = _prove(engine, "2", *inputs)
    finally:
        engine.configure()
    _assert_equals_model(orc, *got, model)
    assert _flat(orc, engine, *got) == default


def test_bls12_377(engine):
    """The BLS12-377 build at n = 8.  There is no BLS12-377 model of the generic GIPA, so this is a self-consistency check: the verifier accepts the proof
    against commitments computed by the trait-level calls, rejects a tampered inner-product step, and both forms of the rounds give the same transcript."""
    import orclib377 as o7
    import ripp_amd.bls12_377 as R7
    R7.init(0)
    n = 8
    a, m_b, ck_a, ck_b = R7.synth_g1(11, n), R7.synth_fr(5, n), R7.synth_g2(33, n), R7.synth_g1(44, n)
    m_a = o7.blind_g1(a, 1)
    ka, kb = o7.to_jac_g2(ck_a), o7.to_jac_g1(ck_b)
    com = (R7.AFGHOCommitmentG1.commit(ka, m_a), R7.PedersenCommitmentG1.commit(kb, m_b), [R7.MultiexponentiationInnerProductG1.inner_product(m_a, m_b)])
    proof, aux, extra = _prove(R7, "2", m_a, m_b, ck_a, ck_b)
    proof2, aux2, extra2 = _prove(R7, str(1 << 40), m_a, m_b, ck_a, ck_b)
    assert extra["round_order_transcript"].tobytes() == extra2["round_order_transcript"].tobytes()
    assert extra["round_order_com_gt"].tobytes() == extra2["round_order_com_gt"].tobytes()
    assert np.array_equal(R7.normalize_batch_g1(extra["round_order_com_ip"]), R7.normalize_batch_g1(extra2["round_order_com_ip"]))
    assert np.array_equal(R7.normalize_batch_g1(extra["round_order_com_ped"]), R7.normalize_batch_g1(extra2["round_order_com_ped"]))
    ck = (ck_a, ck_b, None)
    assert R7.GIPA_MEXP.verify(ck, com, proof) and R7.GIPA_MEXP.verify(ck, com, proof2)
    steps = list(proof["r_commitment_steps"]); s = steps[1]
    steps[1] = ((s[0][0], s[0][1], [o7.to_jac_g1(R7.synth_g1(999, 1))[0]]), s[1])
    assert not R7.GIPA_MEXP.verify(ck, com, {"r_commitment_steps": steps, "r_base": proof["r_base"]})


def test_device_memory_returns(engine, orc):
    """ripp_release_scratch frees everything the prover and the verifier hold, the parked vector set included"""
    inputs, model = _reference(64)
    c = model[4]
    _prove(engine, "2", *I.regular(orc, 2))              # the flag word of the VM folds (4 bytes) is allocated by the first fold of a process and lives until ripp_shutdown
    engine.release_scratch()
    before = engine.device_bytes()
    for bound in ("2", str(1 << 40)):
        proof, _, _ = _prove(engine, bound, *inputs)
        assert engine.device_bytes() > before
        assert engine.GIPA_MEXP.verify((inputs[2], inputs[3], None), (c[0], c[1], [c[2]]), proof)
    engine.release_scratch()
    assert engine.device_bytes() == before
