"""GPU parity (-m gpu): the native TIPA provers / verifiers for multiexponentiation products with a committed scalar vector (ripp_tipa_mexp_*;
ripp_amd.api.TIPA_MEXP) and for scalar products (ripp_tipa_scalar_*; TIPA_SCALAR) against the CPU model tests/model/tipa_generic_oracle.py.

RIPP_TIPA_SCALAR_CROSS_MIN moves the key length from which a scalar-product round's two G2 commitments run as ONE crossed pass of the batched MSM pipeline
in its G2 form (tipa_scalar.hpp) and its two G1 commitments as one crossed pass of the G1 form: 2 = every round, 64 = the long rounds only, 1 << 40 = never
(two single MSMs per group).  RIPP_GIPA_MEXP_BATCH_MIN does the same for the four G1 MSMs of a multiexponentiation round.  All forms compute the same group
elements, so every output is compared exactly: GT values and scalars as bytes, projective points after normalisation."""
import os

import numpy as np
import pytest

import tipa_generic_inputs as I

pytestmark = pytest.mark.gpu

NEVER = str(1 << 40)
MEXP_ENV, SCAL_ENV = "RIPP_GIPA_MEXP_BATCH_MIN", "RIPP_TIPA_SCALAR_CROSS_MIN"
MEXP_BOUNDS, SCAL_BOUNDS = ("2", NEVER), ("2", "64", NEVER)
FIXED = ("base_a", "base_b", "final_ck_a", "final_ck_b", "opening_a", "opening_b", "kzg_c")


def _with_env(changes, fn):
    saved = {k: os.environ.get(k) for k in changes}
    os.environ.update(changes)
    try:
        return fn()
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def _fr(orc, v):
    return orc.fr_array([v % orc.R])[0]


def _prove(mod, cls, env_name, bound, srs, case, shift=1, env=None, orc=None):
    """one native proof of a case of tipa_generic_inputs with the bound (None: the library's default) and further environment switches set for the call"""
    import orclib
    orc = orc or orclib
    changes = dict(env or {})
    if bound is not None: changes[env_name] = bound
    args = (srs, (case["m_a"], case["m_b"]), (orc.normalize_g2(case["ck_a"]), orc.normalize_g1(case["ck_b"])))
    if shift == 1:
        return _with_env(changes, lambda: getattr(mod, cls).prove(*args))
    return _with_env(changes, lambda: getattr(mod, cls).prove_with_srs_shift(*args, _fr(orc, shift)))


def _native_srs(mod, case):
    s = case["srs"]
    return mod.SRS(s[0], s[1], s[2], s[3])


def _vkey(case):
    g, h, g_beta, h_alpha = I.verifier_srs(case)
    return {"g": g, "h": h, "g_beta": g_beta, "h_alpha": h_alpha}


MEXP_STEPS = (("com_gt", "GT"), ("com_ped", "G1"), ("com_ip", "G1"))
SCAL_STEPS = (("com_g2", "G2"), ("com_g1", "G1"), ("com_fr", "FR"))
MEXP_TYPES = dict(base_a="G1", base_b="FR", final_ck_a="G2", final_ck_b="G1", opening_a="G2", opening_b="G1", kzg_c="FR")
SCAL_TYPES = dict(MEXP_TYPES, base_a="FR")


def _canon(orc, tag, v):
    v = np.asarray(v)
    if tag == "G1": return orc.g1_to_affine(v).tobytes()
    if tag == "G2": return orc.g2_to_affine(v).tobytes()
    return v.tobytes()


def _flat(orc, proof, steps, types):
    """every output of a native proof in a form that compares exactly"""
    out = [proof["tr"].tobytes()]
    for name, tag in steps:
        out += [_canon(orc, tag, row) for row in proof[name]]
    out += [_canon(orc, types[k], proof[k]) for k in FIXED]
    return tuple(out)


def _model_value(orc, tag, v):
    return _fr(orc, v) if tag == "FR" else v


def _assert_equals_model(orc, proof, model, steps, types):
    rounds = len(model["steps"])
    for name, _ in steps: assert len(proof[name]) == 2 * rounds
    for k in range(rounds):
        for side in range(2):
            for j, (name, tag) in enumerate(steps):
                assert _canon(orc, tag, proof[name][2 * k + side]) == _canon(orc, tag, _model_value(orc, tag, model["steps"][k][side][j])), (k, side, name)
    assert proof["tr"].tobytes() == orc.fr_array(model["tr"]).tobytes()
    want = dict(base_a=model["base"][0], base_b=model["base"][1], final_ck_a=model["final_ck"][0], final_ck_b=model["final_ck"][1],
                opening_a=model["opening_a"], opening_b=model["opening_b"], kzg_c=model["kzg_c"])
    for k in FIXED:
        assert _canon(orc, types[k], proof[k]) == _canon(orc, types[k], _model_value(orc, types[k], want[k])), k


def _as_model_proof(orc, proof, steps, types):
    """a native proof in the layout of the model's verifier"""
    val = lambda tag, v: orc.limbs_to_fr(v) if tag == "FR" else np.asarray(v)
    rounds = len(proof["tr"])
    st = [tuple(tuple(val(tag, proof[name][2 * k + side]) for name, tag in steps) for side in range(2)) for k in range(rounds)]
    return dict(steps=st, base=(val(types["base_a"], proof["base_a"]), val("FR", proof["base_b"])), final_ck=(proof["final_ck_a"], proof["final_ck_b"]),
                opening_a=proof["opening_a"], opening_b=proof["opening_b"])


def _native_com(orc, case, inst):
    c = case["com"]
    return (c[0], c[1], _fr(orc, c[2]) if inst[3] == "FR" else c[2])


def _parity(engine, orc, cls, inst, env_name, bounds, case, steps, types, shift=1):
    import tipa_generic_oracle as T
    srs = _native_srs(engine, case)
    try:
        outs = []
        for bound in bounds:
            proof = _prove(engine, cls, env_name, bound, srs, case, shift)
            _assert_equals_model(orc, proof, case["model"], steps, types)
            outs.append(_flat(orc, proof, steps, types))
        assert all(x == outs[0] for x in outs)
        V = getattr(engine, cls)
        com = _native_com(orc, case, inst)
        if shift == 1:
            assert V.verify(_vkey(case), com, proof)
        else:
            assert V.verify_with_srs_shift(_vkey(case), com, proof, _fr(orc, shift))
            assert not V.verify(_vkey(case), com, proof)                                          # r_shift = 1: the opening of ck_a no longer fits
        assert T.verify(inst, I.verifier_srs(case), case["com"], _as_model_proof(orc, proof, steps, types), shift)
        st = proof["stats"]
        assert st["total_ms"] > 0 and st["miller_products_ms"] > 0 and st["fold_ms"] > 0 and st["host_ms"] > 0
    finally:
        srs.close()


@pytest.mark.parametrize("n", I.SIZES_MEXP)
def test_mexp_parity_with_the_model(engine, orc, n):
    """n = 2: one round, h = 1, three SRS powers; n = 8: the reference's TEST_SIZE; n = 16: the LEN of its bench.  Both forms of the round's four G1 MSMs."""
    _parity(engine, orc, "TIPA_MEXP", I.INST_MEXP, MEXP_ENV, MEXP_BOUNDS, I.mexp_case(n), MEXP_STEPS, MEXP_TYPES)


@pytest.mark.parametrize("n", I.SIZES_SCAL)
def test_scalar_parity_with_the_model(engine, orc, n):
    """n = 2: one round, h = 1, three SRS powers; n = 8: the reference's TEST_SIZE; n = 16: the LEN of its bench; 64: the bound 64 mixes both forms in one proof.
    n = 512: the crossed G2 digit pass has a lane per key, 256 to a block, so 512 is the smallest length with more than one block.  The LDS sort runs in tiles
    of msm_sort_tile(p) >= 1024 terms, a G2 row has 4 terms per key, so more than one tile needs 4 n > 1024: n = 512 as well (at n = 512 the plan has
    c = 4, 2 x 16 virtual windows, 15 tiles wanted of ceil(2048 / 15) terms rounded up to 1024: two tiles).  The larger of the two is 512."""
    _parity(engine, orc, "TIPA_SCALAR", I.INST_SCAL, SCAL_ENV, SCAL_BOUNDS, I.scalar_case(n), SCAL_STEPS, SCAL_TYPES)


def test_shifted_statements(engine, orc):
    """r_shift != 1 at n = 8: ck_a shifted by the inverse powers and m_a by the powers (tipa/mod.rs:545-561).  The verifier rejects with r_shift = 1."""
    _parity(engine, orc, "TIPA_MEXP", I.INST_MEXP, MEXP_ENV, MEXP_BOUNDS, I.mexp_case(8, I.SHIFT), MEXP_STEPS, MEXP_TYPES, I.SHIFT)
    _parity(engine, orc, "TIPA_SCALAR", I.INST_SCAL, SCAL_ENV, ("2", NEVER), I.scalar_case(8, I.SHIFT), SCAL_STEPS, SCAL_TYPES, I.SHIFT)


@pytest.mark.parametrize("trapdoors", sorted(I.TRAPDOORS))
@pytest.mark.parametrize("which", [0, 1])
def test_scalar_edges(engine, orc, trapdoors, which):
    """n = 8, crossed form forced: the zero remainders and quotients of the base-|x| split on the G2 side, the lambda edges on the G1 side, and SRS sets whose
    powers are all +-generator, so that the gather meets doublings and P + (-P) and the exceptional-slot fix-up runs in both groups.
    tests/test_tipa_generic_cpu.py::test_model_proves_the_scalar_edge_sets holds the model to these inputs."""
    _parity(engine, orc, "TIPA_SCALAR", I.INST_SCAL, SCAL_ENV, ("2", NEVER), I.scalar_edge_case(trapdoors, which), SCAL_STEPS, SCAL_TYPES)


def _dbl(orc, tag, v):
    import gipa_generic_oracle as G
    return G.plus(tag, v, v) if tag != "FR" else _fr(orc, 2 * orc.limbs_to_fr(v))


def _rejects(engine, orc, cls, inst, env_name, case, steps, types, not_gt):
    srs = _native_srs(engine, case)
    try:
        proof = _prove(engine, cls, env_name, "2", srs, case)
    finally:
        srs.close()
    V, vk, com = getattr(engine, cls).verify, _vkey(case), _native_com(orc, case, inst)
    out_tags = (steps[0][1], "G1", inst[3])
    assert V(vk, com, proof)
    other = {"G1": orc.to_jac_g1(orc.gen_g1(999, 1))[0], "G2": orc.to_jac_g2(orc.gen_g2(999, 1))[0]}

    def changed(**kw):
        p = dict(proof); p.update(kw); return p

    first = steps[0][0]
    swapped = {name: proof[name].copy() for name, _ in steps}
    for name in swapped: swapped[name][[2, 3]] = swapped[name][[3, 2]]
    assert not V(vk, com, changed(**swapped))                                                        # com_1 and com_2 swapped in round 1
    for j, (name, tag) in enumerate(steps):                                                       # one tampered element of each step array
        arr = proof[name].copy(); arr[j] = _dbl(orc, tag, arr[j]) if tag != "GT" else orc.gt_mul(arr[j], arr[j])
        assert not V(vk, com, changed(**{name: arr})), name
    if not_gt:                                                                                    # no element of GT at all: refused, not an error
        arr = proof[first].copy(); arr[0, 0] ^= 1
        assert not V(vk, com, changed(**{first: arr}))
    assert not V(vk, com, changed(base_a=_dbl(orc, types["base_a"], proof["base_a"])))
    assert not V(vk, com, changed(base_b=_fr(orc, orc.limbs_to_fr(proof["base_b"]) + 1)))
    assert not V(vk, com, changed(final_ck_a=other["G2"]))
    assert not V(vk, com, changed(final_ck_b=other["G1"]))
    assert not V(vk, com, changed(opening_a=other["G2"]))
    assert not V(vk, com, changed(opening_b=other["G1"]))
    for j in range(3):                                                                            # com_a / com_b / com_t
        c = list(com); c[j] = orc.gt_mul(c[j], c[j]) if out_tags[j] == "GT" else _dbl(orc, out_tags[j], c[j])
        assert not V(vk, tuple(c), proof), j
    assert V(vk, com, proof)


def test_mexp_verifier_rejects(engine, orc):
    """every tampered proof is refused with RIPP_OK and accept = 0 (the binding raises on any other status); the untouched proof is accepted before and after"""
    _rejects(engine, orc, "TIPA_MEXP", I.INST_MEXP, MEXP_ENV, I.mexp_case(8), MEXP_STEPS, MEXP_TYPES, True)


def test_scalar_verifier_rejects(engine, orc):
    _rejects(engine, orc, "TIPA_SCALAR", I.INST_SCAL, SCAL_ENV, I.scalar_case(8), SCAL_STEPS, SCAL_TYPES, False)


@pytest.mark.parametrize("switch", ["no_msm_glv", "no_fq", "no_vm", "RIPP_NO_MSM_BATCH"])
def test_legacy_switches_take_the_fallback(engine, orc, switch):
    """under the legacy MSM switches the bound is ignored (msm_batch_legacy()): n = 64 with the bound at 2 gives the proof of the default path"""
    case = I.scalar_case(64)
    srs = _native_srs(engine, case)
    try:
        default = _flat(orc, _prove(engine, "TIPA_SCALAR", SCAL_ENV, None, srs, case), SCAL_STEPS, SCAL_TYPES)
        try:
            if switch.startswith("RIPP_"):
                got = _prove(engine, "TIPA_SCALAR", SCAL_ENV, "2", srs, case, env={switch: "1"})
            else:
                engine.configure(**{switch: 1})
                got = _prove(engine, "TIPA_SCALAR", SCAL_ENV, "2", srs, case)
        finally:
            engine.configure()
    finally:
        srs.close()
    _assert_equals_model(orc, got, case["model"], SCAL_STEPS, SCAL_TYPES)
    assert _flat(orc, got, SCAL_STEPS, SCAL_TYPES) == default


def test_template_regression(engine, orc):
    """The batched MSM pipeline became a template over the field: its G1 forms still give the oracle's points -- ripp_msm_g1_batch_a at 3 x 300 with stride 320
    (the plain form) and the four-row form inside GIPA_MEXP.prove_with_aux at n = 64 with the bound at 2."""
    import ctypes
    import gipa_mexp_inputs as GI
    from ripp_amd._lib import lib
    rows, cols, stride = 3, 300, 320
    bases = orc.gen_g1(7, cols); sc = orc.gen_scalars(9, rows * stride).reshape(rows, stride, 4)
    out = np.zeros((rows, 18), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib().ripp_msm_g1_batch_a(p(bases), ctypes.c_size_t(cols), p(sc), ctypes.c_size_t(rows), ctypes.c_size_t(cols), ctypes.c_size_t(stride), p(out)) == 0
    for r in range(rows):
        want = orc.msm_g1_a(bases, np.ascontiguousarray(sc[r, :cols]))
        assert np.array_equal(orc.g1_to_affine(out[r]), orc.g1_to_affine(want)), r
    inputs = GI.regular(orc, 64)
    steps, tr, base, ck_base, com = GI.model_prove(orc, *inputs)
    proof, aux, extra = _with_env({MEXP_ENV: "2"}, lambda: engine.GIPA_MEXP.prove_with_aux(*inputs))
    assert extra["round_order_transcript"].tobytes() == orc.fr_array(tr).tobytes()
    for k in range(len(steps)):
        for side in range(2):
            assert np.array_equal(extra["round_order_com_gt"][2 * k + side], steps[k][side][0])
            assert _canon(orc, "G1", extra["round_order_com_ped"][2 * k + side]) == _canon(orc, "G1", steps[k][side][1])
            assert _canon(orc, "G1", extra["round_order_com_ip"][2 * k + side]) == _canon(orc, "G1", steps[k][side][2])


def test_bls12_377(engine):
    """The BLS12-377 build at n = 8, both provers.  There is no BLS12-377 model of the generic TIPA, so this is a self-consistency check: the verifier accepts
    the proof against commitments computed by the trait-level calls, rejects a tampered step, and both bound settings give the same transcript."""
    import orclib377 as o7
    import ripp_amd.bls12_377 as R7
    R7.init(0)
    n = 8
    alpha, beta = R7.synth_fr(91, 1)[0], R7.synth_fr(92, 1)[0]
    srs = R7.SRS.from_trapdoors(alpha, beta, n)
    try:
        ck_a, ck_b = srs.get_commitment_keys()
        vk = srs.get_verifier_key()
        a = o7.blind_g1(R7.synth_g1(11, n), 1); s1, s2 = R7.synth_fr(5, n), R7.synth_fr(6, n)
        cases = (("TIPA_MEXP", MEXP_ENV, (a, s1), (R7.AFGHOCommitmentG1.commit(ck_a, a), R7.PedersenCommitmentG1.commit(ck_b, s1), R7.MultiexponentiationInnerProductG1.inner_product(a, s1)), "com_ip",
                  o7.to_jac_g1(R7.synth_g1(999, 1))[0]),
                 ("TIPA_SCALAR", SCAL_ENV, (s1, s2), (R7.PedersenCommitmentG2.commit(ck_a, s1), R7.PedersenCommitmentG1.commit(ck_b, s2), R7.ScalarInnerProduct.inner_product(s1, s2)), "com_fr",
                  R7.synth_fr(999, 1)[0]))
        for cls, env_name, values, com, step, other in cases:
            C = getattr(R7, cls)
            p1 = _with_env({env_name: "2"}, lambda: C.prove(srs, values, (ck_a, ck_b)))
            p2 = _with_env({env_name: NEVER}, lambda: C.prove(srs, values, (ck_a, ck_b)))
            assert p1["tr"].tobytes() == p2["tr"].tobytes() and p1["kzg_c"].tobytes() == p2["kzg_c"].tobytes()
            com = tuple(np.asarray(c).reshape(-1) for c in com)
            assert C.verify(vk, com, p1) and C.verify(vk, com, p2)
            bad = dict(p1); arr = p1[step].copy(); arr[2] = other; bad[step] = arr
            assert not C.verify(vk, com, bad)
    finally:
        srs.close()


def test_device_memory_returns(engine, orc):
    """ripp_release_scratch frees everything the provers and the verifiers hold, the parked vector sets included"""
    cases = (("TIPA_MEXP", I.INST_MEXP, MEXP_ENV, I.mexp_case(16)), ("TIPA_SCALAR", I.INST_SCAL, SCAL_ENV, I.scalar_case(64)))
    warm = I.scalar_case(2); s = _native_srs(engine, warm)
    _prove(engine, "TIPA_SCALAR", SCAL_ENV, "2", s, warm); s.close()   # the flag word of the VM folds (4 bytes) is allocated by the first fold of a process and lives until ripp_shutdown
    engine.release_scratch()
    before = engine.device_bytes()
    for cls, inst, env_name, case in cases:
        srs = _native_srs(engine, case)
        try:
            for bound in ("2", NEVER):
                proof = _prove(engine, cls, env_name, bound, srs, case)
                assert engine.device_bytes() > before
                assert getattr(engine, cls).verify(_vkey(case), _native_com(orc, case, inst), proof)
        finally:
            srs.close()
    engine.release_scratch()
    assert engine.device_bytes() == before
