"""GPU parity (-m gpu): the native polynomial commitments (`ripp_pc_*`, `ripp_kzg_*`, `ripp_msm_g1_batch_a`; ripp_amd/poly_commit/native.py) against
the existing implementations: the loop of single MSMs, the CPU oracle (tests/model/poly_commit_oracle.py) and the package's Python path
(ripp_amd/poly_commit).  Group elements are compared after normalisation, GT and Fr values byte for byte; these are exact values, nothing is tolerated.

The timing condition at the end (batched MSM against the 64-call loop it replaces, same process, same device, medians of 5 after a warm-up) is a
condition on the batch plan, not a tuned number."""
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
def N(engine):
    from ripp_amd.poly_commit import native
    return native


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _same_g1(orc, a, b):
    a, b = np.asarray(a).reshape(-1, 18), np.asarray(b).reshape(-1, 18)
    return np.array_equal(orc.normalize_g1(np.ascontiguousarray(a)), orc.normalize_g1(np.ascontiguousarray(b)))


def _same_g2(orc, a, b):
    a, b = np.asarray(a).reshape(-1, 36), np.asarray(b).reshape(-1, 36)
    return np.array_equal(orc.normalize_g2(np.ascontiguousarray(a)), orc.normalize_g2(np.ascontiguousarray(b)))


def _msm_loop(engine, bases, scalars):
    """the parent's only way: one ripp_msm_g1_a per row over the same bases; scalars (rows, cols, 4)"""
    from ripp_amd._lib import lib
    out = np.zeros((len(scalars), 18), dtype=np.uint64)
    for r, row in enumerate(scalars):
        row = np.ascontiguousarray(row); b = np.ascontiguousarray(bases[:len(row)])
        assert lib().ripp_msm_g1_a(_p(b), _p(row), ctypes.c_size_t(len(row)), _p(out[r])) == 0
    return out


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


# ---------------------------------------------------------------------------------------------------------------- batched MSM
@pytest.mark.parametrize("cols", [1, 5, 255, 4096, 16384])
@pytest.mark.parametrize("rows", [1, 2, 3, 64])
def test_batch_msm_equals_the_loop(engine, orc, N, rows, cols):
    bases = engine.synth_g1(1000, cols + 7)
    sc = engine.synth_fr(rows * 100000 + cols, rows * (cols + 3)).reshape(rows, cols + 3, 4)
    exp = _msm_loop(engine, bases, sc[:, :cols])
    got = N.msm_g1_batch(bases[:cols], np.ascontiguousarray(sc[:, :cols]))
    assert N.msm_batch_chunks() == 1
    assert _same_g1(orc, got, exp)
    assert _same_g1(orc, N.msm_g1_batch(bases, sc[:, :cols]), exp)                       # n > cols and stride > cols: the view's rows are passed as they lie
    if cols <= 255:
        oexp = np.stack([orc.msm_g1_a(np.ascontiguousarray(bases[:cols]), np.ascontiguousarray(sc[r, :cols])) for r in range(rows)])
        assert _same_g1(orc, got, oexp)


@pytest.mark.parametrize("rows,cols", [(4, 300), (8, 4096)])
def test_batch_msm_scalar_sets(engine, orc, N, P, rows, cols):
    bases = engine.synth_g1(77, cols)
    rnd = engine.synth_fr(5, rows * cols).reshape(rows, cols, 4)
    # an all-zero row among non-zero rows
    sc = rnd.copy(); sc[1] = 0
    got = N.msm_g1_batch(bases, sc); assert _same_g1(orc, got, _msm_loop(engine, bases, sc))
    assert not orc.normalize_g1(np.ascontiguousarray(got[1:2])).any()
    # all scalars equal: every term in one bucket per window
    sc = np.broadcast_to(rnd[0, 0], (rows, cols, 4)).copy()
    got = N.msm_g1_batch(bases, sc); assert _same_g1(orc, got, _msm_loop(engine, bases, sc))
    # scalars 0, 1, r - 1
    vals = P.frs([0, 1, orc.R - 1])
    sc = vals[np.arange(rows * cols) % 3].reshape(rows, cols, 4).copy()
    got = N.msm_g1_batch(bases, sc); assert _same_g1(orc, got, _msm_loop(engine, bases, sc))
    # one row repeated: identical rows give identical points
    sc = rnd.copy(); sc[rows - 1] = sc[0]
    got = N.msm_g1_batch(bases, sc); assert _same_g1(orc, got, _msm_loop(engine, bases, sc))
    assert np.array_equal(orc.normalize_g1(np.ascontiguousarray(got[:1])), orc.normalize_g1(np.ascontiguousarray(got[rows - 1:])))


@pytest.mark.parametrize("rows,cols", [(3, 64), (5, 1024)])
def test_batch_msm_infinity_and_repeated_bases(engine, orc, N, rows, cols):
    """bases holding the point at infinity and repeated bases: equal addends meet in a slot (the exceptional-addition fix-up)"""
    bases = engine.synth_g1(9, cols)
    bases[3] = 0; bases[cols // 2] = 0
    bases[10:20] = bases[20]; bases[cols - 8:] = bases[1]
    sc = engine.synth_fr(11, rows * cols).reshape(rows, cols, 4).copy()
    sc[0, :] = sc[0, 0]                                                                 # equal scalars on repeated bases: P + P inside one bucket
    got = N.msm_g1_batch(bases, sc)
    assert _same_g1(orc, got, _msm_loop(engine, bases, sc))
    if cols <= 64:
        assert _same_g1(orc, got, np.stack([orc.msm_g1_a(np.ascontiguousarray(bases), np.ascontiguousarray(sc[r])) for r in range(rows)]))


@pytest.fixture(scope="module")
def batch_tune_inputs(engine, orc):
    """3 rows over 256 bases, random and all-equal scalars, with the oracle's points (computed once for all the corners)"""
    rows, cols = 3, 256
    bases = engine.synth_g1(515, cols)
    rnd = engine.synth_fr(516, rows * cols).reshape(rows, cols, 4).copy()
    same = np.broadcast_to(rnd[0, 0], (rows, cols, 4)).copy()
    exp = {k: np.stack([orc.msm_g1_a(np.ascontiguousarray(bases), np.ascontiguousarray(sc[r])) for r in range(rows)]) for k, sc in (("random", rnd), ("equal", same))}
    return bases, {"random": rnd, "equal": same}, exp


@pytest.mark.parametrize("c", ["4", "13"])
@pytest.mark.parametrize("ch", ["1", "4"])
@pytest.mark.parametrize("gmin", ["1", "16"])
def test_batch_msm_tuning_corners_vs_oracle(engine, orc, N, batch_tune_inputs, c, ch, gmin):
    """the in-range corners of ripp_config.msm_c / msm_ch / msm_gmin on the batched pipeline (msm_batch_dev: rows x windows virtual windows through the same
    stages), against the oracle; all-equal scalars with CH = 4, GMIN = 1 put 128 slots into one bucket, so the grouping passes run over virtual windows"""
    bases, scalars, exp = batch_tune_inputs
    env = {"RIPP_MSM_C": c, "RIPP_MSM_CH": ch, "RIPP_MSM_GMIN": gmin}
    os.environ.update(env)
    try:
        for kind, sc in scalars.items():
            got = N.msm_g1_batch(bases, sc)
            assert N.msm_batch_chunks() == 1, (env, kind)                                   # the batched pipeline, not the per-row loop
            assert _same_g1(orc, got, exp[kind]), (env, kind)
    finally:
        for k in env: del os.environ[k]


@pytest.mark.parametrize("c", ["3", "14"])
def test_batch_msm_tuning_outside_the_range_is_refused(engine, orc, N, c):
    """msm_batch_dev has no sort but the one through the 8192 LDS counters: RIPP_MSM_C = 14 (and 3, with the single MSM) is refused by msm_tune_ok before anything is
    allocated or launched; the next call without the variable gives the loop's points"""
    rows, cols = 3, 64
    bases = engine.synth_g1(517, cols); sc = engine.synth_fr(518, rows * cols).reshape(rows, cols, 4).copy()
    os.environ["RIPP_MSM_C"] = c
    try:
        with pytest.raises(ValueError, match="RIPP_MSM_C"): N.msm_g1_batch(bases, sc)
    finally:
        del os.environ["RIPP_MSM_C"]
    got = N.msm_g1_batch(bases, sc)
    assert _same_g1(orc, got, np.stack([orc.msm_g1_a(np.ascontiguousarray(bases), np.ascontiguousarray(sc[r])) for r in range(rows)]))


def test_batch_msm_forced_chunking_gives_the_same_points(engine, orc, N):
    """a low ripp_config.mem_cap_bytes cuts the rows into chunks; the legacy switches select the per-row loop"""
    rows, cols = 64, 16384
    bases = engine.synth_g1(4000, cols); sc = engine.synth_fr(21, rows * cols).reshape(rows, cols, 4)
    whole = N.msm_g1_batch(bases, sc); assert N.msm_batch_chunks() == 1
    engine.release_scratch()
    try:
        engine.configure(mem_cap_bytes=engine.device_bytes() + (96 << 20))
        cut = N.msm_g1_batch(bases, sc); chunks = N.msm_batch_chunks()
    finally:
        engine.configure()
    assert chunks > 1, chunks
    assert _same_g1(orc, cut, whole)
    for switch in ("no_msm_glv", "no_fq", "no_vm"):
        try:
            engine.configure(**{switch: 1})
            legacy = N.msm_g1_batch(bases[:1024], np.ascontiguousarray(sc[:3, :1024])); chunks = N.msm_batch_chunks()
        finally:
            engine.configure()
        assert chunks == 0 and _same_g1(orc, legacy, N.msm_g1_batch(bases[:1024], np.ascontiguousarray(sc[:3, :1024]))), switch


# ---------------------------------------------------------------------------------------------------------------- KZG
@pytest.mark.parametrize("degree", [0, 1, 6, 255])
def test_kzg(engine, orc, P, N, degree):
    """mod.rs:50-119 against the oracle"""
    import poly_commit_oracle as PC
    rng = random.Random(100 + degree)
    alpha, beta = rng.randrange(1, orc.R), rng.randrange(1, orc.R)
    size = max(degree, 7)
    srs = N.KZG.setup(P.frs([alpha])[0], P.frs([beta])[0], size); epowers, ev_ = PC.kzg_setup(alpha, beta, size)
    assert srs.degrees() == (0, size) and np.array_equal(srs.kzg_powers(), epowers)
    v = srs.verifier_key()
    assert _same_g1(orc, v["g_beta"], ev_["g_beta"]) and _same_g2(orc, v["h_alpha"], ev_["h_alpha"]) and _same_g1(orc, v["g"], ev_["g"]) and _same_g2(orc, v["h"], ev_["h"])
    p = [rng.randrange(orc.R) for _ in range(degree + 1)]
    points = [rng.randrange(orc.R), 0]
    if degree:                                                                          # z a root of p: p <- p * (X - root) has the same number of coefficients
        root = rng.randrange(1, orc.R); q = [rng.randrange(orc.R) for _ in range(degree)]
        proot = [(-root * q[0]) % orc.R] + [(q[i - 1] - root * q[i]) % orc.R for i in range(1, degree)] + [q[degree - 1]]
    for poly, zs in ((p, points), (proot, [root]) if degree else (p, [])):
        if not zs:
            continue
        c = P.frs(poly)
        com = N.KZG.commit(srs, c)
        assert _same_g1(orc, com, PC.kzg_commit(epowers, poly))
        # trailing zero coefficients do not change anything (DensePolynomial strips them), even past the number of powers
        assert _same_g1(orc, N.KZG.commit(srs, np.concatenate([c, np.zeros((size + 5, 4), dtype=np.uint64)])), com)
        for z in zs:
            proof, val = N.KZG.open(srs, c, P.frs([z])[0])
            assert _same_g1(orc, proof, PC.kzg_open(epowers, poly, z))
            assert _int(orc, val) == PC.horner(poly, z)
            if poly is not p:
                assert _int(orc, val) == 0
            proof0, val0 = N.KZG.open(srs, np.concatenate([c, np.zeros((3, 4), dtype=np.uint64)]), P.frs([z])[0])
            assert _same_g1(orc, proof0, proof) and np.array_equal(val0, val)
            fz = P.frs([z])[0]
            assert N.KZG.verify(v, com, fz, val, proof) and PC.kzg_verify(ev_, com, z, _int(orc, val), proof)
            assert P.KZG.verify(v, com, z, _int(orc, val), proof)
            assert not N.KZG.verify(v, com, fz, P.frs([_int(orc, val) + 1])[0], proof)
            if degree:                                                                  # a constant evaluates to `val` everywhere
                assert not N.KZG.verify(v, com, P.frs([z + 1])[0], val, proof)
    # more coefficients than powers: RIPP_ERR_ARG where the reference asserts
    with pytest.raises(ValueError):
        N.KZG.commit(srs, P.frs([1] * (size + 2)))
    with pytest.raises(ValueError):
        N.KZG.open(srs, P.frs([1] * (size + 2)), P.frs([5])[0])
    srs.close()


def test_kzg_65535_equals_the_python_path(engine, orc, P, N):
    degree = 65535
    rng = random.Random(7)
    alpha, beta = rng.randrange(1, orc.R), rng.randrange(1, orc.R)
    srs = N.KZG.setup(P.frs([alpha])[0], P.frs([beta])[0], degree)
    powers, v = P.KZG.setup(alpha, beta, degree)
    assert np.array_equal(srs.kzg_powers(), powers)
    c = engine.synth_fr(3, degree + 1); p = _ints(orc, c); z = rng.randrange(orc.R)
    com = N.KZG.commit(srs, c); proof, val = N.KZG.open(srs, c, P.frs([z])[0])
    assert _same_g1(orc, com, P.KZG.commit(powers, p)) and _same_g1(orc, proof, P.KZG.open(powers, p, z))
    assert _int(orc, val) == _horner(orc, p, z)
    assert N.KZG.verify(srs.verifier_key(), com, P.frs([z])[0], val, proof) and P.KZG.verify(v, com, z, _int(orc, val), proof)
    srs.close()


def test_kzg_ragged_scan_sizes(engine, orc, P, N):
    """the quotient scan where a lane owns several chunks and the tail is ragged (msm_batch.hpp: per = ceil(chunks / 256) > 1 with a short last lane, empty lanes
    above it and a last chunk of fewer than 64 coefficients), through the public entry points: p(z) against Python Horner, the proof against the oracle's MSM of the
    Python-integer quotient over the handle's powers (pinned to the oracle by test_kzg)"""
    size = 64 * 513 + 5
    rng = random.Random(513)
    alpha, beta = rng.randrange(1, orc.R), rng.randrange(1, orc.R)
    srs = N.KZG.setup(P.frs([alpha])[0], P.frs([beta])[0], size - 1)
    powers = srs.kzg_powers(); v = srs.verifier_key()
    assert len(powers) == size
    call = engine.synth_fr(41, size); pall = _ints(orc, call)
    for m in (64 * 256 + 1, 64 * 257 + 63, size):
        c, p = np.ascontiguousarray(call[:m]), pall[:m]
        assert p[m - 1] != 0
        com = N.KZG.commit(srs, c)
        for z in (rng.randrange(2, orc.R - 1), orc.R - 1):
            s, acc = [0] * m, 0                                                          # suffix Horner: the quotient is s[1:], p(z) = s[0]
            for k in range(m - 1, -1, -1):
                acc = (acc * z + p[k]) % orc.R; s[k] = acc
            fz = P.frs([z])[0]
            proof, val = N.KZG.open(srs, c, fz)
            assert _int(orc, val) == s[0] == _horner(orc, p, z), (m, hex(z))
            assert _same_g1(orc, proof, orc.msm_g1_a(np.ascontiguousarray(powers[:m - 1]), P.frs(s[1:]))), (m, hex(z))
            assert N.KZG.verify(v, com, fz, val, proof), (m, hex(z))
            assert not N.KZG.verify(v, com, fz, P.frs([(s[0] + 1) % orc.R])[0], proof), (m, hex(z))
    srs.close()


# ---------------------------------------------------------------------------------------------------------------- bivariate
def _cmp_ssm(orc, got, exp):
    assert np.array_equal(got["com_gt"], exp["com_gt"]) and np.array_equal(got["tr"], exp["tr"]) and np.array_equal(got["kzg_c"], exp["kzg_c"])
    assert np.array_equal(got["base_b"], exp["base_b"])
    assert _same_g1(orc, got["com_g1"], exp["com_g1"]) and _same_g1(orc, got["base_a"], exp["base_a"])
    assert _same_g2(orc, got["final_ck_a"], exp["final_ck_a"]) and _same_g2(orc, got["opening_a"], exp["opening_a"])


def _cmp_proof(orc, got, exp):
    _cmp_ssm(orc, got["ip_proof"], exp["ip_proof"])
    assert _same_g1(orc, got["y_eval_comm"], exp["y_eval_comm"]) and _same_g1(orc, got["kzg_proof"], exp["kzg_proof"])


@pytest.mark.parametrize("x_degree,y_degree,n_rows,n_cols", [pytest.param(7, 7, 8, 8, id="7-7-8"), pytest.param(1, 3, 2, 4, id="1-3-2"), pytest.param(3, 15, 3, 16, id="3-15-3"),
                                                            pytest.param(1, 7, 2, 5, id="1-7-2-cols5")])
def test_bivariate_poly_commit(engine, orc, P, N, x_degree, y_degree, n_rows, n_cols):
    """mod.rs:405-443; n_rows < x_degree + 1 exercises the zero-polynomial padding (mod.rs:183-187).  The three cases of the shared commit core: n_cols == y_degree + 1
    (the batched MSM gathers from the handle's resident extended bases), n_cols < y_degree + 1 (it rebuilds them for the shorter rows), n_rows < x_degree + 1 (missing
    rows are the identity)."""
    import poly_commit_oracle as PC
    B = N.BivariatePolynomialCommitment
    rng = random.Random(x_degree * 100 + y_degree)
    alpha, beta = rng.randrange(1, orc.R), rng.randrange(1, orc.R)
    before = engine.device_bytes()
    srs = B.setup(P.frs([alpha])[0], P.frs([beta])[0], x_degree, y_degree); s = PC.bi_setup(alpha, beta, x_degree, y_degree)
    assert srs.degrees() == (x_degree, y_degree) and np.array_equal(srs.kzg_powers(), s["kzg"])
    v_srs = srs.verifier_key()
    ys = [[rng.randrange(orc.R) for _ in range(n_cols)] for _ in range(n_rows)]
    coeffs = np.stack([P.frs(r) for r in ys])
    com, coms = B.commit(srs, coeffs); ecom, ecoms = PC.bi_commit(s, ys)
    assert np.array_equal(com, ecom) and _same_g1(orc, coms, ecoms)
    wide = np.zeros((n_rows, n_cols + 3, 4), dtype=np.uint64); wide[:, :n_cols] = coeffs; wide[:, n_cols:] = 0xABCDEF       # stride > cols: the tail is never read
    com2, coms2 = B.commit(srs, wide[:, :n_cols]); assert np.array_equal(com2, com) and _same_g1(orc, coms2, coms)
    point = (rng.randrange(orc.R), rng.randrange(orc.R)); fpoint = (P.frs([point[0]])[0], P.frs([point[1]])[0])
    proof, val = B.open(srs, coeffs, coms, fpoint); eproof = PC.bi_open(s, ys, ecoms, point)
    _cmp_proof(orc, proof, eproof)                                                         # every member, as test_gpu_poly_commit._cmp_ssm does
    ival = _int(orc, val); assert ival == PC.bi_evaluate(ys, point)
    # two opens in a row on one handle give identical bytes
    proof2, val2 = B.open(srs, wide[:, :n_cols], coms, fpoint)
    assert np.array_equal(val2, val) and all(np.array_equal(proof2["ip_proof"][k], proof["ip_proof"][k]) for k in ("com_gt", "com_g1", "tr", "base_a", "base_b", "final_ck_a", "opening_a", "kzg_c"))
    assert np.array_equal(proof2["y_eval_comm"], proof["y_eval_comm"]) and np.array_equal(proof2["kzg_proof"], proof["kzg_proof"])
    assert B.verify(v_srs, com, fpoint, val, proof)
    assert PC.bi_verify(s["v"], com, point, ival, proof)                                   # the oracle accepts the native proof
    assert B.verify(v_srs, ecom, fpoint, val, eproof)                                      # the native verifier the oracle's
    assert P.BivariatePolynomialCommitment.verify(v_srs, com, point, ival, proof)          # and the Python verifier the native proof
    assert not B.verify(v_srs, com, fpoint, P.frs([ival + 1])[0], proof)
    assert not B.verify(v_srs, com, (P.frs([point[0] + 1])[0], fpoint[1]), val, proof)
    bad = dict(proof); bad["y_eval_comm"] = proof["kzg_proof"]
    assert not B.verify(v_srs, com, fpoint, val, bad)
    with pytest.raises(ValueError):
        B.commit(srs, np.zeros((x_degree + 2, y_degree + 1, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        B.commit(srs, np.zeros((1, y_degree + 2, 4), dtype=np.uint64))
    # memory: the handle and the scratch are all the library held for this
    srs.close(); engine.release_scratch()
    assert engine.device_bytes() <= before, (engine.device_bytes(), before)


def test_memory_returns_to_its_value_before_setup(engine, P, N):
    engine.release_scratch()
    before = engine.device_bytes()
    U = N.UnivariatePolynomialCommitment
    srs = U.setup(P.frs([11])[0], P.frs([13])[0], 1023)
    assert engine.device_bytes() > before
    c = engine.synth_fr(1, 1024); com, coms = U.commit(srs, c); U.open(srs, c, coms, P.frs([99])[0])
    srs.close(); engine.release_scratch()
    assert engine.device_bytes() == before


# ---------------------------------------------------------------------------------------------------------------- univariate
@pytest.mark.parametrize("degree", [56, 1023])
def test_univariate_against_the_oracle(engine, orc, P, N, degree):
    import poly_commit_oracle as PC
    U = N.UnivariatePolynomialCommitment
    rng = random.Random(degree)
    alpha, beta = rng.randrange(1, orc.R), rng.randrange(1, orc.R)
    xd, yd = U.bivariate_degrees(degree)
    srs = U.setup(P.frs([alpha])[0], P.frs([beta])[0], degree); v_srs = srs.verifier_key()
    assert srs.degrees() == (xd, yd)
    p = [rng.randrange(orc.R) for _ in range(degree + 1)]; c = P.frs(p)
    com, coms = U.commit(srs, c)
    z = rng.randrange(orc.R); fz = P.frs([z])[0]
    proof, val = U.open(srs, c, coms, fz)
    ival = _int(orc, val); assert ival == PC.horner(p, z)
    s = PC.bi_setup(alpha, beta, xd, yd); ys = PC.split(p, xd, yd)
    ecom, ecoms = PC.bi_commit(s, ys)
    assert np.array_equal(com, ecom) and _same_g1(orc, coms, ecoms)
    eproof = PC.bi_open(s, ys, ecoms, (pow(z, yd + 1, orc.R), z))
    _cmp_proof(orc, proof, eproof)
    assert U.verify(v_srs, degree, com, fz, val, proof) and not U.verify(v_srs, degree, com, fz, P.frs([ival + 1])[0], proof)
    assert PC.bi_verify(s["v"], com, (pow(z, yd + 1, orc.R), z), ival, proof)
    assert P.UnivariatePolynomialCommitment.verify(v_srs, degree, com, z, ival, proof)
    # trailing zeros, and a polynomial longer than the SRS
    com0, _ = U.commit(srs, np.concatenate([c, np.zeros((9, 4), dtype=np.uint64)])); assert np.array_equal(com0, com)
    with pytest.raises(ValueError):
        U.commit(srs, P.frs([1] * ((xd + 1) * (yd + 1) + 1)))
    srs.close()


def test_univariate_65535_equals_the_python_path_member_for_member(engine, orc, P, N):
    degree = 65535
    U, PU = N.UnivariatePolynomialCommitment, P.UnivariatePolynomialCommitment
    rng = random.Random(degree)
    alpha, beta = rng.randrange(1, orc.R), rng.randrange(1, orc.R)
    assert U.bivariate_degrees(degree) == (15, 4095)
    srs = U.setup(P.frs([alpha])[0], P.frs([beta])[0], degree); psrs = PU.setup(alpha, beta, degree)
    assert np.array_equal(srs.kzg_powers(), psrs[1])
    c = engine.synth_fr(17, degree + 1); p = _ints(orc, c)
    com, coms = U.commit(srs, c); pcom, pcoms = PU.commit(psrs, p)
    assert np.array_equal(com, pcom) and _same_g1(orc, coms, pcoms)
    z = rng.randrange(orc.R)
    proof, val = U.open(srs, c, coms, P.frs([z])[0]); pproof = PU.open(psrs, p, pcoms, z)
    _cmp_proof(orc, proof, pproof)
    ival = _int(orc, val); assert ival == _horner(orc, p, z)
    v_srs = srs.verifier_key()
    assert U.verify(v_srs, degree, com, P.frs([z])[0], val, proof) and PU.verify(psrs[0].get_verifier_key(), degree, com, z, ival, proof)
    psrs[0].close(); srs.close()


def test_univariate_2p20_commit_and_open(engine, orc, P, N):
    degree = (1 << 20) - 1
    U, PU = N.UnivariatePolynomialCommitment, P.UnivariatePolynomialCommitment
    assert U.bivariate_degrees(degree) == (63, 16383)
    srs = U.setup(P.frs([123456789])[0], P.frs([987654321])[0], degree); v_srs = srs.verifier_key()
    c = engine.synth_fr(29, degree + 1)
    com, coms = U.commit(srs, c)
    assert N.msm_batch_chunks() == 1
    z = 0x1234567890ABCDEF1234567890ABCDEF % orc.R
    proof, val = U.open(srs, c, coms, P.frs([z])[0])
    ival = _int(orc, val)
    assert ival == _horner(orc, _ints(orc, c), z)
    assert PU.verify(v_srs, degree, com, z, ival, proof)                                   # the existing Python verifier accepts
    assert not PU.verify(v_srs, degree, com, z, (ival + 1) % orc.R, proof)                 # and rejects value + 1
    assert U.verify(v_srs, degree, com, P.frs([z])[0], val, proof)
    srs.close(); engine.release_scratch()


# ---------------------------------------------------------------------------------------------------------------- BLS12-377
def test_bls12_377_bivariate_equals_the_python_path(engine):
    """bivariate (7, 7) on libripp_hip_377.so: native against the same steps through ripp_amd.bls12_377 (per-row MSMs, AFGHO commitment, TIPAWithSSM, host field arithmetic)"""
    import ripp_amd.bls12_377 as R7
    from ripp_amd.poly_commit import native
    R7.init(0)
    N7 = native.bind(R7.lib); L = R7.lib(); r = R7.R_MOD
    B = N7.BivariatePolynomialCommitment

    def fr(v):
        m = (v % r) * (1 << 256) % r
        return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)

    def frs(vals): return np.stack([fr(v) for v in vals])

    def same_g1(a, b): return np.array_equal(R7.normalize_batch_g1(np.asarray(a).reshape(-1, 18)), R7.normalize_batch_g1(np.asarray(b).reshape(-1, 18)))
    def same_g2(a, b): return np.array_equal(R7.normalize_batch_g2(np.asarray(a).reshape(-1, 36)), R7.normalize_batch_g2(np.asarray(b).reshape(-1, 36)))

    def powers(fn, s, num, width):
        out = np.zeros((num, width), dtype=np.uint64); assert getattr(L, fn)(_p(fr(s)), ctypes.c_size_t(num), _p(out)) == 0; return out

    def msm(bases, coeffs):
        sc = frs(list(coeffs) + [0] * (len(bases) - len(coeffs))); out = np.zeros(18, dtype=np.uint64)
        assert L.ripp_msm_g1_a(_p(bases), _p(sc), ctypes.c_size_t(len(bases)), _p(out)) == 0; return out

    x_degree = y_degree = 7
    rng = random.Random(377)
    alpha, beta = rng.randrange(1, r), rng.randrange(1, r)
    srs = B.setup(fr(alpha), fr(beta), x_degree, y_degree)
    kzg = R7.normalize_batch_g1(powers("ripp_srs_powers_g1", alpha, y_degree + 1, 18))
    assert np.array_equal(srs.kzg_powers(), kzg)
    hbp = powers("ripp_srs_powers_g2", beta, 2 * x_degree + 1, 36); g = powers("ripp_srs_powers_g1", 1, 1, 18)
    ip_srs = R7.SRS(np.repeat(g, len(hbp), axis=0), hbp, powers("ripp_srs_powers_g1", beta, 2, 18)[1], powers("ripp_srs_powers_g2", alpha, 2, 36)[1])
    v = srs.verifier_key(); pv = {"g": g[0], "h": hbp[0], "g_beta": ip_srs.g_beta, "h_alpha": ip_srs.h_alpha}
    assert same_g1(v["g"], pv["g"]) and same_g1(v["g_beta"], pv["g_beta"]) and same_g2(v["h"], pv["h"]) and same_g2(v["h_alpha"], pv["h_alpha"])
    ys = [[rng.randrange(r) for _ in range(y_degree + 1)] for _ in range(x_degree + 1)]
    coeffs = np.stack([frs(row) for row in ys])
    com, coms = B.commit(srs, coeffs)
    ck, _ = ip_srs.get_commitment_keys()
    pcoms = np.stack([msm(kzg, row) for row in ys]); pcom = R7.AFGHOCommitmentG1.commit(ck, pcoms)
    assert same_g1(coms, pcoms) and np.array_equal(np.asarray(com).reshape(-1), np.asarray(pcom).reshape(-1))
    x, y = rng.randrange(r), rng.randrange(r)
    proof, val = B.open(srs, coeffs, coms, (fr(x), fr(y)))
    xp = [pow(x, i, r) for i in range(x_degree + 1)]
    ye = [sum(px * row[j] for px, row in zip(xp, ys)) % r for j in range(y_degree + 1)]
    pip = R7.TIPAWithSSM.prove_with_structured_scalar_message(ip_srs, (pcoms, frs(xp)), (ck,))
    q = [0] * y_degree; carry = 0
    for i in range(y_degree, 0, -1):
        carry = (ye[i] + carry * y) % r; q[i - 1] = carry
    ip = proof["ip_proof"]
    assert np.array_equal(ip["com_gt"], pip["com_gt"]) and np.array_equal(ip["tr"], pip["tr"]) and np.array_equal(ip["kzg_c"], pip["kzg_c"]) and np.array_equal(ip["base_b"], pip["base_b"])
    assert same_g1(ip["com_g1"], pip["com_g1"]) and same_g1(ip["base_a"], pip["base_a"]) and same_g2(ip["final_ck_a"], pip["final_ck_a"]) and same_g2(ip["opening_a"], pip["opening_a"])
    assert same_g1(proof["y_eval_comm"], msm(kzg, ye)) and same_g1(proof["kzg_proof"], msm(kzg, q))
    acc = 0
    for cf in reversed(ye):
        acc = (acc * y + cf) % r
    assert np.array_equal(val, fr(acc))
    assert B.verify(v, com, (fr(x), fr(y)), val, proof)
    assert R7.TIPAWithSSM.verify_with_structured_scalar_message(pv, (com, proof["y_eval_comm"]), fr(x), ip)
    assert not B.verify(v, com, (fr(x), fr(y)), fr(acc + 1), proof)
    ip_srs.close(); srs.close()


# ---------------------------------------------------------------------------------------------------------------- the timing condition
def test_batched_msm_is_not_slower_than_the_loop_it_replaces(engine, orc, N):
    """rows = 64, cols = 16 384 (the univariate split at degree 2^20 - 1): ripp_msm_g1_batch_a against 64 calls of ripp_msm_g1_a, both from host slices
    (bases and scalars uploaded by both), same process and device, medians of 5 after a warm-up"""
    rows, cols = 64, 16384
    bases = engine.synth_g1(31337, cols); sc = np.ascontiguousarray(engine.synth_fr(8, rows * cols).reshape(rows, cols, 4))

    def median_ms(fn):
        fn(); fn()
        ts = []
        for _ in range(5):
            t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
        return sorted(ts)[2]

    t_loop = median_ms(lambda: _msm_loop(engine, bases, sc))
    t_batch = median_ms(lambda: N.msm_g1_batch(bases, sc))
    print(f"\nbatched MSM 64 x 16384: {t_batch:.2f} ms, loop of 64 single MSMs: {t_loop:.2f} ms, ratio {t_loop / t_batch:.2f}")
    assert _same_g1(orc, N.msm_g1_batch(bases, sc), _msm_loop(engine, bases, sc))
    assert t_batch <= t_loop, (t_batch, t_loop)
