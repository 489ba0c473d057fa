"""GPU (-m gpu): bulk validation of untrusted points on the device -- ripp_validate_g1a / ripp_validate_g2a / ripp_vec_validate, the byte readers
ripp_de_g1_vec / ripp_de_g2_vec and ripp_de_groth16_proofs -- on both curves, against flags computed from the DEFINITION by tests/validate_inputs.py
(range, curve equation, [r]P = O in the Python models; never an endomorphism).  Every comparison is exact.

Shapes are the smallest at which the kernels can go wrong: lengths one below, at and above the wave (64) and block (256) sizes with bad points on both
sides of the seams, every small-order and pure-torsion point alone and among valid points (the exceptional-lane path: the fast group law's preconditions
break on exactly these), chunk seams at n = 300 with 128 points per launch, views of resident vectors, strided and tampered byte images."""
import ctypes

import numpy as np
import pytest

import validate_inputs as V

pytestmark = pytest.mark.gpu
LENGTHS = (1, 63, 64, 65, 255, 256, 257)
SZ = ctypes.c_size_t


def P(a): return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module", params=V.TAGS)
def eng(request, engine):
    """(tag, api module, raw library) of one curve"""
    if request.param == "381":
        from ripp_amd._lib import lib
        return "381", engine, lib()
    import ripp_amd.bls12_377 as R7
    R7.init(0)
    return "377", R7, R7.lib()


def validate(R, g, pts): return (R.validate_g1 if g == 1 else R.validate_g2)(pts)


def raw_validate(L, g, pts, with_flags):
    """the C call itself, with or without a flags pointer -> (flags or None, n_bad, first_bad)"""
    n = len(pts); nb, fb = SZ(0), SZ(0)
    flags = np.full(n, 0xEE, dtype=np.uint8) if with_flags else None
    fn = L.ripp_validate_g1a if g == 1 else L.ripp_validate_g2a
    assert fn(P(pts), SZ(n), P(flags) if with_flags else None, ctypes.byref(nb), ctypes.byref(fb)) == 0
    return flags, nb.value, fb.value


@pytest.mark.parametrize("g", (1, 2))
def test_mixed_vectors_at_wave_and_block_seams(eng, g):
    tag, R, L = eng
    for n in LENGTHS:
        pts, want = V.vector(tag, g, n)
        assert want[0] != 0 and want[n - 1] != 0 and all(want[i] != 0 for i in (63, 64, 255, 256) if i < n)
        n_bad, first_bad = V.summary(want)
        flags, nb, fb = raw_validate(L, g, pts, True)
        assert np.array_equal(flags, want), (n, flags.tolist(), want.tolist())
        assert (nb, fb) == (n_bad, first_bad)
        assert raw_validate(L, g, pts, False)[1:] == (n_bad, first_bad)
        f2, nb2, fb2 = validate(R, g, pts)
        assert np.array_equal(f2, want) and (nb2, fb2) == (n_bad, first_bad)
    pts = V.valid(tag, g, 65)                                                  # nothing bad: first_bad = n
    assert raw_validate(L, g, pts, True)[1:] == (0, 65) and raw_validate(L, g, pts, False)[1:] == (0, 65)


@pytest.mark.parametrize("g", (1, 2))
def test_small_order_and_torsion_points_alone_and_among_valid_points(eng, g):
    """the exceptional-lane path: a point with y = 0 doubles to Z = 0, a point of order 3 meets T = -Q at the first addition, the chain of a point of small
    prime order passes through O -- such lanes are redone with the complete formulas and must not report `valid` from an invalid intermediate"""
    tag, R, _ = eng
    cls = V.classes(tag, g)
    hostile = cls["small"] + cls["torsion"]
    base = V.valid(tag, g, 256)
    for raw, want in hostile:
        assert want == V.SUBGROUP
        one = V.rows([raw])
        flags, nb, fb = validate(R, g, one)
        assert (flags.tolist(), nb, fb) == ([want], 1, 0), raw
        v = base.copy(); v[128] = one[0]
        flags, nb, fb = validate(R, g, v)
        assert (nb, fb) == (1, 128) and flags[128] == want and not flags[:128].any() and not flags[129:].any(), raw
    # all of them side by side in one wave, valid points between them
    v = base.copy(); want = np.zeros(256, dtype=np.uint8)
    for k, (raw, f) in enumerate(hostile): v[2 * k + 1] = V.rows([raw])[0]; want[2 * k + 1] = f
    flags, nb, fb = validate(R, g, v)
    assert np.array_equal(flags, want) and (nb, fb) == (len(hostile), 1)


def test_synthetic_points_are_valid(eng):
    _, R, _ = eng
    for g, pts in ((1, R.synth_g1(1000, 1024)), (2, R.synth_g2(2000, 1024))):
        flags, nb, fb = validate(R, g, pts)
        assert not flags.any() and (nb, fb) == (0, 1024)


@pytest.mark.parametrize("g", (1, 2))
def test_chunk_seams(eng, g):
    """n = 300 with 128 points per launch: bad points at 127 | 128 (a chunk seam) and 299 (the last chunk's last lane); the flags equal the unchunked run's.
    The chunk length is set through the library's test hook and restored."""
    tag, R, L = eng
    cls = V.classes(tag, g)
    pts = V.valid(tag, g, 300); want = np.zeros(300, dtype=np.uint8)
    for i, (raw, f) in zip((127, 128, 299), (cls["outside"][0], cls["offcurve"][0], cls["torsion"][0])): pts[i] = V.rows([raw])[0]; want[i] = f
    whole = validate(R, g, pts)
    assert np.array_equal(whole[0], want) and whole[1:] == (3, 127)
    old = L.ripp_validate_set_chunk(SZ(128))
    try:
        assert old == 1 << 20
        cut = validate(R, g, pts)
        v = R.Vec.upload("G1" if g == 1 else "G2", pts)
        cut_vec = R.vec_validate(v); v.close()
        imgs = b"".join((R.ser_g1 if g == 1 else R.ser_g2)(p) for p in pts)
        cut_de = (R.deserialize_g1_vec if g == 1 else R.deserialize_g2_vec)(imgs, compress=False)
    finally:
        assert L.ripp_validate_set_chunk(SZ(0)) == 128
    for got in (cut, cut_vec, cut_de[1:]):
        assert np.array_equal(got[0], whole[0]) and got[1:] == whole[1:]


@pytest.mark.parametrize("g", (1, 2))
def test_resident_vectors_and_views(eng, g):
    """the bad point comes in through the AFFINE upload (a normalising upload could not carry it); first_bad is relative to the view"""
    tag, R, L = eng
    pts = V.valid(tag, g, 100); pts[40] = V.rows([V.classes(tag, g)["outside"][1][0]])[0]
    v = R.Vec.upload("G1" if g == 1 else "G2", pts)
    flags, nb, fb = R.vec_validate(v)
    assert (nb, fb) == (1, 40) and flags[40] == V.SUBGROUP and flags.sum() == V.SUBGROUP
    clean = v[41:]
    flags, nb, fb = R.vec_validate(clean)
    assert len(flags) == 59 and not flags.any() and (nb, fb) == (0, 59)
    inside = v[30:50]
    flags, nb, fb = R.vec_validate(inside)
    assert (nb, fb) == (1, 10) and flags[10] == V.SUBGROUP and flags.sum() == V.SUBGROUP
    nbad, first = SZ(9), SZ(9)                                                 # without a flags pointer
    assert L.ripp_vec_validate(inside._h, None, ctypes.byref(nbad), ctypes.byref(first)) == 0 and (nbad.value, first.value) == (1, 10)
    fr = R.Vec.upload("Fr", np.zeros((4, 4), dtype=np.uint64))
    assert L.ripp_vec_validate(fr._h, None, ctypes.byref(nbad), ctypes.byref(first)) == 4      # RIPP_ERR_ARG for scalars
    for x in (clean, inside, v, fr): x.close()


@pytest.mark.parametrize("compress", (False, True))
@pytest.mark.parametrize("g", (1, 2))
def test_byte_readers_round_trip_stride_and_tampered_images(eng, g, compress):
    tag, R, L = eng
    ser = {(1, False): R.ser_g1, (1, True): R.ser_g1_compressed, (2, False): R.ser_g2, (2, True): R.ser_g2_compressed}[(g, compress)]
    de = R.deserialize_g1_vec if g == 1 else R.deserialize_g2_vec
    pts = V.valid(tag, g, 70); pts[33] = 0                                     # the identity among them
    imgs = [ser(p) for p in pts]; size = len(imgs[0])
    out, flags, nb, fb = de(b"".join(imgs), compress=compress)
    assert np.array_equal(out, pts) and not flags.any() and (nb, fb) == (0, 70)
    stride = size + 13                                                         # a stride larger than the image, junk between the images
    out, flags, nb, fb = de(b"".join(i + b"\xa5" * 13 for i in imgs), compress=compress, n=70, stride=stride)
    assert np.array_equal(out, pts) and not flags.any() and (nb, fb) == (0, 70)
    # one tampered image per class, each between valid ones; the expected flag: the parse reason, or 3 for an image that parses and fails on the device
    cases = [(bytes(img), parse if parse else (0 if ok else V.SUBGROUP)) for c, img, parse, ok in V.tampered_images(tag, g, L) if bool(c) == compress]
    assert sorted({f for _, f in cases}) == [0, 1, 2, 3]
    data, want, ref = [], [], []
    for k, (img, f) in enumerate(cases):
        data += [imgs[k], img]; want += [0, f]; ref += [pts[k], None]
    out, flags, nb, fb = de(b"".join(data), compress=compress)
    assert flags.tolist() == want and (nb, fb) == V.summary(np.array(want))
    for k, (f, r) in enumerate(zip(want, ref)):
        if f: assert not out[k].any()                                          # out[i] = (0, 0) wherever flags[i] != 0
        elif r is not None: assert np.array_equal(out[k], r)
    good = [k for k, f in enumerate(want) if f == 0 and ref[k] is None]        # the untampered images of the list: the valid point and the identity
    assert np.array_equal(out[good[0]], V.rows([V.classes(tag, g)["subgroup"][9][0]])[0]) and not out[good[1]].any()


@pytest.mark.parametrize("compress", (False, True))
def test_groth16_proofs(eng, compress):
    tag, R, L = eng
    import helpers
    if tag == "381":
        import orclib as o
    else:
        import orclib377 as o
    _, _, a, b, c = helpers.fake_groth16(8, 2, 4242, o)
    s1 = R.ser_g1_compressed if compress else R.ser_g1
    s2 = R.ser_g2_compressed if compress else R.ser_g2
    image = lambda bb: b"".join(s1(a[i]) + s2(bb[i]) + s1(c[i]) for i in range(8))
    a2, b2, c2, flags, nb, fb = R.deserialize_groth16_proofs(image(b), compress=compress)
    assert len(image(b)) == 8 * (192 if compress else 384)
    assert np.array_equal(a2, a) and np.array_equal(b2, b) and np.array_equal(c2, c) and flags.shape == (8, 3) and not flags.any() and (nb, fb) == (0, 8)
    if not compress:                                                           # ripp_aggregate_proofs on the arrays read back: unchanged from a direct call
        osrs = helpers.make_srs(8, 0xa1fa, 0xbe7a, o); srs = R.SRS(osrs[0], osrs[1])
        direct, _ = R.aggregate_proofs(srs, a, b, c)
        again, _ = R.aggregate_proofs(srs, a2, b2, c2)
        srs.close()
        for k in ("com_a", "com_b", "com_c", "ip_ab", "r", "ab_kzg_c", "c_base_b", "c_kzg_c"):      # (the projective members are MSM sums whose Z varies run to run)
            assert np.array_equal(direct.field(k), again.field(k)), k
        for k in ("ab_com_steps", "ab_transcript", "c_com_gt", "c_transcript"):
            assert np.array_equal(getattr(direct, k), getattr(again, k)), k
    bad = b.copy(); bad[3] = V.rows([V.classes(tag, 2)["outside"][0][0]])[0]  # B_3: a twist point outside G2
    a2, b2, c2, flags, nb, fb = R.deserialize_groth16_proofs(image(bad), compress=compress)
    assert (nb, fb) == (1, 3) and flags[3].tolist() == [0, 3, 0] and flags.sum() == 3
    assert not b2[3].any() and np.array_equal(np.delete(b2, 3, axis=0), np.delete(b, 3, axis=0)) and np.array_equal(a2, a) and np.array_equal(c2, c)
    nbad, first = SZ(0), SZ(0)                                                 # without a flags pointer
    img = np.frombuffer(image(bad), dtype=np.uint8)
    assert L.ripp_de_groth16_proofs(P(img), SZ(len(img) // 8), SZ(8), int(compress), P(a2), P(b2), P(c2), None, ctypes.byref(nbad), ctypes.byref(first)) == 0
    assert (nbad.value, first.value) == (1, 3)

