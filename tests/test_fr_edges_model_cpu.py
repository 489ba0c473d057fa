"""CPU: the case lists and the Python model of tests/fr_edges.py, which tests/test_gpu_fr_edges.py holds the device code to.

  * the constants agree with the build's parameter headers (read here only to compare) and the operand lists hold what they promise;
  * products (and mul2_add) reach both sides of reduce_once's branch, at least 20 cases each per field and curve;
  * the Barrett estimate of msm_divmod is exact for some k of the list and one short for others, at least 20 of each per divisor, and never two short;
  * the restatement of the three KZG scan kernels equals suffix Horner on the whole size / lane-share / point / polynomial list;
  * the digit model reconstructs every component for every window width a plan can have."""
import pytest

import fr_edges as E
import fold_edge_scalars as FES

TAGS = E.TAGS


@pytest.mark.parametrize("tag", TAGS)
def test_constants_match_the_build(tag):
    C = E.CURVES[tag]
    r, u, lam = FES.params(tag)
    assert (C.r, C.x, C.lam) == (r, u, lam)
    assert 2 * C.r < 1 << 256 and 2 * C.p < 1 << 384
    assert (4 * C.r < 1 << 256) == (tag == "377")                          # Fr of BLS12-381 has ONE spare bit
    assert C.lam < 1 << 128 and (C.r - 1) // C.lam < 1 << 128 and C.x < 1 << 64 and C.r < C.x**4


@pytest.mark.parametrize("fname", ["fr", "fp"])
@pytest.mark.parametrize("tag", TAGS)
def test_operand_list(tag, fname):
    F = E.CURVES[tag].field(fname)
    m, ops = F.m, E.operands(tag, fname)
    assert all(0 <= v < m for v in ops) and len(E.randoms(tag, fname)) == 200
    for v in (0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, F.R % m, F.R * F.R % m):
        assert v in ops
    for k in range(1, F.N):
        assert (1 << (32 * k)) in ops and (1 << (32 * k)) - 1 in ops       # every limb boundary lies below both moduli
    ones = [v for v in ops if v & ((1 << (32 * (F.N - 1))) - 1) == (1 << (32 * (F.N - 1))) - 1]
    assert ones and max(ones) + (1 << (32 * (F.N - 1))) >= m
    sums = {a + b for a, b in E.add_cases(tag, fname)}
    assert {m - 1, m, m + 1, 2 * m - 2} <= sums
    subs = set(E.sub_cases(tag, fname))
    assert {(0, m - 1), (m - 1, 0), (m - 1, m - 1), (0, 0), (m - 2, m - 1), (0, 1)} <= subs
    for cases in (E.mul_cases(tag, fname), E.add_cases(tag, fname), E.sub_cases(tag, fname)):
        assert all(0 <= v < m for c in cases for v in c)


@pytest.mark.parametrize("fname", ["fr", "fp"])
@pytest.mark.parametrize("tag", TAGS)
def test_products_take_both_reduction_branches(tag, fname):
    F = E.CURVES[tag].field(fname)
    lo, hi = E.branch_counts(tag, fname, E.mul_cases(tag, fname))
    print("mul %s %s: t < m %d, t >= m %d" % (tag, fname, lo, hi))
    assert lo >= 20 and hi >= 20
    for a, b in E.mul_cases(tag, fname)[::37]:                              # the model's product is the reduced t
        t = F.redc_t(a * b)
        assert (t - F.m if t >= F.m else t) == E.expect(tag, fname, "mul", (a, b))
    if fname == "fp":
        cases = E.mul2_cases(tag)
        assert all(0 <= v < F.m for c in cases for v in c)
        lo, hi = E.branch_counts(tag, fname, cases)
        print("mul2_add %s: t < m %d, t >= m %d" % (tag, lo, hi))
        assert lo >= 20 and hi >= 20
        for c in cases[::17]:
            t = F.redc_t(c[0] * c[1] + c[2] * c[3])
            assert (t - F.m if t >= F.m else t) == E.expect(tag, fname, "mul2_add", c)


@pytest.mark.parametrize("which", ["lambda", "x"])
@pytest.mark.parametrize("tag", TAGS)
def test_barrett_estimates(tag, which):
    C, d = E.CURVES[tag], E.divisor(tag, which)
    ks = E.divmod_cases(tag)
    for j in (1, 2, 3, C.r // d):
        assert j * d in ks and j * d - 1 in ks
    assert C.r - 1 in ks and all(v % C.r in ks for v in FES.scalars(tag)) and all(v in ks for v in E.operands(tag, "fr"))
    short = [E.barrett_shortfall(k, d) for k in ks]
    print("divmod %s %s: exact %d, one short %d" % (tag, which, short.count(0), short.count(1)))
    assert set(short) <= {0, 1}, "a k of the list needs two corrections"
    assert short.count(0) >= 20 and short.count(1) >= 20
    assert all(E.barrett_shortfall(j * d, d) == 1 for j in (1, 2, 3, C.r // d))
    if which == "x":                                                       # the later steps of the chain divide quotients: same bound
        for k in ks:
            for q, _ in E.x_chain(tag, k)[:2]:
                assert E.barrett_shortfall(q, d) in (0, 1)
            digits = [rem for _, rem in E.x_chain(tag, k)] + [E.x_chain(tag, k)[2][0]]
            assert digits == E.components(tag, k, 4) and all(v < 1 << 64 for v in digits)


@pytest.mark.parametrize("tag", TAGS)
def test_scan_points(tag):
    r = E.CURVES[tag].r
    z64, z128 = E.scan_point(tag, "order64"), E.scan_point(tag, "order128")
    assert pow(z64, 64, r) == 1 and pow(z64, 32, r) == r - 1 and pow(z128, 64, r) == r - 1
    assert len({E.scan_point(tag, n) for n in E.SCAN_POINTS_ALL}) == 7


@pytest.mark.parametrize("case", E.scan_cases(), ids=lambda c: "m%d_per%d" % (c[0], c[1]))
@pytest.mark.parametrize("tag", TAGS)
def test_scan_model_is_suffix_horner(tag, case):
    m, per, points = case
    r = E.CURVES[tag].r
    for zn in points:
        z = E.scan_point(tag, zn)
        for kind in E.SCAN_POLYS:
            p = E.scan_poly(tag, m, kind, z)
            assert len(p) == m and all(0 <= v < r for v in p)
            s = E.suffix_horner(p, z, r)
            h, cin, q, ev = E.scan_model(p, z, r, per)
            assert q == s[1:] and ev == s[0], (tag, m, per, zn, kind)
            assert cin == [s[(c + 1) * 64] if (c + 1) * 64 < m else 0 for c in range(len(cin))]
            if kind == "root": assert ev == 0
            if kind == "top_only": assert ev == p[-1] * pow(z, m - 1, r) % r


def test_scan_case_list():
    cases = E.scan_cases()
    assert [c[0] for c in cases if c[1] == 0] == E.SCAN_SIZES and [(c[0], c[1]) for c in cases if c[1]] == E.SCAN_OVERRIDES
    ragged = []
    for m, per, _ in cases:
        nchunk = -(-m // 64)
        per = per or -(-nchunk // 256)
        if per > 1 and (nchunk % per or nchunk < 256 * per) and m % 64: ragged.append(m)      # a short last lane or empty lanes, and a short last chunk
    assert ragged, "no size with per > 1 and a ragged tail"


@pytest.mark.parametrize("split", [1, 2, 4])
@pytest.mark.parametrize("tag", TAGS)
def test_digit_model(tag, split):
    C = E.CURVES[tag]
    ks = list(E.divmod_cases(tag)) + E.digit_scalars(tag, 40, 1)
    assert 0 in E.digit_scalars(tag, 2, 0) and C.r - 1 in E.digit_scalars(tag, 1, 0)
    nbits = E.NBITS[split]
    for c in range(4, 14):
        nwin = (nbits + c - 1) // c
        plan = {"c": c, "nwin": nwin, "nb": 1 << c, "n": split * 3, "nreal": 3}
        E.check_plan(plan, split, 3)
        for k in ks:
            E.check_digit_model(tag, k, split, plan)
    plan = {"c": 5, "nwin": (nbits + 4) // 5, "nb": 32, "n": split * 3, "nreal": 3}
    placement = {(0, 0): C.r - 1, (1, 2): C.lam}
    dg = E.expected_digits(tag, plan, split, 2, placement)
    assert len(dg) == 2 * plan["nwin"] * plan["n"]
    for row, pos, k in ((0, 0, C.r - 1), (1, 2, C.lam)):                     # read the buffer back the way the pipeline indexes it
        for j, v in enumerate(E.components(tag, k, split)):
            assert sum(dg[(row * plan["nwin"] + w) * plan["n"] + j * 3 + pos] << (5 * w) for w in range(plan["nwin"])) == v
    assert sum(1 for d in dg if d) == sum(1 for k in placement.values() for v in E.components(tag, k, split) for d in E.windows(v, 5, plan["nwin"]) if d)
    h = E.histogram(plan, dg[:plan["nwin"] * plan["n"]])
    assert sum(h) == sum(1 for d in dg[:plan["nwin"] * plan["n"]] if d) and all(h[w * 32] == 0 for w in range(plan["nwin"]))
