"""CPU: the models of the device inversions (tools/inv_model.py: fp_inv_bingcd with its float32 tail, fp_inv_kaliski) over the edge list of
tests/inv_edges.py, on both primes, with every model assertion on; and the BLS12-377 table of Kaliski corrections.  tests/test_gpu_inv_edges.py runs
the device code on the same list."""
import os

import pytest

import inv_edges as E
import inv_model as IM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag", E.TAGS)
def test_edge_list_is_what_it_says(tag):
    C = IM.CURVES[tag]
    p, vals = C.P, E.values(tag)
    assert all(0 <= v < p for v in vals) and len(set(E.structured(tag))) == len(E.structured(tag))
    assert 3300 <= len(vals) <= 3500 and len(E.randoms(tag)) == 1000 and vals[-1000:] == E.randoms(tag)
    have = set(vals)
    assert {0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2, p // 3, 2 * p // 3} <= have
    for k in range(C.BITS):
        for d in (-1, 0, 1):
            assert all(v in have for v in ((1 << k) + d, p - (1 << k) + d) if 0 < v < p)
    assert {(1 << k) - 1 for k in E.WINDOW_SWITCHES} <= have
    for s in list(range(1, 20)) + [p - 1, p - 2]:
        assert {s * pow(2, e, p) % p for e in (384, -384, 392, -392)} <= have
    assert set(E.full_run(tag)) <= have


@pytest.mark.parametrize("tag", E.TAGS)
def test_bingcd_model_inverts_the_whole_list(tag):
    """every value, through the 26 outer iterations and the float32 tail, with the model's assertions on (window form, factor and column bounds, exact
    division, |u|, |v| < 64 p, a = 0 and b = 1, top limb < 2^24, 0 <= r < 2p); the list meets all three window forms"""
    C = IM.CURVES[tag]
    assert C.ITER == 26
    tr, stats = E.traces(tag)
    for y, (x, needed) in zip(E.values(tag), tr):
        assert x == (pow(y, -1, C.P) if y else 0), hex(y)
        assert IM.device_result(x, tag) == E.expected(tag, y)
        assert needed <= C.ITER and (needed == 0) == (y == 0)
    assert stats["forms"] == {"exact56", "exact64", "top34"}
    assert stats["uv"] < 64 and stats["r"] < 2 and stats["top"] < 1 << 24


@pytest.mark.parametrize("tag", E.TAGS)
def test_only_structured_inputs_need_every_iteration(tag):
    """Outer iterations until a = 0, counted by the model.  BLS12-381: the 1 000 random values need 17-20, the list has 22 values that need all 26
    (2^k and p - 2^k, 370 <= k <= 380).  BLS12-377: random 17-19, 6 values need all 26 (374 <= k <= 376).  So the last iterations, the iteration count
    and the small-value windows of the last passes are reached by the structured values alone."""
    C = IM.CURVES[tag]
    tr, _ = E.traces(tag)
    vals = E.values(tag)
    full = [y for y, (_, needed) in zip(vals, tr) if needed == C.ITER]
    assert len(full) >= 1 and sorted(full) == sorted(E.full_run(tag))
    assert len(full) == {"381": 22, "377": 6}[tag]
    rnd = [needed for _, needed in tr[-E.N_RANDOM:]]
    assert max(rnd) < C.ITER and 17 <= min(rnd) and max(rnd) <= 20


@pytest.mark.parametrize("tag", E.TAGS)
def test_one_iteration_fewer_fails_on_the_list(tag):
    """the model run with ITER - 1 outer iterations: a != 0 on every full-run value (its assertion fires), while the random values still pass -- what a
    device loop one iteration short would do, and why random inputs cannot see it"""
    C = IM.CURVES[tag]
    for y in E.full_run(tag):
        with pytest.raises(AssertionError, match="a != 0"):
            IM.inv_trace(y, tag, iters=C.ITER - 1)
    for y in E.randoms(tag)[:20]:
        assert IM.inv_trace(y, tag, iters=C.ITER - 1)[0] == pow(y, -1, C.P)


@pytest.mark.parametrize("tag", E.TAGS)
def test_kaliski_model_inverts_the_whole_list(tag):
    """fp_inv_kaliski's model: BITS <= k <= 2 BITS - 1 <= 768 and r < 2p (asserted inside), result = y^-1.  The list reaches k = BITS (1, 5, ...) and
    k = 2 BITS - 1 (2^(BITS-1)): 761 on BLS12-381, 753 on BLS12-377; the random values stay within 492..584."""
    C = IM.CURVES[tag]
    ks = E.kaliski_steps(tag)
    for y, k in zip(E.values(tag), ks):
        k2, x = IM.kaliski(y, tag)
        assert k2 == k and x == (pow(y, -1, C.P) if y else 0), hex(y)
    live = [k for y, k in zip(E.values(tag), ks) if y]
    assert min(live) == C.BITS and max(live) == 2 * C.BITS - 1 == {"381": 761, "377": 753}[tag]
    assert ks[E.values(tag).index(1)] == C.BITS and ks[E.values(tag).index(1 << (C.BITS - 1))] == 2 * C.BITS - 1


def test_kaliski_fix_table_377():
    """KALISKI_FIX[k] = R^3 2^-k mod p of bls12_377/inv_table.inc: the rows test_kaliski_fix_table (tests/test_vmgen_cpu.py) checks on the BLS12-381 table,
    at this curve's k = BITS, and every other row as well"""
    p = IM.CURVES["377"].P
    R = 1 << 384
    rows = [l for l in open(os.path.join(ROOT, "ripp_amd", "csrc", "bls12_377", "inv_table.inc")) if l.startswith("{")]
    assert len(rows) == 769
    table = []
    for row in rows:
        limbs = [int(x.rstrip("u"), 16) for x in row.strip().rstrip(",").strip("{}").split(",")]
        assert len(limbs) == 12 and all(0 <= v < 1 << 32 for v in limbs)
        table.append(sum(v << (32 * i) for i, v in enumerate(limbs)))
    for k in (0, 1, 377, 381, 500, 768):
        assert table[k] == pow(R, 3, p) * pow(2, -k, p) % p
    assert table == [pow(R, 3, p) * pow(2, -k, p) % p for k in range(769)]
    # and the algorithm with this table, as the device applies it: x = p - r, one Montgomery product with row k
    for y in [1, 2, p - 1] + list(E.randoms("377")[:50]):
        k, x = IM.kaliski(y, "377")
        almost = x * pow(2, k, p) % p                                  # p - r
        assert almost * table[k] * pow(R, -1, p) % p == E.expected("377", y)
