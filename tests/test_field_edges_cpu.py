"""CPU checks of tests/field_edges.py: the largest-limb generator, the legality of every case list the GPU harness test feeds (tests/test_gpu_field_edges.py),
the replayed column sums of k_line_products_k against the models' f12mul, and the float quotient estimate of fq_reduce at every value bound."""
import random

import numpy as np
import pytest

import field_edges as F

VMAX = 2500


@pytest.mark.parametrize("LM", [F.L28, (1 << 29) - 1, 1 << 29, 3 * F.L28 - 1, 4 * (F.L28 - 1) + 1, 14 * F.L28 - 13, F.LWIDE])
def test_largest_limbs(LM):
    rng = random.Random(LM)
    for tag in ("381", "377"):
        P = F.CURVES[tag].P
        for v in [0, 1, P - 1, P, 2 * P - 1, 36 * P - 1, 258 * P - 1] + [rng.randrange(2500 * P) for _ in range(50)]:
            l = F.largest_limbs(v, LM)
            assert F.value(l) == v and all(0 <= x < LM for x in l[:13])
            rest = v
            for i in range(13):                          # maximal: the next admissible limb value (+ 2^28) would pass LM or what is left
                assert l[i] % F.L28 == rest % F.L28 and (l[i] + F.L28 >= LM or l[i] + F.L28 > rest)
                rest = (rest - l[i]) >> F.W
            if LM == F.L28:
                assert l == F.to_limbs(v)


def _dot_fits(nt, L1, L2):
    return nt * 14 * (L1 - 1) * (L2 - 1) + 14 * (1 << 56) + (1 << 37) < (1 << 64)


def test_tables_are_legal_types():
    """every instantiation of the harness satisfies the static checks of fq28.hpp, so it compiles for the reason the engine's types do"""
    for LM, VB in F.REDUCE + F.SUB + F.SQR:
        assert LM <= 1 << 32 and 1 <= VB <= VMAX
    for LM, VB in F.REDUCE:
        assert LM <= F.LWIDE
    for (L1, V1), (L2, V2) in F.MUL:
        assert _dot_fits(1, L1, L2) and V1 * V2 <= VMAX
    for L1, V1 in F.SQR:
        assert _dot_fits(1, L1, L1) and L1 <= 1 << 31 and V1 * V1 <= VMAX
    for nt, tab in ((2, F.DOT2), (4, F.DOT4)):
        for (L1, V1), (L2, V2) in tab:
            assert _dot_fits(nt, L1, L2) and nt * V1 * V2 <= VMAX


@pytest.mark.parametrize("tag", ["381", "377"])
def test_case_lists_respect_bounds(tag):
    """every operand the GPU test builds passes check_type for its instantiation (the builders assert it; this runs them all without a device)"""
    C = F.CURVES[tag]
    rng = random.Random(3)
    for LM, VB in F.REDUCE:
        for _, _, v in F.reduce_inputs(C, VB):
            F.operand(C, v, LM, VB)
            F.check_type(F.to_limbs(v), LM, VB, C.P)
    for L2, V2 in F.SUB:
        b = F.subtrahend_max(C, L2, V2)
        assert b[:13] == [L2 - 1] * 13 and F.value(b) < V2 * C.P <= F.value(b) + (1 << 364)
    ops = [t for pair in F.MUL + F.DOT2 + F.DOT4 + F.F2MUL[tag] + F.F2MULFQ for t in pair] + F.SQR + F.F2SQR[tag]
    ops += [t for q in F.MULSUB + F.F2MULSUB[tag] for t in q]
    for LM, VB in ops:
        for v in F.edge_values(C, VB) + [rng.randrange(VB * C.P)]:
            F.operand(C, v, LM, VB)
    for v in F.storage_values(C, rng):
        assert 0 <= v < C.P
    for M, T, rows in F.LP_SHAPES:
        for row in F.lp_lines(C, M, rows, 1):
            assert len(row) == M and all(0 <= c < C.P for line in row for c in line)


def _reduce_estimate_ok(C, v):
    """fq_reduce's quotient estimate in float32 (fq_curve.hpp): the result v - q p must lie in [0, 2p)"""
    inv = np.float32(np.float32(1.0) - np.float32(1.0) / np.float32(1048576.0)) / np.float32(C.P_TOP + 1)
    q = int(np.float32(np.float32(v >> 364) * inv))
    return 0 <= v - q * C.P < 2 * C.P


@pytest.mark.parametrize("tag", ["381", "377"])
def test_reduce_estimate_margin(tag):
    """the estimate is never too large and at most one too small at every value bound the harness instantiates (up to VMAX p, largest 2500), and the
    first failing bound lies far above VMAX: found by a scan of k p - 1, k p, k p + 2^364 - 1"""
    C = F.CURVES[tag]
    for k in range(1, VMAX + 1):
        for v in (k * C.P - 1, k * C.P, k * C.P + 1, k * C.P + (1 << 364) - 1):
            assert _reduce_estimate_ok(C, v), (tag, k)
    limit = (1 << 31) // (C.P_TOP + 1)                   # fq_reduce's own static check: VB (P_TOP + 1) < 2^31
    first_bad = next((k for k in range(VMAX, limit) if not all(_reduce_estimate_ok(C, v) for v in (k * C.P - 1, k * C.P, k * C.P + (1 << 364) - 1))), None)
    print("fq_reduce estimate BLS12-%s: first failing multiple of p: %s (VMAX = %d, static limit %d)" % (tag, first_bad, VMAX, limit))
    assert first_bad is None or first_bad > 4 * VMAX


def test_line_products_k_model_matches_f12mul():
    """the replayed signed column sums of k_line_products_k give the models' sparse Fp12 product on every stage-2a case of the GPU test; the largest
    |column| (reached by the extreme sequences, F.lp_extreme_sequences) and the range of the reduced values are the margins of the kernel's int64 columns
    and of its (-0.01 p, 1.01 p) claim"""
    C = F.CURVES["381"]
    st = F.LkStats()
    for si, (M, T, rows) in enumerate(F.LP_SHAPES):
        lines = F.lp_lines(C, M, rows, seed=100 + si)
        for r in range(rows):
            for tt in range(T):
                ls = [lines[r][i] for i in range(tt, M, T)]
                assert F.lk_model(C, ls, st) == F.expected_accumulator(C, ls), (M, T, rows, r, tt)
    for seed in F.LP_HIGH_SEEDS:
        ls, fin = F.lp_high_lines(C, seed), []
        assert F.lk_model(C, ls, st, fin) == F.expected_accumulator(C, ls)
        assert max(fin) >= C.P, seed                     # a final value in [p, 1.01 p): the write-out's second subtraction of p is needed
    rest = st.col_max
    for name, ls in F.lp_extreme_sequences(C).items():
        assert F.lk_model(C, ls, st) == F.expected_accumulator(C, ls), name
    print("k_line_products_k: largest |int64 column| = 2^%.3f (2^%.3f without the extreme sequences), reduced values in (%.6f p, %.6f p)"
          % (np.log2(float(st.col_max)), np.log2(float(rest)), st.vmin, st.vmax))
    assert st.col_max < 1 << 63
    assert st.col_max > rest                             # the extreme sequences are the probe of the column margin
    assert -0.01 < st.vmin and st.vmax < 1.01
