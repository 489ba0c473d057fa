"""CPU: the limb-exact model of the field VM interpreter (tests/vm_model.py) against the generator's own evaluation and independent formulas, the
committed headers as the model executes them, every case the GPU module launches (tests/vm_edges.py) with all the model's assertions on, and the margin
of the heavy LIN's float quotient estimate."""
import random

import pytest

import vm_edges as E
import vm_model as M
from vm_model import vmgen

TAGS = ["381", "377"]


def _inputs(c, rng, P):
    return {n: rng.randrange(P) for n in c["ins"]}


@pytest.mark.parametrize("tag", TAGS)
def test_model_agrees_with_generator_and_formulas(tag):
    """random canonical inputs, all seven programs: the model's outputs mod p are vmgen.run_compiled's; line_double, line_add and fp12_mul also equal the
    plain formulas vmgen holds (on the field elements the slots stand for), so model and generator cannot share one mistake"""
    name = M.TAGS[tag]
    C, gen, hdr = M.CURVES[name], E.generator_tables(name), E.header_tables(name)
    rng = random.Random(70)
    for prog in E.PROGS:
        c, h = gen[prog], hdr[prog]
        kinds, ops = M.pack(c["layers"])
        for _ in range(4):
            inp = _inputs(c, rng, C.P)
            ws = [0] * c["nslots"]
            for n, s in c["ins"].items(): ws[s] = inp[n] * C.ONE % C.P          # the slot stands for inp[n]: its R'-form
            out = M.run(C, kinds, ops, ws, columns=True)
            vmgen.set_curve(name)
            try:
                ref = vmgen.run_compiled(c, inp)
            finally:
                vmgen.set_curve("bls12_381")
            assert {n: out[s] * C.RINV % C.P for n, s in c["outs"].items()} == ref, prog
            assert all(out[s] < 2 * C.P for s in c["outs"].values())
            f = E.formula_outputs(name, prog, h, ws)
            assert (f is not None) == (prog in ("line_double", "line_add", "fp12_mul"))
            for s, r in (f or {}).items(): assert out[s] % C.P == r, (prog, s)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("g2", [0, 1], ids=["G1", "G2"])
def test_model_group_law_chains(tag, g2):
    """the hdbl / cadd programs chained as VmCurve<F> chains them (the cases the GPU module launches): identity on either side, T = +-Q, a point of order
    3, Z != 1, 64 doublings, a 64-bit double-and-add chain -- as points against the affine group law of tests/model"""
    n = 0
    for sname, steps, rows in E.curve_cases(tag, g2):
        for cname, T, Q, model, point in rows:
            assert E.affine_of(tag, g2, model) == point, (sname, cname); n += 1
    assert n >= 6 * 8


@pytest.mark.parametrize("tag", TAGS)
def test_committed_header_is_what_the_generator_builds(tag):
    """the parsed header (what the model executes, and what the device harness exports) equals vmgen.validate()'s tables, packed as vmgen.emit packs them"""
    name = M.TAGS[tag]
    gen, hdr = E.generator_tables(name), E.header_tables(name)
    assert set(hdr) == set(gen) == set(E.PROGS)
    for prog, c in gen.items():
        h = hdr[prog]
        kinds, ops = M.pack(c["layers"])
        assert (kinds, ops) == (h["kinds"], h["ops"]) and h["nlayers"] == len(c["layers"]) and h["nslots"] == c["nslots"], prog
        assert h["ins"] == c["ins"] and h["outs"] == c["outs"], prog
        assert M.ops_from_bytes(M.op_bytes(ops)) == ops and len(M.op_bytes(ops)) == 36 * 16 * len(kinds)


def test_contract_checker_refuses_illegal_tables():
    """every launch is guarded by check_contract: it must refuse what the device cannot take"""
    lin = lambda *ops: E.pad(M.LIN, list(ops))
    mul = lambda *ops: E.pad(M.MUL, list(ops))
    tab = lambda layers, nslots=6: dict(layers=layers, nslots=nslots, ins={}, outs={})
    B = {2: 16, 3: 16}
    for c in (tab([lin(E.lin_op(4, [(1, 2)]))]), tab([mul(E.mul_op(5, [2, 3, 2, 3], 0b0101))]), tab([mul(E.mul_op(5, [2, 3, 2, 3], 15))]),
              tab([lin(E.lin_op(4, [(-1, 2)], 16, True))])):
        M.check_contract(c, B)
    illegal = [
        tab([lin(E.lin_op(4, [(2, 2)]))]),                                   # a light total of 32 p
        tab([lin(E.lin_op(4, [(-1, 2)], 15))]),                              # the bias does not cover the negative term
        tab([lin(E.lin_op(4, [(-1, 2)], 16))]),                              # a light total that can be exactly 16 p
        tab([lin(E.lin_op(4, [(127, 2)], 0, True))]),                        # beyond HEAVY_MAX
        tab([lin(E.lin_op(4, [(1, 2)] * 17, 0, True))]),                     # 17 terms
        tab([lin(E.lin_op(4, [(128, 0), (1, 2)]))]),                         # a coefficient beyond COEF_MAX
        tab([lin(E.lin_op(4, [(1, 2)]), E.lin_op(4, [(1, 3)]))]),            # two writers of one slot
        tab([lin(E.lin_op(0, [(1, 2)]))]),                                   # writes the zero slot
        tab([lin(E.lin_op(4, [(1, 1)]))]),                                   # reads the dump slot
        tab([lin(E.lin_op(6, [(1, 2)]))]),                                   # a destination outside the workspace
        tab([lin(E.lin_op(4, [(1, 5)]))]),                                   # reads a slot nobody declared or wrote
        tab([mul(E.mul_op(5, [2, 0, 2, 0], 0b0010))]),                       # a negation on an absent second term
        tab([mul(E.mul_op(5, [2, 0, 2, 0], 16))]),                           # flags beyond the four terms
    ]
    for c in illegal:
        with pytest.raises((AssertionError, KeyError)): M.check_contract(c, B)
    with pytest.raises(AssertionError): M.check_contract(tab([lin(E.lin_op(4, [(0, 2)]))]), {2: 17})          # a slot declared beyond LIGHT_MAX


@pytest.mark.parametrize("tag", TAGS)
def test_every_gpu_case_stays_inside_the_contract(tag):
    """every input set tests/test_gpu_vm_edges.py launches runs through the model first, with the column-wise product walk and all assertions on: the
    reference alone must stay inside the contract on all of them"""
    C = M.CURVES[M.TAGS[tag]]
    st = M.Stats()
    syn = E.synthetic_cases(tag)
    assert {c.name[4:] for c in syn} >= {"lin_light", "mul", "rotation", "lin_heavy_bias_0", "lin_heavy_neg_0"} | {"copy_%d" % n for n in E.COPY_SLOTS} | {"mix_n%d" % n for n in E.WAVE_SHAPES}
    for case in syn:
        assert (case.nslots + case.guard) * 256 * case.waves <= E.LDS_MAX
        case.expected(C, st, columns=True)
    assert st.q_exact > 0 and st.q_short > 0                    # both outcomes of the quotient estimate occur
    assert st.max_mul_col >= 1 << 62 and st.max_lin_col < 1 << 62
    print("BLS12-%s synthetic cases: quotient estimate exact %d / one short %d; largest MUL column 2^%.2f, largest LIN column 2^%.2f"
          % (tag, st.q_exact, st.q_short, _log2(st.max_mul_col), _log2(st.max_lin_col)))
    cases, table = E.production_cases(tag)
    for case in cases: case.expected(C, None, columns=True)
    for prog, row in table.items(): print("  %-12s attained / declared: light LIN %s  MUL operand %s" % (prog, row["light_lin"], row["mul_operand"]))
    for Tin in E.TREE_TINS:
        for r in range(E.TREE_ROWS):
            vals = E.tree_input(C, Tin, r)
            Tout = (Tin + 1) // 2
            for j, w in enumerate(E.tree_expected(tag, vals, Tout)):
                if j + Tout < Tin: assert w == E.tree_formula(tag, vals[j], vals[j + Tout]), (Tin, r, j)


def _log2(x):
    import math
    return math.log2(x) if x else 0.0


@pytest.mark.parametrize("tag,first,reason", [("381", 40324, "top limb leaves 32 bits"), ("377", 18909, "result outside [0, 2p)")])
def test_quotient_estimate_margin(tag, first, reason):
    """the smallest k for which the heavy step leaves [0, 2p) on k p - 1, k p or k p + 1: far above HEAVY_MAX.  On BLS12-381 the top limb of the total
    leaves 32 bits (k = 40 324) before the estimate fails; on BLS12-377 the estimate first falls two short at k = 18 909."""
    C = M.CURVES[M.TAGS[tag]]
    k, why = M.first_failing_k(C, 70000)
    print("BLS12-%s: the heavy step first fails at k = %s (%s)" % (tag, k, why))
    assert k is not None and k > vmgen.HEAVY_MAX
    assert (k, why) == (first, reason)                           # the figures of the docstring, re-derived here
    for kk in range(vmgen.HEAVY_MAX + 1):                        # and every k the contract admits yields q in {k, k - 1} (or the exact floor for the offsets)
        for d in (-1, 0, 1, E.BIG):
            T = kk * C.P + d
            if T >= 0: assert C.quotient_estimate(T >> 364) in (T // C.P, T // C.P - 1)
