"""GPU (-m gpu): the lane-parallel field VM (ripp_amd/csrc/vm.hpp) AT THE BOUNDS OF ITS CONTRACT, through the device harness tests/device/vm_edges.hip
(built from the production headers by build(): tests/device/build/libvm_edges_{381,377}.so).

Every case comes from tests/vm_edges.py, where it was checked against the contract (vm_model.check_contract) and where tests/test_vm_model_cpu.py runs
it through the model with all assertions on; here the device runs it and the WHOLE final workspace (every slot but DUMP_SLOT, every limb) must equal the
model's (tests/vm_model.py: Python integers, the float32 quotient estimate emulated with numpy), the guard slots behind each workspace must come back
untouched, and where a plain formula exists (vmgen's ref_line_double, ref_line_add, f12m; the group law of tests/model) the result must equal it mod p."""
import ctypes
import os

import numpy as np
import pytest

import vm_edges as E
import vm_model as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = ["381", "377"]
U32P = ctypes.POINTER(ctypes.c_uint32)
U8P = ctypes.POINTER(ctypes.c_ubyte)


class Harness:
    def __init__(self, tag):
        path = os.path.join(HERE, "device", "build", "libvm_edges_%s.so" % tag)
        assert os.path.exists(path), "device harness missing: %s (build() builds it: make -C tests/device)" % path
        self.lib = ctypes.CDLL(path)
        self.tag, self.C = tag, M.CURVES[M.TAGS[tag]]
        assert self.lib.ve_curve() == int(tag)
        self.lib.ve_guard_word.restype = ctypes.c_uint32

    def run_table(self, case, fill, n=None):
        """-> (workspaces n x nslots x 14, guards n x guard x 16)"""
        els = case.elements if n is None else case.elements[:n]
        n, ns, g = len(els), case.nslots, case.guard
        assert (ns + g) * 256 * case.waves <= E.LDS_MAX
        kind = (ctypes.c_ubyte * len(case.kinds))(*case.kinds)
        raw = M.op_bytes(case.ops)
        ops = (ctypes.c_ubyte * len(raw)).from_buffer_copy(raw)
        a = np.array([[M.limbs(v) for v in ws] for ws in els], dtype=np.uint32).reshape(n, ns, 14)
        out = np.zeros_like(a); gout = np.zeros((n, max(g, 1), 16), dtype=np.uint32)
        rc = self.lib.ve_run_table(kind, ops, len(case.kinds), ns, g, fill, case.waves, a.ctypes.data_as(U32P), n, out.ctypes.data_as(U32P), gout.ctypes.data_as(U32P))
        assert rc == 0, "ve_run_table returned %d (%s)" % (rc, case.name)
        return out, gout[:, :g, :]

    def export(self, prog):
        hdr = (ctypes.c_int * 4)(); kind = (ctypes.c_ubyte * 64)(); ops = (ctypes.c_ubyte * (64 * 16 * 36))(); io = (ctypes.c_ubyte * 64)()
        rc = self.lib.ve_export(prog, hdr, kind, ops, io)
        assert rc == 0, "ve_export returned %d" % rc
        nl, ns, ni, no = list(hdr)
        return dict(nlayers=nl, nslots=ns, kinds=list(kind)[:nl], ops=M.ops_from_bytes(bytes(ops)[:nl * 16 * 36]), **{"in": list(io)[:ni], "out": list(io)[ni:ni + no]})


@pytest.fixture(scope="module")
def H(engine):
    return {t: Harness(t) for t in CURVES}


def check_case(h, case, fills=(0, 1), expected=None, stats=None):
    """bit for bit: the whole final workspace except DUMP_SLOT, and the guards"""
    want = case.expected(h.C, stats) if expected is None else expected
    for fill in fills:
        out, gout = h.run_table(case, fill)
        for e, ws in enumerate(want):
            for s, v in enumerate(ws):
                if s == M.DUMP_SLOT: continue
                got = [int(x) for x in out[e, s]]
                assert got == M.limbs(v), (case.name, "fill", fill, "element", e, "slot", s, hex(M.value(got)), hex(v))
            for g in range(case.guard):
                assert [int(x) for x in gout[e, g]] == [h.lib.ve_guard_word(e, g, w) for w in range(16)], (case.name, "guard", fill, e, g)
    return want


# ---- a. the interpreter against its contract ------------------------------------------------------------------------------------------------------
def _synthetic(tag, pred):
    return [c for c in E.synthetic_cases(tag) if pred(c.name[4:])]


@pytest.mark.parametrize("tag", CURVES)
def test_lin_light_at_sixteen_p(H, tag):
    for case in _synthetic(tag, lambda n: n == "lin_light"):
        want = check_case(H[tag], case)
        P = H[tag].C.P
        assert want[0][40] == 16 * P - 1 and want[0][41] == 16 * P - 8 and want[0][42] == 16 * P - 1 and want[0][43] == 15 * P       # the edge totals are what the case claims


@pytest.mark.parametrize("tag", CURVES)
def test_lin_heavy_every_multiple_of_p(H, tag):
    """T = k p - 1, k p, k p + 1, k p + 2^364 - 1 for every k < HEAVY_MAX, by the bias and through negative terms.  The device's quotient estimate equals
    the float32 emulation wherever the results are equal bit for bit (a result is T - q p); both outcomes (exact, one short) must occur."""
    h = H[tag]
    st = M.Stats()
    seen = set()
    cases = _synthetic(tag, lambda n: n.startswith("lin_heavy"))
    assert len(cases) >= 20
    for case in cases:
        want = check_case(h, case, stats=st)
        if "bias" in case.name:
            for dst, fl, nb, s, c in case.ops:                     # T = (slot 2: p - 1, 3: 0, 4: 1, 5: 2^364 - 1) + nbias p
                if dst != M.DUMP_SLOT: seen.add((nb + (1 if s[0] == 2 else 0), s[0]))
    assert seen >= {(k, s) for k in range(1, M.vmgen.HEAVY_MAX) for s in (2, 3, 4, 5)}          # every k with all four offsets
    assert max(op[2] for case in cases for op in case.ops) == M.vmgen.HEAVY_MAX and any(op[2] >= 256 for case in cases for op in case.ops)
    print("heavy LIN quotient estimate on BLS12-%s: exact %d, one short %d" % (tag, st.q_exact, st.q_short))
    assert st.q_exact > 0 and st.q_short > 0


@pytest.mark.parametrize("tag", CURVES)
def test_mul_operands_at_their_bounds(H, tag):
    for case in _synthetic(tag, lambda n: n == "mul"):
        st = M.Stats()
        want = case.expected(H[tag].C, st, columns=True)
        check_case(H[tag], case, expected=want)
        P = H[tag].C.P
        assert want[0][68] == M.montgomery(H[tag].C, [2 * k for k in H[tag].C.K17], [2 * k for k in H[tag].C.K17])          # 34 p x 34 p
        assert want[0][71] % P == 0 and want[0][72] % P == 0                                                                 # operands = 0 mod p
        assert st.max_mul_col >= 1 << 62                                                                                       # the 64-bit fit is met, not approached


@pytest.mark.parametrize("tag", CURVES)
def test_read_before_write_rotation(H, tag):
    for case in _synthetic(tag, lambda n: n == "rotation"):
        want = check_case(H[tag], case)
        P = H[tag].C.P
        for ws0, ws in zip(case.elements, want):
            for i in range(16): assert ws[16 + (i + 3) % 16] % P == 3 * ws0[16 + i] % P          # three rotations, the last one times 3


@pytest.mark.parametrize("tag", CURVES)
@pytest.mark.parametrize("nslots", E.COPY_SLOTS)
def test_slot_numbering_and_lds_rotation(H, tag, nslots):
    for case in _synthetic(tag, lambda n: n == "copy_%d" % nslots):
        assert case.guard == (0 if nslots == 255 else 4)
        check_case(H[tag], case)


@pytest.mark.parametrize("tag", CURVES)
@pytest.mark.parametrize("n", E.WAVE_SHAPES)
def test_wave_shapes(H, tag, n):
    for case in _synthetic(tag, lambda nm: nm == "mix_n%d" % n):
        assert len(case.elements) == n
        check_case(H[tag], case)


# ---- b. the production programs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CURVES)
def test_compiled_tables_are_the_committed_header(H, tag):
    hdr = E.header_tables(M.TAGS[tag])
    for pid, prog in enumerate(E.PROGS):
        got = H[tag].export(pid)
        for k in ("nlayers", "nslots", "kinds", "ops", "in", "out"):
            assert got[k] == hdr[prog][k], (prog, k)
    assert H[tag].lib.ve_f12_slots() == hdr["fp12_mul"]["nslots"]
    for g2 in (0, 1):
        assert H[tag].lib.ve_curve_slots(g2) == max(hdr["g%d_hdbl" % (g2 + 1)]["nslots"], hdr["g%d_cadd" % (g2 + 1)]["nslots"])


@pytest.mark.parametrize("tag", CURVES)
def test_production_programs_on_edge_inputs(H, tag):
    h = H[tag]
    name = M.TAGS[tag]
    cases, table = E.production_cases(tag)
    for pid, (prog, case) in enumerate(zip(E.PROGS, cases)):
        got = h.export(pid)
        assert (got["kinds"], got["ops"]) == (case.kinds, case.ops)               # the table the model runs is the one the library holds
        hd = E.header_tables(name)[prog]
        for fill in (0, 1):
            out, _ = h.run_table(case, fill)
            want = case.expected(h.C) if fill == 0 else want
            for e, ws in enumerate(want):
                for s, v in enumerate(ws):
                    if s != M.DUMP_SLOT: assert [int(x) for x in out[e, s]] == M.limbs(v), (prog, fill, e, s)
                ref = E.formula_outputs(name, prog, hd, case.elements[e])
                for s, r in (ref or {}).items():
                    assert M.value(out[e, s]) % h.C.P == r, (prog, "formula", e, s)
    print("attained / declared on BLS12-%s (smallest, largest over the ops of a program):" % tag)
    for prog, row in table.items(): print("  %-12s light LIN %s  MUL operand %s  (%d elements)" % (prog, row["light_lin"], row["mul_operand"], row["elements"]))


def _words(a):
    return [int(x) for x in a]


@pytest.mark.parametrize("tag", CURVES)
@pytest.mark.parametrize("g2", [0, 1], ids=["G1", "G2"])
def test_vm_curve_sequences(H, tag, g2):
    """VmCurve<F>: put -> dbl_ / add_ steps -> get on engine-format values: identity on either side, T = +-Q, a point of order 3, Z != 1, 64 doublings and
    a 64-bit double-and-add chain; bit for bit against the chained model, and as a point against tests/model"""
    h = H[tag]
    C = h.C
    cw = 24 if g2 else 12
    for sname, steps, rows in E.curve_cases(tag, g2):
        a = np.array([E.engine_words(C, T + Q, g2) for _, T, Q, _, _ in rows], dtype=np.uint32)
        out = np.zeros((len(rows), 3 * cw), dtype=np.uint32)
        st = (ctypes.c_ubyte * len(steps))(*steps)
        rc = h.lib.ve_curve_seq(g2, a.ctypes.data_as(U32P), st, len(steps), len(rows), out.ctypes.data_as(U32P))
        assert rc == 0, rc
        for (cname, T, Q, model, point), o in zip(rows, out):
            assert _words(o) == E.engine_words(C, model, g2), (tag, g2, sname, cname)
            assert E.affine_of(tag, g2, model) == point, (tag, g2, sname, cname, "the model against the group law")


# ---- c. k_vm_fp12_tree ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CURVES)
@pytest.mark.parametrize("Tin", E.TREE_TINS)
def test_fp12_tree_level(H, tag, Tin):
    """out[j] = in[j] * in[j + Tout] for j + Tout < Tin, the odd tail copied.  Inputs cross re-sliced (vm.hpp header note): the words of an engine value
    a 2^384 are read as the 2^392-form of a 2^-8, the bilinear product leaves the 2^392-form of (a b 2^-8) 2^-8, whose words are the engine value of
    a b 2^-8 -- the Fp12 product times 2^-8, once per product level (tests/vm_edges.py tree_formula), canonical."""
    h = H[tag]
    Tout, rows = (Tin + 1) // 2, E.TREE_ROWS
    vals = [E.tree_input(h.C, Tin, r) for r in range(rows)]
    buf = np.zeros((rows, 36, Tin, 4), dtype=np.uint32)
    for r in range(rows):
        for j, el in enumerate(vals[r]):
            for k in range(12):
                w = [(el[k] >> (32 * i)) & 0xFFFFFFFF for i in range(12)]
                for c in range(3): buf[r, 3 * k + c, j, :] = w[4 * c:4 * c + 4]
    out = np.zeros((rows, 36, Tout, 4), dtype=np.uint32)
    rc = h.lib.ve_fp12_tree(buf.ctypes.data_as(U32P), Tin, out.ctypes.data_as(U32P), Tout, rows)
    assert rc == 0, rc
    for r in range(rows):
        want = E.tree_expected(tag, vals[r], Tout)
        for j in range(Tout):
            got = tuple(sum(int(x) << (32 * i) for i, x in enumerate(out[r, 3 * k:3 * k + 3, j, :].reshape(12))) for k in range(12))
            assert got == want[j], (tag, Tin, r, j)
            if j + Tout < Tin: assert got == E.tree_formula(tag, vals[r][j], vals[r][j + Tout]), (tag, Tin, r, j, "formula")
