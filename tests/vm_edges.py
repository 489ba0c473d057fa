"""Cases for the device harness tests/device/vm_edges.hip (TEST INFRASTRUCTURE ONLY): tables and workspaces at the bounds the field VM's contract
admits (tools/vmgen.py: TMAX, COEF_MAX, BOUND_IN, LIGHT_MAX, HEAVY_MAX, NEG_K, VMAX), the production programs on edge inputs, VmCurve<F> step
sequences and k_vm_fp12_tree inputs.

Both tests/test_vm_model_cpu.py and tests/test_gpu_vm_edges.py take their cases from here: the CPU test runs every case through the model
(tests/vm_model.py) with all its assertions on, the GPU test launches the same cases and compares bit for bit.  A table is checked against the
contract (vm_model.check_contract) where it is built, so an illegal table is an assertion here and never a launch.
"""
import functools
import os
import random

import vm_model as M
from vm_model import MUL, LIN, G, vmgen

ROOT = M.ROOT
PROGS = ["fp12_mul", "g1_cadd", "g1_hdbl", "g2_cadd", "g2_hdbl", "line_add", "line_double"]          # the harness's program ids, in this order
BIG = (1 << 364) - 1
LDS_MAX = 65536


class Case:
    """one launch: a packed table, the initial workspaces of n elements, the launch shape"""

    def __init__(self, name, layers, nslots, in_bounds, elements, guard=4, decl=None, kinds=None, ops=None):
        self.name, self.nslots, self.elements = name, nslots, elements
        if layers is not None:
            c = dict(layers=layers, nslots=nslots, ins={}, outs={})
            self.decl = M.check_contract(c, in_bounds)
            self.kinds, self.ops = M.pack(layers)
        else:
            self.decl, self.kinds, self.ops = decl, kinds, ops
        self.in_bounds = in_bounds
        for ws in elements:
            assert len(ws) == nslots and ws[0] == 0
            for s, v in enumerate(ws):
                if s >= 2: assert 0 <= v < max(in_bounds.get(s, 0), 0) * M.CURVES[self.curve_of(name)].P or v == 0, (name, s)
        self.guard = guard if (nslots + guard) * 256 <= LDS_MAX else 0
        self.waves = min(4, LDS_MAX // ((nslots + self.guard) * 256))
        assert self.waves >= 1

    @staticmethod
    def curve_of(name): return "bls12_377" if name.startswith("377") else "bls12_381"

    def expected(self, C, stats=None, columns=False):
        return [M.run(C, self.kinds, self.ops, ws, self.decl, stats, columns) for ws in self.elements]


def lin_op(dst, terms, nbias=0, heavy=False): return dict(dst=dst, terms=list(terms), nbias=nbias, heavy=heavy)
def mul_op(dst, a, neg=0): return dict(dst=dst, a=list(a), neg=neg)


def pad(kind, row):
    row = list(row)
    while len(row) < G:
        row.append(mul_op(M.DUMP_SLOT, [0] * 4) if kind == MUL else lin_op(M.DUMP_SLOT, []))
    assert len(row) == G
    return (kind, row)


def ones13(C, b): return (((b * C.P) >> 364) << 364) - 1       # the largest value < b p whose 13 low limbs are all 2^28 - 1
def zeros13(C, b): return ((b * C.P) >> 364) << 364            # the largest value < b p whose 13 low limbs are all 0


def elements_from(C, nslots, edge, bounds, n_random, seed):
    """element 0: the edge values; then workspaces with every input slot random below its declared bound"""
    rng = random.Random(seed)
    out = []
    for e in range(1 + n_random):
        ws = [0] * nslots
        for s, b in bounds.items():
            ws[s] = edge[s] if e == 0 else (rng.randrange(b * C.P) if b else 0)
        out.append(ws)
    return out


# ---- a. synthetic tables --------------------------------------------------------------------------------------------------------------------------
def case_lin_light(C, pre):
    P = C.P
    edge = {2: 16 * P - 1, 3: 2 * P - 1, 4: 15 * P - 1, 5: 0, 6: 0, 7: 0, 24: ones13(C, 16), 25: zeros13(C, 16), 26: ones13(C, 8), 27: 5 * P - 1, 28: 3 * P - 1}
    bounds = {2: 16, 3: 2, 4: 15, 5: 1, 6: 1, 7: 1, 24: 16, 25: 16, 26: 8, 27: 5, 28: 3}
    for s in range(8, 24): edge[s], bounds[s] = P - 1, 1
    rows = [
        [(1, 2)],                                        # 16p - 1, one term
        [(8, 3)],                                        # 8 (2p - 1)
        [(1, 4), (-1, 5)],                               # mixed signs, the smallest covering bias: 15p - 1 - 0 + p
        [(-5, 5), (-5, 6), (-5, 7)],                     # all negative on zero slots: exactly nbias p
        [(1, s) for s in range(8, 24)],                  # 16 terms
        [(127, 0), (-127, 0), (1, 2)],                   # the extreme coefficients (a light total admits them on the zero slot only)
        [(1, 24)], [(1, 25)], [(2, 26)],                 # limb patterns: 13 low limbs all ones / all zero
        [(3, 28), (-2, 3), (1, 28)],
        [(-1, 4)],                                       # 15 p - (15 p - 1) = 1
        [(16, 8)],
        [(7, 3), (-1, 5), (-1, 6)],
        [(1, 3), (1, 27), (1, 26)],
        [(4, 3), (-1, 26)],
        [(15, 8), (-1, 9)],
    ]
    ops = []
    for i, terms in enumerate(rows):
        neg = sum(-c * (bounds[s] if s else 0) for c, s in terms if c < 0)
        ops.append(lin_op(40 + i, terms, neg))
    return Case(pre + "lin_light", [pad(LIN, ops)], 56, bounds, elements_from(C, 56, edge, bounds, 3, 21))


def cases_lin_heavy_bias(C, pre):
    """T = k p - 1, k p, k p + 1, k p + 2^364 - 1 for every k in [0, HEAVY_MAX): one term of coefficient 1 on a slot holding p - 1, 0, 1 or 2^364 - 1
    plus nbias = k - 1 or k (pos + nbias <= HEAVY_MAX admits nbias up to 999).  Lane 15 of every layer is a small op (q = 0): the flag is per layer."""
    P = C.P
    edge = {2: P - 1, 3: 0, 4: 1, 5: BIG}
    bounds = {2: 1, 3: 1, 4: 1, 5: 1}
    todo = []
    for k in range(vmgen.HEAVY_MAX):
        if k >= 1: todo.append((2, k - 1))
        todo += [(3, k), (4, k), (5, k)]
    cases = []
    per_table = 15 * 15
    for t0 in range(0, len(todo), per_table):
        layers, dst = [], 6
        chunk = todo[t0:t0 + per_table]
        for l0 in range(0, len(chunk), 15):
            row = []
            for src, nb in chunk[l0:l0 + 15]:
                row.append(lin_op(dst, [(1, src)], nb, True)); dst += 1
            while len(row) < 15: row.append(lin_op(M.DUMP_SLOT, []))
            row.append(lin_op(dst, [(1, 4)], 0, False)); dst += 1
            layers.append((LIN, row))
        cases.append(Case(pre + "lin_heavy_bias_%d" % (t0 // per_table), layers, dst, bounds, elements_from(C, dst, edge, bounds, 1, 22 + t0)))
    return cases


def cases_lin_heavy_neg(C, pre):
    """the same totals through negative terms with the smallest covering bias: T = K p - x - sum c z with nbias = K = the sum of the coefficients (every
    negated slot declared < p), z = 0 and x = 0, 1, p - 1, p - (2^364 - 1) on elements 0..3: K p, K p - 1, (K - 1) p + 1, (K - 1) p + 2^364 - 1, K = 1..1000"""
    P = C.P
    bounds = {s: 1 for s in range(2, 11)}
    xs = [0, 1, P - 1, P - BIG]
    cases = []
    Ks = list(range(1, vmgen.HEAVY_MAX + 1))
    per_table = 15 * 15
    for t0 in range(0, len(Ks), per_table):
        layers, dst = [], 11
        chunk = Ks[t0:t0 + per_table]
        for l0 in range(0, len(chunk), 15):
            row = []
            for K in chunk[l0:l0 + 15]:
                terms, rest, z = [(-1, 2)], K - 1, 3
                while rest > 0:
                    c = min(rest, vmgen.COEF_MAX); terms.append((-c, z)); rest -= c; z += 1
                row.append(lin_op(dst, terms, K, True)); dst += 1
            while len(row) < 15: row.append(lin_op(M.DUMP_SLOT, []))
            row.append(lin_op(dst, [(-1, 2)], 1, False)); dst += 1                       # p - x: q = 0 or 1
            layers.append((LIN, row))
        els = []
        for x in xs:
            ws = [0] * dst; ws[2] = x; els.append(ws)
        rng = random.Random(23 + t0)
        ws = [0] * dst
        for s in range(2, 11): ws[s] = rng.randrange(P)
        els.append(ws)
        cases.append(Case(pre + "lin_heavy_neg_%d" % (t0 // per_table), layers, dst, bounds, els))
    return cases


def case_mul(C, pre):
    P = C.P
    edge = {2: 16 * P - 1, 3: 16 * P - 1, 4: 0, 5: 0, 6: P, 7: C.ONE, 8: ones13(C, 16), 9: zeros13(C, 16), 10: 2 * P - 1, 11: 1, 12: P - 1, 13: P + 1}
    bounds = {2: 16, 3: 16, 4: 16, 5: 16, 6: 2, 7: 1, 8: 16, 9: 16, 10: 2, 11: 1, 12: 1, 13: 2}
    plain = [(2, 3), (8, 8), (9, 9), (8, 9), (2, 8), (10, 10), (6, 6), (6, 10), (7, 2), (11, 11), (12, 12), (13, 13), (0, 2), (2, 0), (0, 0), (12, 13)]
    m1 = [mul_op(20 + i, [a, 0, b, 0]) for i, (a, b) in enumerate(plain)]                                    # no lane negates, no second term
    m2 = [mul_op(36 + i, [a, 0, b, 0], 1 if i == 7 else 0) for i, (a, b) in enumerate(plain)]                 # a single lane negates (K17 - p = 16 p)
    m3 = [mul_op(52 + i, [a, 3 if i == 15 else 0, b, 0]) for i, (a, b) in enumerate(plain[:15] + [(2, 10)])]  # only lane 15 has a second term
    full = [
        ([4, 5, 4, 5], 15),        # both terms of both operands negated over zero slots: 34 p x 34 p
        ([2, 3, 2, 3], 0),         # two positive 16 p - 1 terms: 32 p x 32 p
        ([4, 2, 4, 3], 0b0101),    # K17 - 0 + (16 p - 1)
        ([6, 0, 10, 0], 0b0001),   # a negated slot holding exactly p: the term is 16 p
        ([6, 6, 10, 0], 0b0010),   # p + (K17 - p) = 17 p
        ([2, 0, 3, 0], 0),         # second terms absent on both sides in a layer that has them
        ([8, 8, 9, 9], 0),
        ([8, 9, 8, 9], 0b1010),
        ([9, 8, 3, 2], 0b0101),
        ([10, 12, 13, 11], 15),
        ([0, 2, 0, 3], 0b1010),
        ([0, 0, 2, 0], 0b0001),    # K17 - (slot 0)
        ([7, 0, 2, 3], 0),
        ([12, 13, 12, 13], 0b0110),
        ([3, 4, 5, 2], 0b0110),
        ([11, 0, 11, 0], 0b0101),
    ]
    m4 = [mul_op(68 + i, a, neg) for i, (a, neg) in enumerate(full)]
    return Case(pre + "mul", [(MUL, m1), (MUL, m2), (MUL, m3), (MUL, m4)], 84, bounds, elements_from(C, 84, edge, bounds, 3, 24))


def mix_table(C):
    """LIN light -> MUL on its results (negated, summed) -> LIN heavy with coefficients +-127 on the products"""
    P = C.P
    edge = {2: 16 * P - 1, 3: 2 * P - 1, 4: ones13(C, 2), 5: P, 6: 0, 7: P - 1}
    bounds = {2: 16, 3: 2, 4: 2, 5: 2, 6: 1, 7: 1}
    l1 = [lin_op(10, [(1, 2)]), lin_op(11, [(8, 3)]), lin_op(12, [(8, 4)]), lin_op(13, [(7, 5), (-2, 6)], 2), lin_op(14, [(-15, 7)], 15), lin_op(15, [(1, 3), (-1, 5)], 2)]
    prods = [([10, 11, 10, 11], 0), ([10, 11, 11, 10], 0b0110), ([12, 13, 14, 15], 15), ([12, 0, 13, 0], 0b0101), ([14, 10, 15, 2], 0b1001), ([13, 12, 11, 14], 0b0011),
             ([10, 0, 12, 0], 0), ([15, 15, 15, 15], 0b1100), ([11, 13, 10, 12], 0b0101), ([2, 10, 3, 11], 0), ([14, 14, 14, 14], 15), ([12, 11, 13, 10], 0b1010),
             ([3, 4, 5, 7], 0b0101), ([10, 2, 2, 10], 0b1001), ([11, 12, 12, 11], 0), ([13, 0, 13, 0], 0)]
    l2 = [mul_op(20 + i, a, neg) for i, (a, neg) in enumerate(prods)]
    l3 = []
    for i in range(16):
        a, b, c = 20 + i, 20 + (i + 5) % 16, 20 + (i + 11) % 16
        terms = [(127, a), (127, b), (-127, c)] if i % 2 == 0 else [(-127, a), (-127, b), (127, c), (10, 10)]
        neg = sum(-cf * (16 if s == 10 else 2) for cf, s in terms if cf < 0)
        l3.append(lin_op(40 + i, terms, neg, True))
    return [pad(LIN, l1), (MUL, l2), (LIN, l3)], 56, bounds, edge


def case_mix(C, pre, n, seed):
    layers, nslots, bounds, edge = mix_table(C)
    return Case(pre + "mix_n%d" % n, layers, nslots, bounds, elements_from(C, nslots, edge, bounds, n - 1, seed))


def case_rotation(C, pre):
    """every lane's destination is another lane's source: a 16-cycle of slots through a MUL layer (times Montgomery one), a light and a heavy LIN layer"""
    bounds = {2: 1}; edge = {2: C.ONE}
    rng = random.Random(25)
    vals = [0, 1, C.P - 1, C.P, C.P + 1, 2 * C.P - 1, ones13(C, 2), zeros13(C, 2)] + [rng.randrange(2 * C.P) for _ in range(8)]
    for i in range(16): bounds[16 + i], edge[16 + i] = 2, vals[i]
    rot = lambda i: 16 + (i + 1) % 16
    layers = [(MUL, [mul_op(rot(i), [16 + i, 0, 2, 0]) for i in range(16)]),
              (LIN, [lin_op(rot(i), [(1, 16 + i)]) for i in range(16)]),
              (LIN, [lin_op(rot(i), [(3, 16 + i)], 0, True) for i in range(16)])]
    els = elements_from(C, 32, edge, bounds, 2, 26)
    for ws in els: ws[2] = C.ONE
    return Case(pre + "rotation", layers, 32, bounds, els)


def case_copy(C, pre, nslots, n=5):
    """distinct contents in every slot, the upper half mirrored into the lower half: slot numbering and the LDS chunk rotation"""
    pairs = [(2 + j, nslots - 1 - j) for j in range((nslots - 2) // 2)]
    if not pairs and nslots > 2: pairs = [(2, 2)]
    layers = [pad(LIN, [lin_op(d, [(1, s)]) for d, s in pairs[i:i + G]]) for i in range(0, len(pairs), G)] or [pad(LIN, [])]
    bounds = {s: 2 for s in range(2, nslots)}
    rng = random.Random(27 + nslots)
    els = []
    for e in range(n):
        ws = [0] * nslots
        for s in range(2, nslots): ws[s] = rng.randrange(2 * C.P)
        els.append(ws)
    return Case(pre + "copy_%d" % nslots, layers, nslots, bounds, els)


WAVE_SHAPES = [1, 3, 4, 5, 15, 16, 17, 255, 256, 257]
COPY_SLOTS = [2, 3, 16, 104, 106, 255]


@functools.lru_cache(maxsize=None)
def synthetic_cases(tag):
    C = M.CURVES[M.TAGS[tag]]
    pre = tag + "_"
    cases = [case_lin_light(C, pre), case_mul(C, pre), case_rotation(C, pre)]
    cases += cases_lin_heavy_bias(C, pre) + cases_lin_heavy_neg(C, pre)
    cases += [case_copy(C, pre, ns) for ns in COPY_SLOTS]
    cases += [case_mix(C, pre, n, 30 + n) for n in WAVE_SHAPES]
    return cases


# ---- b. the production programs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def generator_tables(name):
    """vmgen.validate()'s tables of one curve, by program name"""
    vmgen.set_curve(name)
    try:
        return {n: c for (n, _), c in vmgen.validate().items()}
    finally:
        vmgen.set_curve("bls12_381")


@functools.lru_cache(maxsize=None)
def header_tables(name):
    return M.parse_header(os.path.join(ROOT, vmgen.CURVES[name]["header"]))


def input_values(C, rng):
    P = C.P
    return [0, 1, P - 1, P, P + 1, 2 * P - 1, ones13(C, 2), C.ONE, rng.randrange(P), P + rng.randrange(P)]


@functools.lru_cache(maxsize=None)
def production_cases(tag):
    """per program: a Case on the committed header's table with all-equal and mixed edge inputs, plus the inputs a seeded search found that push a
    light LIN result or a MUL operand closest to its declared bound; and the attained / declared table {program: {kind: (smallest, largest) over ops}}"""
    name = M.TAGS[tag]
    C = M.CURVES[name]
    hdr, gen = header_tables(name), generator_tables(name)
    cases, table = [], {}
    for prog in PROGS:
        h, c = hdr[prog], gen[prog]
        decl = M.check_contract(c)
        assert M.pack(c["layers"]) == (h["kinds"], h["ops"]) and c["nslots"] == h["nslots"]
        rng = random.Random(40 + PROGS.index(prog))
        ins = h["in"]
        def ws_of(vals):
            ws = [0] * h["nslots"]
            for s, v in zip(ins, vals): ws[s] = v
            return ws
        els = [ws_of([v] * len(ins)) for v in input_values(C, rng)]
        for _ in range(24):
            vs = input_values(C, rng); els.append(ws_of([rng.choice(vs) for _ in ins]))
        if prog in ("line_add", "line_double"):                  # real points, as k_vm_miller_lines feeds them (every slot the R'-form): T = Q and T = -Q make lambda = 0
            m = _models()[tag]
            Qa, Pa = m.g2_mul(1234567), m.g1_mul(7654321)
            for sign in (1, -1):
                Ta = Qa if sign > 0 else m.ec_neg(m._Fp2, Qa)
                v = dict(X0=Ta[0][0], X1=Ta[0][1], Y0=Ta[1][0], Y1=Ta[1][1], Z0=1, Z1=0, xP=Pa[0], yP=Pa[1], qx0=Qa[0][0], qx1=Qa[0][1], qy0=Qa[1][0], qy1=Qa[1][1])
                els.append(ws_of([v[n] * C.ONE % C.P for n in h["ins"]]))
        # the search: keep a candidate when it raises the attained / declared ratio of any op
        best = M.Stats()
        for ws in els: M.run(C, h["kinds"], h["ops"], ws, decl, best, False)
        high = [2 * C.P - 1, ones13(C, 2), 2 * C.P - 2, C.P - 1, 0]
        kept = 0
        for _ in range(60):
            vals = [rng.choice(high) if rng.random() < 0.7 else rng.randrange(2 * C.P) for _ in ins]
            st = M.Stats()
            M.run(C, h["kinds"], h["ops"], ws_of(vals), decl, st, False)
            if any(r > best.ratio.get(k, 0.0) + 1e-9 for k, r in st.ratio.items()) and kept < 24:
                els.append(ws_of(vals)); kept += 1
                for k, r in st.ratio.items(): best.ratio[k] = max(best.ratio.get(k, 0.0), r)
        t = [r for k, r in best.ratio.items() if k[2] == "T"]; o = [r for k, r in best.ratio.items() if k[2] != "T"]
        table[prog] = dict(light_lin=(min(t), max(t)) if t else None, mul_operand=(min(o), max(o)), elements=len(els))
        cases.append(Case(tag + "_" + prog, None, h["nslots"], {s: vmgen.BOUND_IN for s in ins}, els, decl=decl, kinds=h["kinds"], ops=h["ops"]))
    return cases, table


def formula_outputs(name, prog, h, ws):
    """the plain formulas vmgen holds (ref_line_double, ref_line_add, f12m) on the field elements the slots stand for (slot value x R'^-1), as the
    slot residues mod p the program must leave: {slot: residue}; None for the programs whose formula is a group law (checked as points elsewhere)"""
    C = M.CURVES[name]
    P = C.P
    fe = lambda nm: ws[h["ins"][nm]] * C.RINV % P
    f2 = lambda nm: (fe(nm + "0"), fe(nm + "1"))
    vmgen.set_curve(name)
    try:
        if prog == "line_double": ref = vmgen.ref_line_double(f2("X"), f2("Y"), f2("Z"), fe("xP"), fe("yP"))
        elif prog == "line_add": ref = vmgen.ref_line_add(f2("X"), f2("Y"), f2("Z"), f2("qx"), f2("qy"), fe("xP"), fe("yP"))
        elif prog == "fp12_mul":
            r = vmgen.f12m([f2("f" + n) for n in vmgen.F12_NAMES], [f2("g" + n) for n in vmgen.F12_NAMES])
            ref = {"f" + n: v for n, v in zip(vmgen.F12_NAMES, r)}
        else: return None
    finally:
        vmgen.set_curve("bls12_381")
    out = {}
    for k, v in ref.items():
        out[h["outs"][k + "0"]] = v[0] * (1 << M.RBITS) % P; out[h["outs"][k + "1"]] = v[1] * (1 << M.RBITS) % P
    return out


# ---- VmCurve<F> sequences ----------------------------------------------------------------------------------------------------------------------------
R384 = 1 << 384
SCALAR = 0xC3A5F00DDEADBEEF


def _models():
    import bls377_model as m377
    import bls381_model as m381
    return {"381": m381, "377": m377}


def step_strings():
    chain = []
    for bit in bin(SCALAR)[3:]:
        chain.append(0)
        if bit == "1": chain.append(1)
    return {"add": [1], "dbl": [0], "dbl_add": [0, 1], "add_add_dbl": [1, 1, 0], "dbl64": [0] * 64, "scalar64": chain}


def curve_points(tag, g2):
    """(name, T, Q): homogeneous (X, Y, Z) field elements (Fp: ints, Fp2: pairs), the identity as (0 : 1 : 0); and the affine points they stand for"""
    m = _models()[tag]
    Fb = m._Fp2 if g2 else m._Fp
    mul = m.g2_mul if g2 else m.g1_mul
    P1, Q1 = mul(1234567), mul(7654321)
    hom = lambda pt, z: (Fb.mul(pt[0], z), Fb.mul(pt[1], z), z)
    inf = (Fb.zero, Fb.one, Fb.zero)
    rng = random.Random(50)
    z1 = (rng.randrange(m.P), rng.randrange(m.P)) if g2 else rng.randrange(m.P)
    z2 = (0, m.P - 1) if g2 else m.P - 1
    out = [("generic", hom(P1, Fb.one), hom(Q1, Fb.one), P1, Q1), ("inf+Q", inf, hom(Q1, Fb.one), None, Q1), ("T+inf", hom(P1, Fb.one), inf, P1, None),
           ("inf+inf", inf, inf, None, None), ("T=Q", hom(P1, Fb.one), hom(P1, Fb.one), P1, P1), ("T=-Q", hom(P1, Fb.one), hom(m.ec_neg(Fb, P1), Fb.one), P1, m.ec_neg(Fb, P1)),
           ("Z!=1", hom(P1, z1), hom(Q1, z2), P1, Q1), ("Z!=1 T=Q", hom(P1, z1), hom(P1, z2), P1, P1)]
    if not g2:
        o3 = (0, 2) if tag == "381" else (0, 1)               # a point of order 3
        out += [("order 3", hom(o3, 1), hom(o3, 1), o3, o3), ("order 3, T=-Q", hom(o3, 1), hom(m.ec_neg(Fb, o3), 1), o3, m.ec_neg(Fb, o3))]
    return out


def engine_words(C, coords, g2):
    """field elements -> engine format: a 2^384 mod p, 12 words per Fp"""
    out = []
    for c in coords:
        for x in (c if g2 else (c,)):
            v = x * R384 % C.P
            out += [(v >> (32 * j)) & 0xFFFFFFFF for j in range(12)]
    return out


def curve_chain(tag, g2, T, Q, steps):
    """the model chained as the harness chains VmCurve<F>: put (re-slice) -> dbl_ / add_ with the addend rewritten before every addition -> get (mod p).
    Returns T as field elements (value 2^-384)."""
    name = M.TAGS[tag]
    C = M.CURVES[name]
    hdr = header_tables(name)
    hd, ha = hdr["g2_hdbl" if g2 else "g1_hdbl"], hdr["g2_cadd" if g2 else "g1_cadd"]
    nf = 2 if g2 else 1
    ws = [0] * max(hd["nslots"], ha["nslots"])
    def put(base, coords):
        for k, c in enumerate(coords):
            for j, x in enumerate(c if g2 else (c,)): ws[base[k] + j] = x * R384 % C.P
    S = [ha["ins"]["X0"], ha["ins"]["Y0"], ha["ins"]["Z0"]]; Qs = [ha["ins"]["qx0"], ha["ins"]["qy0"], ha["ins"]["qz0"]]
    assert [hd["ins"]["X0"], hd["ins"]["Y0"], hd["ins"]["Z0"]] == S and [ha["outs"]["X0"], ha["outs"]["Y0"], ha["outs"]["Z0"]] == S
    put(S, T)
    for st in steps:
        if st == 0: ws = _run_on(C, hd, ws)
        else:
            put(Qs, Q); ws = _run_on(C, ha, ws)
    inv = pow(R384, -1, C.P)
    get = lambda s: tuple((ws[s + j] % C.P) * inv % C.P for j in range(nf)) if g2 else (ws[s] % C.P) * inv % C.P
    return tuple(get(s) for s in S)


def _run_on(C, h, ws):
    """a program on a workspace that may be larger than its own"""
    n = h["nslots"]
    head = M.run(C, h["kinds"], h["ops"], ws[:n], columns=False)
    return head + ws[n:]


def affine_of(tag, g2, XYZ):
    m = _models()[tag]
    Fb = m._Fp2 if g2 else m._Fp
    X, Y, Z = XYZ
    if Z == Fb.zero:
        assert X == Fb.zero and Y != Fb.zero
        return None
    zi = Fb.inv(Z)
    return Fb.mul(X, zi), Fb.mul(Y, zi)


def expected_point(tag, g2, Ta, Qa, steps):
    m = _models()[tag]
    Fb = m._Fp2 if g2 else m._Fp
    for st in steps: Ta = m.ec_add(Fb, Ta, Ta) if st == 0 else m.ec_add(Fb, Ta, Qa)
    return Ta


@functools.lru_cache(maxsize=None)
def curve_cases(tag, g2):
    """[(steps name, steps, [(case name, T, Q, model result (field elements), expected affine point)])]"""
    out = []
    for sname, steps in step_strings().items():
        rows = []
        for cname, T, Q, Ta, Qa in curve_points(tag, g2):
            got = curve_chain(tag, g2, T, Q, steps)
            rows.append((cname, T, Q, got, expected_point(tag, g2, Ta, Qa, steps)))
        out.append((sname, steps, rows))
    return out


# ---- c. k_vm_fp12_tree ----------------------------------------------------------------------------------------------------------------------------------
TREE_TINS = [1, 2, 3, 4, 5, 255, 256, 257]
TREE_ROWS = 2


def tree_elements(C):
    """Fp12 values as 12 engine words (integers < p): zero, the integer 1 in the first coefficient, Montgomery one in each single coefficient, p - 1
    everywhere, four random ones"""
    one = R384 % C.P
    rng = random.Random(60)
    els = [tuple([0] * 12), tuple([1] + [0] * 11)] + [tuple(one if i == k else 0 for i in range(12)) for k in range(12)] + [tuple([C.P - 1] * 12)]
    els += [tuple(rng.randrange(C.P) for _ in range(12)) for _ in range(4)]
    return els


def tree_input(C, Tin, row):
    els = tree_elements(C)
    rng = random.Random(61 + 7 * Tin + row)
    return [els[(j + row) % len(els)] if j < 2 * len(els) else rng.choice(els) for j in range(Tin)]


_tree_cache = {}


def tree_product(tag, f, g):
    """the fp12_mul table of the committed header on the re-sliced words of f and g; the result words (canonical), bit for bit what k_vm_fp12_tree stores"""
    key = (tag, f, g)
    if key not in _tree_cache:
        name = M.TAGS[tag]
        C = M.CURVES[name]
        h = header_tables(name)["fp12_mul"]
        ws = [0] * h["nslots"]
        for k in range(12): ws[h["in"][k]], ws[h["in"][12 + k]] = f[k], g[k]
        out = M.run(C, h["kinds"], h["ops"], ws, columns=False)
        _tree_cache[key] = tuple(out[h["out"][k]] % C.P for k in range(12))
    return _tree_cache[key]


def tree_expected(tag, vals, Tout):
    Tin = len(vals)
    return [tree_product(tag, vals[j], vals[j + Tout]) if j + Tout < Tin else vals[j] for j in range(Tout)]


def tree_formula(tag, f, g):
    """Inputs cross the kernel boundary re-sliced: the 12 words of an engine value a 2^384 are read as the R' = 2^392 form of a 2^-8 (the header note of
    vm.hpp).  The product program is bilinear, so it leaves the R'-form of (a 2^-8)(b 2^-8) = (a b 2^-8) 2^-8, whose words read back as an engine value
    are a b 2^-8: the Fp12 product times 2^-8, once per product level."""
    name = M.TAGS[tag]
    P = M.CURVES[name].P
    inv = pow(R384, -1, P)
    fe = lambda v: [(v[2 * i] * inv % P, v[2 * i + 1] * inv % P) for i in range(6)]
    vmgen.set_curve(name)
    try:
        r = vmgen.f12m(fe(f), fe(g))
    finally:
        vmgen.set_curve("bls12_381")
    s = pow(2, -8, P) * R384 % P
    return tuple(c * s % P for pair in r for c in pair)
