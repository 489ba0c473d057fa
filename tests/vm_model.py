"""A limb-exact model of the lane-parallel field VM interpreter (ripp_amd/csrc/vm.hpp: vm_run, vm_operand, vm_carry) on Python integers
(TEST INFRASTRUCTURE ONLY).

A workspace slot holds 14 limbs of 28 bits whose low 13 limbs are normalised and whose top limb keeps the rest, so a slot IS its integer value:
the model keeps integers and `limbs()` gives the words the device holds.  Where the device works on limbs that are NOT the digits of the value
(the limb-wise K17 - x of a negated MUL term, the 64-bit columns of both layer kinds, the float quotient estimate of a heavy LIN), the model
works on limbs too and asserts what the device only assumes.

    pack(layers)            (kind, row) layers in the shape tools/vmgen.py compile_prog returns -> kind bytes + 36-byte VmOp records, as vmgen.emit writes them
    parse_header(path)      the committed vm_programs.inc -> the same packed form, so the model runs on exactly what the device compiled
    check_contract(c, ..)   what vm_run assumes about a table (the generator's constants), with the declared bound of every initial slot as an argument
    run(curve, kinds, ops, ws, ..)   the interpreter
"""
import os
import re
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import vmgen  # noqa: E402

NL, W, G = 14, 28, 16
MASK = (1 << W) - 1
RBITS = NL * W                     # 392: the Montgomery radix R' = 2^392
MUL, LIN = vmgen.MUL, vmgen.LIN
ZERO_SLOT, DUMP_SLOT = vmgen.ZERO_SLOT, vmgen.DUMP_SLOT


def limbs(v):
    """the device's limbs of a slot value: base-2^28 digits, the top limb keeps the rest"""
    assert v >= 0
    return [(v >> (W * i)) & MASK for i in range(NL - 1)] + [v >> (W * (NL - 1))]


def value(ls):
    return sum(int(x) << (W * i) for i, x in enumerate(ls))


class Curve:
    """the constants of fq28.hpp and vm.hpp for one modulus"""

    def __init__(self, name):
        self.name, self.P = name, vmgen.CURVES[name]["P"]
        P = self.P
        self.P28 = [(P >> (W * i)) & MASK for i in range(NL)]
        assert value(self.P28) == P
        self.P_TOP = self.P28[NL - 1]
        self.INV28 = (-pow(P, -1, 1 << W)) % (1 << W)
        self.PINV_R = pow(P, -1, 1 << RBITS)
        self.RINV = pow(1 << RBITS, -1, P)
        self.ONE = (1 << RBITS) % P
        # neg_bias(): 17 p (normalised, times_p) with n_k + 2^28 [k < 13] - [k > 0]
        n = limbs(vmgen.NEG_K * P)
        self.K17 = [n[k] + ((1 << W) if k < NL - 1 else 0) - (1 if k > 0 else 0) for k in range(NL)]
        assert value(self.K17) == vmgen.NEG_K * P
        assert self.K17[NL - 1] >= vmgen.LIGHT_MAX * (self.P_TOP + 1)          # the static_assert of vm.hpp
        # INV_PTOP = (1.0f - 1.0f / 1048576.0f) / (float)(P_TOP + 1), every step in float32 as the compiler folds it
        self.INV_PTOP = (np.float32(1.0) - np.float32(1.0) / np.float32(1048576.0)) / np.float32(self.P_TOP + 1)
        assert self.INV_PTOP.dtype == np.float32

    def quotient_estimate(self, top):
        """int((float)top * INV_PTOP): u32 -> float32 (round to nearest even), one float32 product, truncation"""
        assert 0 <= top < 1 << 32
        return int(np.float32(top) * self.INV_PTOP)


CURVES = {"bls12_381": Curve("bls12_381"), "bls12_377": Curve("bls12_377")}
TAGS = {"381": "bls12_381", "377": "bls12_377"}


# ---- tables -------------------------------------------------------------------------------------------------------------------------------------
def pack(layers):
    """(kind, row) layers -> (kind bytes, ops) with ops a list of (dst, flags, nbias, s[16], c[16]), 16 per layer: what vmgen.emit writes"""
    kinds, ops = [], []
    for kind, row in layers:
        assert len(row) == G
        if kind == MUL:
            kinds.append(0)
            for op in row:
                ops.append((op["dst"], op["neg"], 0, tuple(op["a"]) + (0,) * 12, (0,) * 16))
        else:
            tmax = max([len(op["terms"]) for op in row] + [1]); heavy = any(op["heavy"] for op in row)
            kinds.append(0x80 | (0x40 if heavy else 0) | tmax)
            for op in row:
                sl = [t[1] for t in op["terms"]]; cf = [t[0] for t in op["terms"]]
                ops.append((op["dst"], 0, op["nbias"], tuple(sl) + (0,) * (16 - len(sl)), tuple(cf) + (0,) * (16 - len(cf))))
    return kinds, ops


def op_bytes(ops):
    """the VmOp records as the device reads them: {u8 dst, u8 flags, u16 nbias, u8 s[16], i8 c[16]}, 36 bytes each, little endian"""
    return b"".join(struct.pack("<BBH16B16b", dst, fl, nb, *(s + c)) for dst, fl, nb, s, c in ops)


def ops_from_bytes(raw):
    assert len(raw) % 36 == 0
    out = []
    for i in range(0, len(raw), 36):
        f = struct.unpack("<BBH16B16b", raw[i:i + 36])
        out.append((f[0], f[1], f[2], tuple(f[3:19]), tuple(f[19:35])))
    return out


_OP = re.compile(r"\{(\d+),(\d+),(\d+),\{([^}]*)\},\{([^}]*)\}\}")


def parse_header(path):
    """the committed tables: {program: dict(nlayers, nslots, kinds, ops, in, out, ins={name: slot}, outs={name: slot})}"""
    text = open(path).read()
    progs = {}
    for m in re.finditer(r"constexpr int (\w+)_g16_nlayers = (\d+), \w+_g16_nslots = (\d+);", text):
        progs[m.group(1)] = dict(nlayers=int(m.group(2)), nslots=int(m.group(3)), ins={}, outs={})
    ints = lambda s: [int(x) for x in s.split(",") if x.strip()]
    for name, d in progs.items():
        tag = name + "_g16"
        d["kinds"] = ints(re.search(r"%s_kind\[\d+\] = \{([^}]*)\}" % tag, text).group(1))
        body = re.search(r"%s_ops\[(\d+)\] = \{(.*)\};" % tag, text)
        d["ops"] = []
        for o in _OP.finditer(body.group(2)):
            s, c = ints(o.group(4)), ints(o.group(5))
            d["ops"].append((int(o.group(1)), int(o.group(2)), int(o.group(3)), tuple(s) + (0,) * (16 - len(s)), tuple(c) + (0,) * (16 - len(c))))
        assert len(d["ops"]) == int(body.group(1)) == G * d["nlayers"] and len(d["kinds"]) == d["nlayers"], name
        d["in"] = ints(re.search(r"%s_in\[\d+\] = \{([^}]*)\}" % tag, text).group(1))
        d["out"] = ints(re.search(r"%s_out\[\d+\] = \{([^}]*)\}" % tag, text).group(1))
        for m in re.finditer(r"constexpr int %s_(in|out)_(\w+) = (\d+);" % tag, text):
            d["ins" if m.group(1) == "in" else "outs"][m.group(2)] = int(m.group(3))
        assert list(d["ins"].values()) == d["in"] and list(d["outs"].values()) == d["out"], name
    return progs


# ---- the contract ---------------------------------------------------------------------------------------------------------------------------------
def check_contract(c, in_bounds=None):
    """What vm.hpp::vm_run assumes about a table `c` (dict with layers, nslots, ins, outs as vmgen.compile_prog returns): slot indices are bytes,
    a LIN op has at most 16 terms with |coefficient| <= 127 and a bias that fits 16 bits and covers its negative terms, a light LIN result stays
    below 16 p, the operand bounds of a MUL multiply to <= VMAX.  `in_bounds` = {slot: declared bound in units of p (<= LIGHT_MAX)} of the initial
    workspace; the default is BOUND_IN for every input of `c`.  Returns per layer and lane what the table DECLARES: ("mul", boundA, boundB) or
    ("lin", pos + nbias, reduced)."""
    V = vmgen
    Gc = len(c["layers"][0][1]) if c["layers"] else G
    assert c["nslots"] <= 255
    bound = {s: V.BOUND_IN for s in c["ins"].values()} if in_bounds is None else dict(in_bounds)
    assert all(0 <= b <= V.LIGHT_MAX and s not in (V.ZERO_SLOT, V.DUMP_SLOT) and 0 <= s < c["nslots"] for s, b in bound.items())
    bound[V.ZERO_SLOT] = 0; bound[V.DUMP_SLOT] = 0
    decl = []
    for kind, row in c["layers"]:
        assert kind in (V.MUL, V.LIN) and len(row) == Gc
        new = {}
        heavy_layer = kind == V.LIN and any(op["heavy"] for op in row)
        dsts = [op["dst"] for op in row if op["dst"] != V.DUMP_SLOT]
        assert len(set(dsts)) == len(dsts) and V.ZERO_SLOT not in dsts          # one writer per slot and layer; slot 0 stays zero
        drow = []
        for op in row:
            assert 0 <= op["dst"] < c["nslots"]
            if kind == V.MUL:
                assert all(0 <= a < c["nslots"] and a != V.DUMP_SLOT for a in op["a"]) and 0 <= op["neg"] < 16
                # "second term absent" is slot 0: the device skips it when no lane of the wave has one, so it must not carry a negation
                assert all(not ((op["neg"] >> (2 * h + 1)) & 1) or op["a"][2 * h + 1] != V.ZERO_SLOT for h in range(2))
                ob = [sum((V.NEG_K if (op["neg"] >> (2 * h + t)) & 1 else bound[op["a"][2 * h + t]]) for t in range(2) if op["a"][2 * h + t] != V.ZERO_SLOT or t == 0) for h in range(2)]
                assert all(bound[a] <= V.LIGHT_MAX for a in op["a"]) and ob[0] * ob[1] <= V.VMAX
                new[op["dst"]] = 2
                drow.append(("mul", ob[0], ob[1]))
            else:
                assert len(op["terms"]) <= V.TMAX and all(abs(cf) <= V.COEF_MAX and 0 <= sl < c["nslots"] and sl != V.DUMP_SLOT for cf, sl in op["terms"]) and 0 <= op["nbias"] < 65536
                neg = sum(-cf * bound[sl] for cf, sl in op["terms"] if cf < 0); pos = sum(cf * bound[sl] for cf, sl in op["terms"] if cf > 0)
                assert op["nbias"] >= neg and pos + op["nbias"] <= V.HEAVY_MAX
                assert heavy_layer or pos + op["nbias"] <= V.LIGHT_MAX
                # with no positive term the total can BE nbias p (negated slots all zero): a light result must still be a value < 16 p
                assert heavy_layer or pos > 0 or op["nbias"] < V.LIGHT_MAX
                new[op["dst"]] = 2 if heavy_layer else pos + op["nbias"]
                drow.append(("lin", pos + op["nbias"], heavy_layer))
        bound.update(new)
        decl.append(drow)
    for s in c["outs"].values(): assert bound[s] <= V.BOUND_IN          # kernels read outputs back as canonical values
    return decl


# ---- the interpreter ------------------------------------------------------------------------------------------------------------------------------
class Stats:
    """what a run met: the two outcomes of the heavy quotient estimate, the largest 64-bit column of either kind, and per op (layer, lane) the
    largest attained / declared ratio of a light LIN result and of a MUL operand"""

    def __init__(self):
        self.q_exact = self.q_short = 0
        self.max_mul_col = self.max_lin_col = 0
        self.ratio = {}

    def note(self, key, attained, declared):
        if declared > 0: self.ratio[key] = max(self.ratio.get(key, 0.0), attained / declared)


def _check_slot(C, v, what):
    l = limbs(v)
    assert v < vmgen.LIGHT_MAX * C.P, ("slot value >= 16 p", what)
    assert all(a <= k for a, k in zip(l, C.K17)), ("a limb of a slot exceeds K17's", what)
    return l


def _operand(C, ws, s0, s1, n0, n1, second):
    """vm_operand: limbs of (+-ws[s0]) (+-ws[s1]); a negated term is K17 - x limb by limb"""
    x = _check_slot(C, ws[s0], ("operand", s0))
    r = [k - a for k, a in zip(C.K17, x)] if n0 else list(x)
    if second:
        y = _check_slot(C, ws[s1], ("operand", s1))
        r = [a + ((k - b) if n1 else b) for a, b, k in zip(r, y, C.K17)]
    assert all(0 <= a < 1 << 30 for a in r), "operand limb >= 2^30"
    return r


def montgomery(C, a, b, stats=None, columns=True):
    """fq_mul on limbs: (A B + m p) >> 392, m = -A B p^-1 mod 2^392; with `columns` the column-wise walk of fq_montgomery, every 64-bit sum checked"""
    A, B = value(a), value(b)
    m = (-A * B * C.PINV_R) % (1 << RBITS)
    r = (A * B + m * C.P) >> RBITS
    assert (A * B + m * C.P) % (1 << RBITS) == 0 and r < 2 * C.P, "product >= 2 p"
    if columns:
        mm, out, carry, big = [0] * NL, [0] * NL, 0, 0
        for k in range(NL):
            s = carry + sum(a[i] * b[k - i] for i in range(k + 1)) + sum(mm[i] * C.P28[k - i] for i in range(k))
            mm[k] = (((s & 0xFFFFFFFF) * C.INV28) & 0xFFFFFFFF) & MASK
            s += mm[k] * C.P28[0]
            big = max(big, s); carry = s >> W
        for k in range(NL, 2 * NL - 1):
            s = carry + sum(a[i] * b[k - i] for i in range(k - NL + 1, NL)) + sum(mm[i] * C.P28[k - i] for i in range(k - NL + 1, NL))
            big = max(big, s); out[k - NL] = s & MASK; carry = s >> W
        out[NL - 1] = carry
        assert big < 1 << 64, "a column of the product overflows 64 bits"
        assert out == limbs(r) and value(mm) == m
        if stats is not None: stats.max_mul_col = max(stats.max_mul_col, big)
    return r


def _carry(col):
    """vm_carry: signed pass, limbs < 2^28, the top limb keeps the rest (and must fit 32 bits)"""
    r, carry = [], 0
    for i in range(NL - 1):
        t = col[i] + carry
        assert -(1 << 63) <= t < 1 << 63
        r.append(t & MASK); carry = t >> W
    top = col[NL - 1] + carry
    assert 0 <= top < 1 << 32, "the top limb of a LIN result leaves 32 bits"
    return r + [top]


def lin(C, xs, cs, nbias, heavy, stats=None):
    """one LIN op on slot values xs with coefficients cs: T = sum c x + nbias p through signed 64-bit columns; returns the stored value"""
    P = C.P
    T = sum(c * x for c, x in zip(cs, xs)) + nbias * P
    assert T >= 0, "nbias does not cover the negative terms"
    xl = [limbs(x) for x in xs]
    assert all(l < 1 << 31 for x in xl for l in x)                 # (int32_t)x.l[i]
    col = [0] * NL
    for c, x in zip(cs, xl):                                       # term by term, as the device accumulates
        for i in range(NL):
            col[i] += c * x[i]
            assert -(1 << 63) <= col[i] < 1 << 63
    for i in range(NL):
        col[i] += nbias * C.P28[i]
        assert -(1 << 63) <= col[i] < 1 << 63
    if stats is not None: stats.max_lin_col = max(stats.max_lin_col, max(abs(x) for x in col))
    r = _carry(col)
    assert value(r) == T
    if not heavy:
        assert T < vmgen.LIGHT_MAX * P, "light LIN result >= 16 p"
        return T
    q = C.quotient_estimate(r[NL - 1])
    true_q = T // P
    assert q in (true_q, true_q - 1), ("quotient estimate", hex(T), q, true_q)
    if stats is not None:
        if q == true_q: stats.q_exact += 1
        else: stats.q_short += 1
    r2 = _carry([r[i] - q * C.P28[i] for i in range(NL)])
    assert value(r2) == T - q * P and value(r2) < 2 * P
    return value(r2)


def run(C, kinds, ops, ws, decl=None, stats=None, columns=True):
    """vm_run on one element: `ws` a list of slot values (slot 0 must be 0).  All reads of a layer happen before its writes; lanes store in
    lane order (only DUMP_SLOT has several writers, and it is not compared).  Returns the final workspace."""
    ws = list(ws)
    assert ws[ZERO_SLOT] == 0 and len(ops) == G * len(kinds)
    for s, v in enumerate(ws):
        if s != DUMP_SLOT: _check_slot(C, v, ("initial", s))
    for l, k in enumerate(kinds):
        row = ops[l * G:(l + 1) * G]
        res = []
        if k == 0:
            second = [any(op[3][2 * h + 1] != 0 for op in row) for h in range(2)]          # __any(s1 != 0u)
            for lane, (dst, fl, nb, s, c) in enumerate(row):
                assert all(not (fl >> (2 * h + 1)) & 1 or s[2 * h + 1] != 0 for h in range(2))
                A = _operand(C, ws, s[0], s[1], fl & 1, fl & 2, second[0])
                B = _operand(C, ws, s[2], s[3], fl & 4, fl & 8, second[1])
                assert value(A) * value(B) <= vmgen.VMAX * C.P * C.P
                if decl is not None and stats is not None and dst != DUMP_SLOT:
                    stats.note((l, lane, "A"), value(A) / C.P, decl[l][lane][1]); stats.note((l, lane, "B"), value(B) / C.P, decl[l][lane][2])
                res.append((dst, montgomery(C, A, B, stats, columns)))
        else:
            assert k & 0x80
            nt, heavy = k & 31, bool(k & 64)
            assert nt <= 16
            for lane, (dst, fl, nb, s, c) in enumerate(row):
                assert all(cf == 0 for cf in c[nt:]), "a term beyond the layer's count"
                v = lin(C, [ws[x] for x in s[:nt]], c[:nt], nb, heavy, stats)
                if decl is not None and stats is not None and not heavy and dst != DUMP_SLOT:
                    stats.note((l, lane, "T"), v / C.P, decl[l][lane][1])
                res.append((dst, v))
        for dst, v in res:
            assert dst != ZERO_SLOT
            if dst != DUMP_SLOT: _check_slot(C, v, ("result", l, dst))
            ws[dst] = v
    return ws


def first_failing_k(C, kmax):
    """the smallest k for which a heavy step on k p - 1, k p or k p + 1 leaves [0, 2p) (None below kmax); totals whose top limb leaves 32 bits end the search"""
    P = C.P
    for k in range(kmax):
        for d in (-1, 0, 1):
            T = k * P + d
            if T < 0: continue
            top = T >> (W * (NL - 1))
            if top >= 1 << 32: return k, "top limb leaves 32 bits"
            q = C.quotient_estimate(top)
            if not 0 <= T - q * P < 2 * P: return k, "result outside [0, 2p)"
    return None, None
