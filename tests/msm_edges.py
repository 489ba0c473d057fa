"""The plain reference of the Pippenger stages behind the digit pass (ripp_amd/csrc/msm.hpp, fq_msm.hpp, msm_batch.hpp) and the inputs of
tests/test_gpu_msm_edges.py (checked on the CPU by tests/test_msm_edges_model_cpu.py).

Reference: Python integers and the affine chord-and-tangent arithmetic of tests/model/bls381_model.py / bls377_model.py.  A device point is compared only after
it is PROJECTED here -- Jacobian (X, Y, Z) -> (X / Z^2, Y / Z^3), homogeneous (X : Y : Z) -> (X / Z, Y / Z), Z = 0 -> the identity (None) -- and equality is
exact.  The image of term j * nreal + i is defined by scalar multiplication, not by the endomorphism the kernels apply: G1: [lambda^j] P_i (j < 2),
G2: [u^j mod r] Q_i with u = |x| (j < 4).

The slot layout is restated without lanes: a window's terms sorted by digit form one run per bucket (bucket 0 has none), a bucket of cnt terms has
ceil(cnt / ch) slots of ch terms (the last one shorter), slots are numbered through the window in bucket order; grouping pass j (stride 8^j) lets every
8 * 8^j-th slot of a bucket with more than gmin * 8^j slots add the up to 8 partial sums stride apart, and the merge of a bucket walks its slots in steps of
8^(passes that applied to it)."""
import functools
import random

import numpy as np

import bls377_model as m377
import bls381_model as m381
import field_edges
import fr_edges

TAGS = ["381", "377"]
MODELS = {"381": m381, "377": m377}
R384 = 1 << 384
SLOT_GROUP, GROUP_PASSES, SEG_FAN, SORT_BLOCK = 8, 3, 4, 1024


class Group:
    """one of the four groups: tag x (G1 | G2)"""
    def __init__(self, tag, g2):
        m = MODELS[tag]
        self.tag, self.g2, self.m, self.P, self.r = tag, g2, m, m.P, m.R
        self.F = m._Fp2 if g2 else m._Fp
        self.gen = m.G2 if g2 else m.G1
        self.nf = 2 if g2 else 1                                        # Fp coordinates per field element
        self.x_abs = fr_edges.CURVES[tag].x
        self.lam = fr_edges.CURVES[tag].lam
        self.split = 4 if g2 else 2                                     # the split the engine uses for this group
        self.rinv = pow(R384, -1, self.P)
        b = 4 if tag == "381" else 1
        self.b = (m.f2muls(m.XI, 4) if tag == "381" else m.B_TWIST) if g2 else b

    def add(self, a, b): return self.m.ec_add(self.F, a, b)
    def neg(self, a): return self.m.ec_neg(self.F, a)
    def mul(self, k, a): return self.m.ec_mul(self.F, k, a)               # k >= 0, NOT reduced: the x = 0 point is outside the subgroup
    def sum(self, pts):
        acc = None
        for q in pts: acc = self.add(acc, q)
        return acc
    def on_curve(self, a):
        if a is None: return True
        F = self.F
        return F.sub(F.mul(a[1], a[1]), F.add(F.mul(F.mul(a[0], a[0]), a[0]), self.b if self.g2 else self.b % self.P)) == F.zero
    def image_scalar(self, j): return pow(self.x_abs, j, self.r) if self.g2 else pow(self.lam, j, self.r)
    def fe(self, v): return v if self.g2 else (v,)                        # field element -> tuple of Fp coordinates
    def ef(self, t): return tuple(t) if self.g2 else t[0]
    def rand_fe(self, rnd):
        while True:
            v = tuple(rnd.randrange(self.P) for _ in range(self.nf))
            if any(v): return self.ef(v)


@functools.lru_cache(maxsize=None)
def group(tag, g2): return Group(tag, bool(g2))


@functools.lru_cache(maxsize=None)
def pool(tag, g2, count=24):
    """`count` distinct non-trivial subgroup points k G, k seeded; pool[i] for i >= 1 is NOT a small multiple of pool[0]"""
    G = group(tag, g2)
    rnd = random.Random("msm_edges pool %s %d" % (tag, g2))
    pts = [G.mul(rnd.randrange(1, G.r), G.gen) for _ in range(count)]
    assert len(set(pts)) == count and all(G.on_curve(q) for q in pts)
    return tuple(pts)


_image_cache = {}


def image(tag, g2, pt, j):
    """the image of a SUBGROUP point that term j * nreal + i stands for: [lambda^j] P resp. [u^j mod r] Q, by double-and-add"""
    if pt is None or j == 0: return pt
    key = (tag, g2, pt, j)
    if key not in _image_cache:
        G = group(tag, g2)
        _image_cache[key] = G.mul(G.image_scalar(j), pt)
    return _image_cache[key]


def x0_point(tag, g2):
    """the curve point with x = 0 (y^2 = b; it is outside the prime-order subgroup), or None where b is no square"""
    import miller_edges as ME
    G = group(tag, g2)
    if g2:
        y = ME.f2_sqrt(ME.CURVES[tag], G.b)
        return None if y is None else ((0, 0), y)
    y = ME.fp_sqrt(G.P, G.b)
    return None if y is None else (0, y)


# ---- words ------------------------------------------------------------------------------------------------------------------------------------------
def _w12(v): return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(12)]


def pack_affine(G, pts):
    """model points (None = the identity = all zero) -> the engine's Montgomery-384 words, 24 (G1) / 48 (G2) per point"""
    out = np.zeros((len(pts), 24 * G.nf), dtype=np.uint32)
    for i, pt in enumerate(pts):
        if pt is None: continue
        out[i] = [w for c in pt for v in G.fe(c) for w in _w12(v * R384 % G.P)]
    return out


def pack_proj(G, triples):
    """(X, Y, Z) field elements -> 36 / 72 Montgomery words per point"""
    out = np.zeros((len(triples), 36 * G.nf), dtype=np.uint32)
    for i, t in enumerate(triples):
        out[i] = [w for c in t for v in G.fe(c) for w in _w12(v * R384 % G.P)]
    return out


def unpack_proj(G, arr):
    """rows of 36 / 72 words -> (X, Y, Z) plain field elements; every coordinate must be a canonical Montgomery value (< p)"""
    out = []
    for row in np.ascontiguousarray(arr).reshape(-1, 36 * G.nf):
        raw = row.tobytes()
        vs = [int.from_bytes(raw[48 * k:48 * k + 48], "little") for k in range(3 * G.nf)]
        assert all(v < G.P for v in vs), "a stored coordinate >= p"
        vs = [v * G.rinv % G.P for v in vs]
        out.append(tuple(G.ef(vs[k * G.nf:(k + 1) * G.nf]) for k in range(3)))
    return out


def project(G, t, hom):
    X, Y, Z = t
    F = G.F
    if Z == F.zero: return None
    zi = F.inv(Z)
    if hom: return (F.mul(X, zi), F.mul(Y, zi))
    z2 = F.mul(zi, zi)
    return (F.mul(X, z2), F.mul(Y, F.mul(z2, zi)))


def represent(G, pt, hom, rnd):
    """a random projective representation with Z != 1 (identity: Z = 0 with the other coordinates a valid, random, identity of that form)"""
    F = G.F
    z = G.rand_fe(rnd)
    while z == F.one: z = G.rand_fe(rnd)
    if pt is None: return (F.zero, z, F.zero) if hom else (F.mul(z, z), F.mul(F.mul(z, z), z), F.zero)
    if hom: return (F.mul(pt[0], z), F.mul(pt[1], z), z)
    z2 = F.mul(z, z)
    return (F.mul(pt[0], z2), F.mul(pt[1], F.mul(z2, z)), z)


def qwords(G, pt):
    """k_msm_extend_q's entry for a point: per Fp coordinate the 12 canonical words of coordinate * 2^392 mod p (field_edges.RP); the identity stays zero"""
    if pt is None: return [0] * (24 * G.nf)
    return [w for c in pt for v in G.fe(c) for w in _w12(v * field_edges.RP % G.P)]


# ---- the sort --------------------------------------------------------------------------------------------------------------------------------------------
SORT_SHAPES = [(4, 2, 1), (4, 2, 1023), (4, 2, 1024), (4, 2, 1025), (4, 3, 2049), (10, 1, 5000), (11, 1, 5000), (13, 2, 3000), (4, 480, 40), (4, 481, 40)]
SORT_CH = [1, 4, 64]
SORT_PATTERNS = ["zero", "one", "top", "uniform", "ch_edges", "last_only"]


def sort_tile(nwin, n):
    """msm.hpp msm_sort_tile restated"""
    tiles = 1 if nwin >= 480 else 480 // nwin
    t = -(-n // tiles)
    return -(-t // SORT_BLOCK) * SORT_BLOCK


def sort_digits(c, nwin, n, ch, pattern):
    """digits[nwin][n] as uint16"""
    nb = 1 << c
    rnd = np.random.RandomState((c * 1000003 + nwin * 1009 + n * 31 + ch) % (1 << 31))
    if pattern == "zero": d = np.zeros((nwin, n), dtype=np.uint16)
    elif pattern == "one": d = np.ones((nwin, n), dtype=np.uint16)
    elif pattern == "top": d = np.full((nwin, n), nb - 1, dtype=np.uint16)
    elif pattern == "uniform": d = rnd.randint(0, nb, size=(nwin, n)).astype(np.uint16)
    elif pattern == "last_only":
        d = np.zeros((nwin, n), dtype=np.uint16); d[:, n - 1] = [1 + (w * 7) % (nb - 1) for w in range(nwin)]
    else:
        # buckets 1, 2, 3, .. take ch - 1, ch, ch + 1, ch - 1, .. terms until the terms run out (a count of 0 leaves the bucket empty); the rest are digit 0;
        # the positions are shuffled so that a bucket's terms are spread over the tiles
        d = np.zeros((nwin, n), dtype=np.uint16)
        for w in range(nwin):
            row, b = [], 1
            while b < nb and len(row) + (ch - 1 + (b + w) % 3) <= n:
                row += [b] * (ch - 1 + (b + w) % 3); b += 1
            row += [0] * (n - len(row))
            d[w] = rnd.permutation(np.array(row, dtype=np.uint16))
    return d


def sort_model(c, nwin, n, ch, digits):
    """-> hist, offs, slot_offs [nwin][nb], slots_per_window [nwin], runs {(w, d): sorted index list}"""
    nb = 1 << c
    hist = np.zeros((nwin, nb), dtype=np.uint32)
    runs = {}
    for w in range(nwin):
        row = digits[w].astype(np.int64)
        cnt = np.bincount(row, minlength=nb); cnt[0] = 0
        hist[w] = cnt
        order = np.argsort(row, kind="stable")
        pos = int((row == 0).sum())
        for d in np.nonzero(cnt)[0]:
            runs[(w, int(d))] = order[pos:pos + cnt[d]].tolist(); pos += int(cnt[d])
    ns = (hist.astype(np.int64) + ch - 1) // ch
    offs = np.cumsum(hist, axis=1, dtype=np.int64) - hist
    slot_offs = np.cumsum(ns, axis=1) - ns
    return hist, offs.astype(np.uint32), slot_offs.astype(np.uint32), ns.sum(axis=1).astype(np.uint32), runs


# ---- the slot layout, lane free ---------------------------------------------------------------------------------------------------------------------------
def layout(hist_w, ch):
    """one window: (offs, slot_offs, slots per bucket, slots of the window)"""
    offs, so, ns, a, b = [], [], [], 0, 0
    for cnt in hist_w:
        offs.append(a); so.append(b); k = -(-int(cnt) // ch); ns.append(k); a += int(cnt); b += k
    return offs, so, ns, b


def slot_terms(run, ch):
    """the slots of one bucket: its run cut into ceil(cnt / ch) pieces"""
    return [run[k:k + ch] for k in range(0, len(run), ch)]


def leaders(ns, gmin, stride):
    """{leader slot (relative to the bucket's first): the slots it adds, itself first} of the grouping pass with this stride, for a bucket of ns slots"""
    if ns <= gmin * stride: return {}
    return {k0: [k for k in range(k0, min(k0 + SLOT_GROUP * stride, ns), stride)] for k0 in range(0, ns, SLOT_GROUP * stride)}


def merge_step(ns, gmin, passes):
    step = 1
    for _ in range(passes):
        if ns > gmin * step: step *= SLOT_GROUP
    return step


def engine_passes(n, ch, gmin):
    """the number of grouping passes msm_launch / msm_batch_dev launch"""
    passes, stride = 0, 1
    while passes < GROUP_PASSES and n // ch + 1 > gmin * stride: stride *= SLOT_GROUP; passes += 1
    return passes


def group_pass(G, vals, ns, gmin, stride):
    """one bucket's slot values (affine) after the pass: leaders hold their group's sum, the others are unchanged"""
    out = list(vals)
    for k0, members in leaders(ns, gmin, stride).items(): out[k0] = G.sum(vals[k] for k in members)
    return out


def merged(G, vals, gmin, passes):
    """what the merge reads after `passes` passes: the sum of every merge_step-th entry"""
    ns = len(vals)
    return G.sum(vals[k] for k in range(0, ns, merge_step(ns, gmin, passes)))


GROUP_SIZES = {1: [1, 2, 8, 9, 16, 17, 64, 65, 72, 73, 128, 129, 512, 513, 577], 2: [1, 2, 3, 15, 16, 17, 31, 32, 33, 127, 128, 129, 130, 255, 257]}


def group_case(tag, g2, c, nwin, gmin, hom):
    """-> hist [nwin][nb] (ch = 1: a bucket of cnt terms has cnt slots), per-(w, d) lists of slot values (affine model points) and of their projective
    representations.  Window 0 holds GROUP_SIZES[gmin] in its first 15 buckets; the other windows hold small buckets and empty ones.  Every bucket of more than
    8 slots starts with a group that cancels (P, -P, Q, -Q, ..) and, from 16 slots, continues with one that begins P, P; identities are sprinkled elsewhere."""
    G, pts = group(tag, g2), pool(tag, g2)
    nb = 1 << c
    rnd = random.Random("msm_edges group %s %d %d %d %d %d" % (tag, g2, c, nwin, gmin, hom))
    hist = np.zeros((nwin, nb), dtype=np.uint32)
    hist[0, 1:16] = GROUP_SIZES[gmin]
    for w in range(1, nwin):
        for d in range(1, nb): hist[w, d] = rnd.choice([0, 0, 1, 2, 3, 8, 9, 10])
    if c > 4: hist[0, nb - 1] = 9                                          # the last bucket, in the second block of the VM merge
    vals, reps = {}, {}
    for w in range(nwin):
        for d in range(nb):
            k = int(hist[w, d])
            if not k: continue
            v = [None if rnd.randrange(5) == 0 else pts[rnd.randrange(len(pts))] for _ in range(k)]
            if k > 8:
                for t in range(4): v[2 * t] = pts[t + d % 7]; v[2 * t + 1] = G.neg(pts[t + d % 7])
            if k >= 16: v[8] = v[9] = pts[d % len(pts)]
            vals[(w, d)] = v
            reps[(w, d)] = [represent(G, q, hom, rnd) for q in v]
    return hist, vals, reps


# ---- segments, reduce, finish -----------------------------------------------------------------------------------------------------------------------------
def segment_sum(G, buckets4, j):
    """sum_r (4 j + r) B_r over the four buckets of segment j"""
    return G.sum(G.mul(4 * j + r, b) for r, b in enumerate(buckets4) if b is not None and 4 * j + r)


def segment_case(tag, g2, nb):
    """-> (nwin, {(w, d): affine point}) -- nb = 16: four windows, segment j of window w has occupancy pattern 4 w + j (bit r: bucket 4 j + r), so all 16
    patterns occur and bucket 0 of segment 0 stays empty as the merge leaves it; nb = 32: two windows, seeded occupancy; nb = 8192: one window, the
    segments 0, 1, 2, 3, nseg / 2 - 1, nseg / 2, nseg - 1 full (except bucket 0)."""
    pts = pool(tag, g2)
    rnd = random.Random("msm_edges segments %s %d %d" % (tag, g2, nb))
    occ = {}
    if nb == 16:
        nwin = 4
        for w in range(4):
            for j in range(4):
                for r in range(4):
                    if ((4 * w + j) >> r) & 1: occ[(w, 4 * j + r)] = pts[rnd.randrange(len(pts))]
    elif nb == 32:
        nwin = 2
        for w in range(2):
            for d in range(1, 32):
                if rnd.randrange(3): occ[(w, d)] = pts[rnd.randrange(len(pts))]
    else:
        nwin, nseg = 1, nb // 4
        for j in (0, 1, 2, 3, nseg // 2 - 1, nseg // 2, nseg - 1):
            for r in range(4):
                if 4 * j + r: occ[(0, 4 * j + r)] = pts[rnd.randrange(len(pts))]
    return nwin, occ


def occupancy_patterns(nwin, nb, occ):
    return {(j >= 1, sum(1 << r for r in range(4) if (w, 4 * j + r) in occ)) for w in range(nwin) for j in range(nb // 4)}


REDUCE_NIN = [1, 2, 3, 4, 5, 16, 17, 2048]


def reduce_case(tag, g2, nin, nwin=2):
    pts = pool(tag, g2)
    rnd = random.Random("msm_edges reduce %s %d %d" % (tag, g2, nin))
    return [[None if rnd.randrange(4) == 0 else pts[rnd.randrange(len(pts))] for _ in range(nin)] for _ in range(nwin)]


def reduce_model(G, row): return [G.sum(row[k:k + SEG_FAN]) for k in range(0, len(row), SEG_FAN)]


FINISH_SHAPES = [(4, 1), (4, 2), (4, 64), (13, 10), (13, 20)]
FINISH_KINDS = ["random", "top_identity", "all_identity", "cancel"]


def finish_case(tag, g2, c, nwin, kind):
    """window sums W_0 .. W_(nwin - 1) (affine): random with identities; the top window the identity; all the identity; W_0 = -2^c W_1 and nothing else"""
    G, pts = group(tag, g2), pool(tag, g2)
    rnd = random.Random("msm_edges finish %s %d %d %d %s" % (tag, g2, c, nwin, kind))
    ws = [None if rnd.randrange(6) == 0 else pts[rnd.randrange(len(pts))] for _ in range(nwin)]
    if nwin > 1 and ws[nwin - 1] is None and kind == "random": ws[nwin - 1] = pts[0]
    if kind == "top_identity": ws[nwin - 1] = None
    elif kind == "all_identity": ws = [None] * nwin
    elif kind == "cancel":
        ws = [None] * nwin
        if nwin > 1: ws[1] = pts[3]; ws[0] = G.neg(G.mul(1 << c, pts[3]))
    return ws


def horner(G, c, ws):
    """sum_w 2^(c w) W_w, evaluated from the top window down (one scalar multiplication's worth of doublings instead of one per window)"""
    acc = None
    for q in reversed(ws): acc = G.add(G.mul(1 << c, acc), q)
    return acc


# ---- slot sums ------------------------------------------------------------------------------------------------------------------------------------------------
def term_point(tag, g2, bases, nreal, t):
    """the point term t stands for"""
    return image(tag, g2, bases[t % nreal], t // nreal)


def pipeline_model(tag, g2, bases, scalars, split, c, ch, gmin):
    """the composition of the stage models: digits (tests/fr_edges.py) -> sort -> slot sums -> grouping passes -> merge -> segments -> 4-ary tree -> Horner"""
    G = group(tag, g2)
    nreal = len(bases); n = split * nreal
    nbits = fr_edges.NBITS[split]; nwin = -(-nbits // c); nb = 1 << c
    plan = dict(c=c, nwin=nwin, nb=nb, n=n, nreal=nreal)
    fr_edges.check_plan(plan, split, nreal)
    digits = np.array(fr_edges.expected_digits(tag, plan, split, 1, {(0, i): k for i, k in enumerate(scalars)}), dtype=np.uint16).reshape(nwin, n)
    hist, offs, slot_offs, spw, runs = sort_model(c, nwin, n, ch, digits)
    passes = engine_passes(n, ch, gmin)
    wins = []
    for w in range(nwin):
        buckets = [None] * nb
        for d in range(1, nb):
            vals = [G.sum(term_point(tag, g2, bases, nreal, t) for t in piece) for piece in slot_terms(runs.get((w, d), []), ch)]
            for j in range(passes): vals = group_pass(G, vals, len(vals), gmin, SLOT_GROUP ** j)
            buckets[d] = merged(G, vals, gmin, passes)
        seg = [segment_sum(G, buckets[4 * j:4 * j + 4], j) for j in range(nb // 4)]
        while len(seg) > 1: seg = reduce_model(G, seg)
        wins.append(seg[0])
    return horner(G, c, wins)


def slot_exceptional(G, pts):
    """the throughput kernels' chain over a slot's term points, the identity bases skipped: the accumulator starts at the first point; an addition is exceptional
    when the accumulator equals the addend or its negative (a doubling or a cancellation).  Only the Fp2 form of the plain kernel also counts an identity base."""
    acc, first = None, True
    for q in pts:
        if q is None: continue
        if first: acc, first = q, False; continue
        if acc is None or acc[0] == q[0]: return True                    # (acc None: the chain cancelled earlier, which was exceptional already)
        acc = G.add(acc, q)
    return False


SLOT_CH = [1, 4, 32]
N_GENERIC = 64


def slot_case(tag, g2, split, ch):
    """-> dict(bases, nreal, n, hist [2][16], sorted [2][n] (the runs back to back, the rest unused), slots {(w, s): term list}, named {name: (w, s)}).
    Plan c = 4, nwin = 2.  Every named group of terms sits alone in a bucket, in the order given, so it is the bucket's first slot when it has <= ch terms."""
    G = group(tag, g2)
    gen = pool(tag, g2, N_GENERIC)
    P0, P1, P2 = gen[0], gen[1], gen[2]
    x0 = x0_point(tag, g2) if split == 1 else None
    special = [P0, P1, P2, G.neg(P0), G.add(P0, P1), G.neg(G.add(P0, P1)), None, P0, image(tag, g2, P1, 1) if split > 1 else gen[3], x0 if x0 is not None else gen[4]]
    bases = special + list(gen[5:])
    nreal = len(bases); n = split * nreal
    generic = [t for j in range(split) for t in range(j * nreal + len(special), (j + 1) * nreal)]            # distinct points, none related to the special ones
    assert len(generic) >= 34
    groups = [("one_term", [0]), ("exactly_ch", generic[:ch]), ("ch_plus_1", generic[1:ch + 2]), ("id_first", [6, 1, 2]), ("id_middle", [1, 6, 2]), ("id_last", [1, 2, 6]),
              ("id_only", [6]), ("id_only_2", [6, 6]), ("P_P", [0, 7]), ("P_negP", [0, 3]), ("P_negP_Q_R", [0, 3, 1, 2]), ("P_Q_PplusQ", [0, 1, 4]), ("P_Q_negPplusQ", [0, 1, 5])]
    if split > 1:
        groups += [("base_and_images", [1] + [j * nreal + 1 for j in range(1, split)]), ("image_doubling", [8, nreal + 1]), ("image_doubling_rev", [nreal + 1, 8])]
    if x0 is not None: groups += [("x0_first", [9, 1]), ("x0_alone", [9]), ("x0_last", [1, 2, 9])]
    assert len(groups) <= 30
    hist = np.zeros((2, 16), dtype=np.uint32)
    srt = np.zeros((2, n), dtype=np.uint32)
    slots, named, fill = {}, {}, [0, 0]
    for k, (name, terms) in enumerate(groups):
        w, d = k % 2, 1 + k // 2
        hist[w, d] = len(terms)
        srt[w, fill[w]:fill[w] + len(terms)] = terms; fill[w] += len(terms)
    for w in range(2):
        offs, so, ns, total = layout(hist[w], ch)
        for k, (name, terms) in enumerate(groups):
            if k % 2 != w: continue
            d = 1 + k // 2
            for part, piece in enumerate(slot_terms(terms, ch)): slots[(w, so[d] + part)] = piece
            named[name] = (w, so[d])
    return dict(bases=bases, nreal=nreal, n=n, hist=hist, sorted=srt, slots=slots, named=named, groups=dict(groups), x0=x0)


def slot_value(tag, g2, case, terms):
    G = group(tag, g2)
    return G.sum(term_point(tag, g2, case["bases"], case["nreal"], t) for t in terms)


def slot_is_exceptional(tag, g2, case, terms):
    return slot_exceptional(group(tag, g2), [term_point(tag, g2, case["bases"], case["nreal"], t) for t in terms])


FORCED_N, FORCED_CH = 1100, 2
FORCED_FLAT = [0, 15, 16, 17, 1023, 1024]                # and the last valid flat index


def forced_case(tag, g2, split):
    """plan c = 4, nwin = 2, ch = 2, n = 1100: nwin * max_slots = 1134 > 1024, so the second block of the fix-up walk has flag bytes to look at"""
    gen = pool(tag, g2, N_GENERIC)
    n = FORCED_N; nreal = n // split
    assert nreal * split == n
    bases = [gen[i % len(gen)] for i in range(nreal)]
    rnd = np.random.RandomState(split * 7 + g2)
    digits = rnd.randint(1, 16, size=(2, n)).astype(np.uint16)
    hist, offs, slot_offs, spw, runs = sort_model(4, 2, n, FORCED_CH, digits)
    srt = np.zeros((2, n), dtype=np.uint32)
    slots = {}
    for w in range(2):
        for d in range(1, 16):
            run = runs.get((w, d), [])
            srt[w, offs[w, d]:offs[w, d] + len(run)] = run
            for part, piece in enumerate(slot_terms(run, FORCED_CH)): slots[(w, int(slot_offs[w, d]) + part)] = piece
    max_slots = n // FORCED_CH + min(16, n) + 1
    return dict(bases=bases, nreal=nreal, n=n, hist=hist, offs=offs, slot_offs=slot_offs, spw=spw, sorted=srt, slots=slots, max_slots=max_slots)
