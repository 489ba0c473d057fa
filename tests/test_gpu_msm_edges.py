"""GPU (-m gpu): the stages of the Pippenger MSM behind the digit pass, one at a time, through the device harnesses tests/device/msm_edges.hip and
msm_slot_edges.hip (built from the production headers by build(): tests/device/build/libmsm_edges_{381,377}.so, libmsm_slot_edges_{381,377}.so), against the
plain model of tests/msm_edges.py (checked on the CPU by tests/test_msm_edges_model_cpu.py).

Every comparison of points is exact: the device's projective point is projected in the model and must EQUAL the model's affine point.  Every output array
comes back whole, with the harness's slack behind it: what a stage must not write still holds the sentinel.  The plan is passed as 8 words, so a test picks
c, nwin, ch and gmin freely; the launch geometry is the engine's (quoted in the harness)."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import msm_edges as E

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U32P = ctypes.POINTER(ctypes.c_uint32)
U16P = ctypes.POINTER(ctypes.c_uint16)
U8P = ctypes.POINTER(ctypes.c_uint8)
GROUPS = [(t, g) for t in E.TAGS for g in (0, 1)]
IDS = ["%s-%s" % (t, "g2" if g else "g1") for t, g in GROUPS]


def _p(a, t=U32P): return a.ctypes.data_as(t)


def plan_words(c, nwin, n, ch, nreal=None, gmin=16):
    return np.array([c, nwin, 1 << c, n, ch, 4, n if nreal is None else nreal, gmin], dtype=np.uint32)


class Harness:
    def __init__(self, tag):
        self.tag = tag
        for name in ("msm_edges", "msm_slot_edges"):
            path = os.path.join(HERE, "device", "build", "lib%s_%s.so" % (name, tag))
            assert os.path.exists(path), "device harness missing: %s (build() builds it: make -C tests/device)" % path
            setattr(self, name, ctypes.CDLL(path))
        info = np.zeros(16, dtype=np.uint32)
        self.msm_edges.ms_info(_p(info))
        assert info[0] == int(tag) and info[2] == E.SORT_BLOCK and info[3] == E.SLOT_GROUP and info[4] == E.GROUP_PASSES and info[5] == E.SEG_FAN and info[6] == 4 and info[9] == 144
        self.fix_grid, self.sentinel, self.slack = int(info[1]), int(info[7]), int(info[8])
        assert self.fix_grid == 128 and self.slack == 64
        info2 = np.zeros(16, dtype=np.uint32)
        self.msm_slot_edges.mss_info(_p(info2))
        assert info2[0] == int(tag) and info2[1] == self.fix_grid and info2[2] == self.sentinel and info2[3] == self.slack
        self.msm_edges.ms_sort_tile.restype = ctypes.c_uint32

    def _rc(self, rc, what):
        if rc > 0: pytest.exit("%s: HIP error %d -- nothing more is started on this device" % (what, rc), returncode=3)
        assert rc == 0, what + " refused its arguments"

    def full(self, shape): return np.full(shape, self.sentinel, dtype=np.uint32)

    def sort(self, pw, digits, lds, hist_in=None):
        nwin, nb, n = int(pw[1]), int(pw[2]), int(pw[3])
        nwb = nwin * nb
        hist = np.zeros(nwb + 64, dtype=np.uint32)
        if hist_in is not None: hist[:nwb] = hist_in.reshape(-1)
        offs, cursor, so, spw, srt = (np.zeros(k, dtype=np.uint32) for k in (nwb + 64, nwb + 64, nwb + 64, nwin + 64, nwin * n + 64))
        tiles = ctypes.c_uint32(0)
        d = np.ascontiguousarray(digits, dtype=np.uint16)
        self._rc(self.msm_edges.ms_sort(_p(pw), _p(d, U16P), int(lds), _p(hist), _p(offs), _p(cursor), _p(so), _p(spw), _p(srt), ctypes.byref(tiles)), "ms_sort")
        return dict(hist=hist, offs=offs, cursor=cursor, slot_offs=so, spw=spw, sorted=srt, tiles=tiles.value)

    def group(self, g2, pw, hist, so, spw, slots, max_slots, stride, hom):
        out = np.ascontiguousarray(slots).copy()
        self._rc(self.msm_edges.ms_group(int(g2), _p(pw), _p(hist), _p(so), _p(spw), _p(out), ctypes.c_uint32(max_slots), ctypes.c_uint32(stride), int(hom)), "ms_group")
        return out

    def merge(self, g2, kind, pw, hist, so, spw, slots, max_slots, passes, hom, jw):
        out = np.zeros((int(pw[1]) * int(pw[2]) + 64, jw), dtype=np.uint32)
        s = np.ascontiguousarray(slots)
        self._rc(self.msm_edges.ms_merge(int(g2), kind, _p(pw), _p(hist), _p(so), _p(spw), _p(s), ctypes.c_uint32(max_slots), ctypes.c_uint32(passes), int(hom), _p(out)), "ms_merge")
        return out

    def segments(self, g2, vm, pw, buckets, nseg, jw):
        out = np.zeros((int(pw[1]) * nseg + 64, jw), dtype=np.uint32)
        b = np.ascontiguousarray(buckets)
        self._rc(self.msm_edges.ms_segments(int(g2), int(vm), _p(pw), _p(b), ctypes.c_uint32(nseg), _p(out)), "ms_segments")
        return out

    def reduce(self, g2, vm, arr, nin, nwin, jw):
        nout = -(-nin // 4)
        out = np.zeros((nwin * nout + 64, jw), dtype=np.uint32)
        a = np.ascontiguousarray(arr)
        self._rc(self.msm_edges.ms_reduce(int(g2), int(vm), _p(a), ctypes.c_uint32(nin), ctypes.c_uint32(nwin), _p(out), ctypes.c_uint32(nout)), "ms_reduce")
        return out

    def finish(self, g2, kind, pw, seg, nseg, jw):
        win, out = np.zeros((64 + 64, jw), dtype=np.uint32), np.zeros((1 + 64, jw), dtype=np.uint32)
        s = np.ascontiguousarray(seg)
        self._rc(self.msm_edges.ms_finish(int(g2), kind, _p(pw), _p(s), ctypes.c_uint32(nseg), _p(win), _p(out)), "ms_finish")
        return win, out

    def finish_batch(self, g2, pw, rows, win, jw):
        out = np.zeros((rows + 64, jw), dtype=np.uint32)
        s = np.ascontiguousarray(win)
        self._rc(self.msm_edges.ms_finish_batch(int(g2), _p(pw), ctypes.c_uint32(rows), _p(s), _p(out)), "ms_finish_batch")
        return out

    def extend(self, g2, bases, split):
        n = len(bases)
        out = np.zeros((split * n + 64, bases.shape[1]), dtype=np.uint32)
        b = np.ascontiguousarray(bases)
        self._rc(self.msm_slot_edges.mss_extend(int(g2), _p(b), ctypes.c_uint32(n), split, _p(out)), "mss_extend")
        return out

    def slot_sum(self, g2, form, pw, bases, hist, offs, so, spw, srt, max_slots, hom, flag, slots):
        """-> (flag after, slot sums after the first launch, slot sums at the end); flag and slots are the caller's initial buffers (not modified)"""
        fl, mid, out = np.ascontiguousarray(flag).copy(), np.zeros_like(slots), np.ascontiguousarray(slots).copy()
        args = [np.ascontiguousarray(a, dtype=np.uint32) for a in (bases, hist, offs, so, spw, srt)]
        self._rc(self.msm_slot_edges.mss_slot_sum(int(g2), form, _p(pw), *[_p(a) for a in args], ctypes.c_uint32(max_slots), int(hom), _p(fl, U8P), _p(mid), _p(out)), "mss_slot_sum")
        return fl, mid, out


@functools.lru_cache(maxsize=None)
def harness(tag): return Harness(tag)


def is_sentinel(H, arr): return (np.asarray(arr) == H.sentinel).all()


def points(G, rows, hom):
    """device rows -> affine model points (None = the identity)"""
    return [E.project(G, t, hom) for t in E.unpack_proj(G, rows)]


# ---- the sort ---------------------------------------------------------------------------------------------------------------------------------------------------------
def check_sort(H, res, c, nwin, n, ch, digits, lds, what):
    nb = 1 << c
    nwb = nwin * nb
    hist, offs, so, spw, runs = E.sort_model(c, nwin, n, ch, digits)
    assert res["tiles"] == -(-n // E.sort_tile(nwin, n)), (what, "tiles", res["tiles"])
    assert np.array_equal(res["hist"][:nwb].reshape(nwin, nb), hist), (what, "hist")
    assert (res["hist"][:nwb].reshape(nwin, nb)[:, 0] == 0).all(), (what, "bucket 0 counted")
    assert np.array_equal(res["offs"][:nwb].reshape(nwin, nb), offs), (what, "offs")
    assert np.array_equal(res["slot_offs"][:nwb].reshape(nwin, nb), so), (what, "slot_offs")
    assert np.array_equal(res["spw"][:nwin], spw), (what, "slots_per_window")
    assert np.array_equal(res["cursor"][:nwb].reshape(nwin, nb), offs + hist), (what, "cursor != offs + hist after the scatter")
    for name, valid in (("hist", nwb), ("offs", nwb), ("cursor", nwb), ("slot_offs", nwb), ("spw", nwin), ("sorted", nwin * n)):
        assert is_sentinel(H, res[name][valid:]), (what, name, "the slack behind the array was written")
    srt = res["sorted"][:nwin * n].reshape(nwin, n)
    for w in range(nwin):
        total = int(hist[w].sum())
        assert is_sentinel(H, srt[w, total:]), (what, "window", w, "a position at or beyond sum(hist) was written")
        for d in np.nonzero(hist[w])[0]:
            run = srt[w, offs[w, d]:offs[w, d] + hist[w, d]]
            assert sorted(run.tolist()) == runs[(w, int(d))], (what, "window", w, "bucket", int(d))


@pytest.mark.parametrize("tag", E.TAGS)
@pytest.mark.parametrize("c,nwin,n", E.SORT_SHAPES, ids=["c%d-w%d-n%d" % s for s in E.SORT_SHAPES])
def test_sort(tag, c, nwin, n):
    H = harness(tag)
    for ch in E.SORT_CH:
        pw = plan_words(c, nwin, n, ch)
        assert H.msm_edges.ms_sort_tile(_p(pw)) == E.sort_tile(nwin, n)                 # the model's tile is the engine's msm_sort_tile
        for pat in E.SORT_PATTERNS:
            digits = E.sort_digits(c, nwin, n, ch, pat)
            res = H.sort(pw, digits, 1)                                               # k_msm_hist_lds, k_msm_scan, k_msm_scatter_lds
            check_sort(H, res, c, nwin, n, ch, digits, 1, ("lds", c, nwin, n, ch, pat))
            if (c, nwin, n) == (4, 2, 1025): assert res["tiles"] == 2
            if (c, nwin, n) == (4, 3, 2049): assert res["tiles"] == 3
            hist = E.sort_model(c, nwin, n, ch, digits)[0]
            res = H.sort(pw, digits, 0, hist_in=hist)                                 # k_msm_scan, k_msm_scatter on the model's histogram
            check_sort(H, res, c, nwin, n, ch, digits, 0, ("lane per term", c, nwin, n, ch, pat))


# ---- extended bases -----------------------------------------------------------------------------------------------------------------------------------------------------
def extend_bases(tag, g2, n, split):
    """base i: the pool cycled with period 19 (256 = 9 mod 19: a lane that reads a neighbouring block's base gets another point), the identity at i = 7 mod 19 and, unsplit
    G1 only, the x = 0 point at i = 11 mod 19; n = 1 variants are built by the caller"""
    pts, x0 = E.pool(tag, g2), E.x0_point(tag, g2) if split == 1 else None
    return [None if i % 19 == 7 else x0 if (x0 is not None and i % 19 == 11) else pts[i % 19] for i in range(n)]


@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
def test_extend_q(tag, g2):
    H, G = harness(tag), E.group(tag, g2)
    for split in (1, G.split):
        x0 = E.x0_point(tag, g2) if split == 1 else None
        sets = [extend_bases(tag, g2, n, split) for n in (1, 255, 256, 257)] + [[None]] + ([[x0]] if x0 is not None else [])
        for bases in sets:
            n = len(bases)
            ext = H.extend(g2, E.pack_affine(G, bases), split)
            assert is_sentinel(H, ext[split * n:]), ("slack", split, n)
            for j in range(split):
                for i, b in enumerate(bases):
                    want = np.array(E.qwords(G, E.image(tag, g2, b, j)), dtype=np.uint32)
                    assert np.array_equal(ext[j * n + i], want), ("image", j, "base", i, "of", n, "split", split)
            if x0 is not None and n > 11: assert ext[11].any() and not ext[7].any()         # the x = 0 point does not read as the identity; the identity stays all zero


# ---- slot sums ------------------------------------------------------------------------------------------------------------------------------------------------------------
SLOT_FORMS = [(0, 0, "k_msm_slot_sum jac"), (0, 1, "k_msm_slot_sum hom"), (1, 0, "k_msm_slot_sum_q + fix jac"), (1, 1, "k_msm_slot_sum_q + fix hom"), (2, 1, "k_msm_slot_sum_q + fix_vm")]


def slot_layout_arrays(case, ch):
    offs, so, spw = np.zeros((2, 16), dtype=np.uint32), np.zeros((2, 16), dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    for w in range(2):
        o, s, ns, total = E.layout(case["hist"][w], ch)
        offs[w], so[w], spw[w] = o, s, total
    return offs, so, spw


@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
@pytest.mark.parametrize("ch", E.SLOT_CH)
def test_slot_sums(tag, g2, ch):
    H, G = harness(tag), E.group(tag, g2)
    jw = 36 * G.nf
    for split in (1, G.split):
        case = E.slot_case(tag, g2, split, ch)
        n, nreal = case["n"], case["nreal"]
        pw = plan_words(4, 2, n, ch, nreal)
        max_slots = n // ch + min(16, n) + 1                                              # msm_launch's
        offs, so, spw = slot_layout_arrays(case, ch)
        want = {ws: E.slot_value(tag, g2, case, terms) for ws, terms in case["slots"].items()}
        exc = {ws for ws, terms in case["slots"].items() if E.slot_is_exceptional(tag, g2, case, terms)}
        assert all(s < spw[w] for (w, s) in want) and len(want) == int(spw.sum()) and max(spw) <= max_slots
        if ch >= 4: assert len(exc) >= 5
        bases = E.pack_affine(G, case["bases"])
        flag0 = np.full(2 * max_slots + 64, 0xFF, dtype=np.uint8)                          # the state of a reused buffer
        slots0 = H.full((2 * max_slots + 64, jw))
        for form, hom, name in SLOT_FORMS:
            what = (name, "split", split, "ch", ch)
            fl, mid, out = H.slot_sum(g2, form, pw, bases, case["hist"], offs, so, spw, case["sorted"], max_slots, hom, flag0, slots0)
            assert is_sentinel(H, out[2 * max_slots:]) and is_sentinel(H, mid[2 * max_slots:]), (what, "slack")
            for w in range(2):
                lo, k = w * max_slots, int(spw[w])
                assert is_sentinel(H, out[lo + k:lo + max_slots]), (what, "window", w, "a slot at or beyond slots_per_window was written")
                assert is_sentinel(H, mid[lo + k:lo + max_slots]), (what, "window", w, "a slot at or beyond slots_per_window was written by the throughput kernel")
                if form: assert (fl[lo + k:lo + max_slots] == 0xFF).all(), (what, "a flag byte at or beyond slots_per_window was written")
                got = points(G, out[lo:lo + k], hom)
                for s in range(k): assert got[s] == want[(w, s)], (what, "window", w, "slot", s, case["slots"][(w, s)])
                if form:
                    for s in range(k):
                        flagged = fl[lo + s] != 0
                        if (w, s) in exc: assert flagged, (what, "window", w, "slot", s, "an exceptional slot was not flagged")
                        if flagged: assert is_sentinel(H, mid[lo + s]), (what, "window", w, "slot", s, "the throughput kernel stored a flagged slot")
                        else: assert points(G, mid[lo + s:lo + s + 1], hom)[0] == want[(w, s)], (what, "window", w, "slot", s, "an unflagged slot was wrong before the fix")
            if form: assert (fl[2 * max_slots:] == 0xFF).all(), (what, "flag slack")


@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
def test_slot_sum_fix_forced_flags(tag, g2):
    """flags set by hand over a walk of two blocks' worth of bytes: exactly those slots are rewritten, correctly; every other word stays as it was"""
    H, G = harness(tag), E.group(tag, g2)
    jw = 36 * G.nf
    for split in (1, G.split):
        fc = E.forced_case(tag, g2, split)
        n, ms = fc["n"], fc["max_slots"]
        pw = plan_words(4, 2, n, E.FORCED_CH, fc["nreal"])
        flat = E.FORCED_FLAT + [ms + int(fc["spw"][1]) - 1]
        flag0 = np.zeros(2 * ms + 64, dtype=np.uint8); flag0[flat] = 1
        flag0[int(fc["spw"][0]):ms] = 0xFF                                               # stale bytes behind window 0's slots: no slot there
        slots0 = H.full((2 * ms + 64, jw))
        bases = E.pack_affine(G, fc["bases"])
        for form, hom in ((3, 0), (3, 1), (4, 1)):
            fl, mid, out = H.slot_sum(g2, form, pw, bases, fc["hist"], fc["offs"], fc["slot_offs"], fc["spw"], fc["sorted"], ms, hom, flag0, slots0)
            assert np.array_equal(fl, flag0) and np.array_equal(mid, slots0), (form, hom, "the fix-up kernel's inputs changed")
            keep = np.ones(len(out), dtype=bool); keep[flat] = False
            assert is_sentinel(H, out[keep]), (form, hom, split, "a slot that was not flagged (or has no terms) was written", np.nonzero((out != H.sentinel).any(axis=1) & keep)[0][:8])
            for f in flat:
                w, s = divmod(f, ms)
                assert points(G, out[f:f + 1], hom)[0] == E.slot_value(tag, g2, fc, fc["slots"][(w, s)]), (form, hom, split, "flat", f)


# ---- grouping and merge -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
@pytest.mark.parametrize("c,nwin,gmin", [(4, 2, 1), (5, 5, 1), (4, 5, 2), (5, 2, 2)])
def test_group_and_merge(tag, g2, c, nwin, gmin):
    H, G = harness(tag), E.group(tag, g2)
    jw, nb = 36 * G.nf, 1 << c
    for hom in (1, 0):
        hist, vals, reps = E.group_case(tag, g2, c, nwin, gmin, hom)
        n = int(hist.sum(axis=1).max())
        pw = plan_words(c, nwin, n, 1, n, gmin)                                             # ch = 1: a bucket of cnt terms has cnt slots
        max_slots = n // 1 + min(nb, n) + 1
        assert E.engine_passes(n, 1, gmin) == 3                                           # the engine's formula is the explicit passes = 3 below
        so, spw = np.zeros((nwin, nb), dtype=np.uint32), np.zeros(nwin, dtype=np.uint32)
        slots = H.full((nwin * max_slots + 64, jw))
        for w in range(nwin):
            _, s, ns, total = E.layout(hist[w], 1)
            so[w], spw[w] = s, total
            for d in range(nb):
                if (w, d) in reps: slots[w * max_slots + s[d]:w * max_slots + s[d] + ns[d]] = E.pack_proj(G, reps[(w, d)])
        sums = {k: G.sum(v) for k, v in vals.items()}
        cur = {k: list(v) for k, v in vals.items()}
        for passes in range(4):
            # the merges after `passes` grouping passes
            kinds = ((0, "k_msm_vm_merge"), (1, "k_msm_bucket_merge hom")) if hom else ((1, "k_msm_bucket_merge jac"),)
            for kind, name in kinds:
                b = H.merge(g2, kind, pw, hist, so, spw, slots[:nwin * max_slots], max_slots, passes, hom, jw)
                assert is_sentinel(H, b[nwin * nb:]), (name, passes, "a bucket d >= nb was written")
                got = points(G, b[:nwin * nb], hom)
                for w in range(nwin):
                    for d in range(nb): assert got[w * nb + d] == sums.get((w, d)), (name, "passes", passes, "window", w, "bucket", d, "slots", int(hist[w, d]))
            if passes == 3: break
            stride = 8 ** passes
            after = H.group(g2, pw, hist, so, spw, slots, max_slots, stride, hom)
            changed = set(np.nonzero((after != slots).any(axis=1))[0].tolist())
            lead = {}
            for (w, d), v in cur.items():
                for k0 in E.leaders(len(v), gmin, stride): lead[w * max_slots + int(so[w, d]) + k0] = (w, d, k0)
            assert changed <= set(lead), ("stride", stride, "hom", hom, "an entry that leads no group changed", sorted(changed - set(lead))[:8])
            nxt = {k: E.group_pass(G, v, len(v), gmin, stride) for k, v in cur.items()}
            idx = sorted(lead)
            got = points(G, after[idx], hom)
            for f, q in zip(idx, got):
                w, d, k0 = lead[f]
                assert q == nxt[(w, d)][k0], ("stride", stride, "hom", hom, "window", w, "bucket", d, "leader", k0, "of", len(cur[(w, d)]))
            cur, slots = nxt, after


# ---- segments, reduce, finish -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
@pytest.mark.parametrize("nb", [16, 32, 8192])
def test_segments(tag, g2, nb):
    H, G = harness(tag), E.group(tag, g2)
    jw, nseg = 36 * G.nf, nb // 4
    nwin, occ = E.segment_case(tag, g2, nb)
    want = {(w, j): E.segment_sum(G, [occ.get((w, 4 * j + r)) for r in range(4)], j) for w in range(nwin) for j in range(nseg) if any((w, 4 * j + r) in occ for r in range(4))}
    pw = plan_words(nb.bit_length() - 1, nwin, 64, 4)
    for vm, name in ((1, "k_msm_vm_segments"), (0, "k_msm_segments")):
        rnd = random.Random("segments %s %d %d %d" % (tag, g2, nb, vm))
        ident = E.pack_proj(G, [E.represent(G, None, vm, rnd) for _ in range(8)])
        buckets = ident[np.arange(nwin * nb) % 8]                                          # empty buckets: identities in several representations
        keys = sorted(occ)
        buckets[[w * nb + d for w, d in keys]] = E.pack_proj(G, [E.represent(G, occ[k], vm, rnd) for k in keys])
        seg = H.segments(g2, vm, pw, buckets, nseg, jw)
        assert is_sentinel(H, seg[nwin * nseg:]), (name, "slack")
        rows = sorted(want)
        got = points(G, seg[[w * nseg + j for w, j in rows]], vm)
        for (w, j), q in zip(rows, got): assert q == want[(w, j)], (name, "window", w, "segment", j)
        rest = np.ones(nwin * nseg, dtype=bool); rest[[w * nseg + j for w, j in rows]] = False
        zcol = seg[:nwin * nseg][rest][:, 2 * jw // 3:]
        assert not zcol.any(), (name, "an empty segment is not the identity")               # Z = 0: Montgomery zero is all zero words


@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
def test_reduce(tag, g2):
    H, G = harness(tag), E.group(tag, g2)
    jw = 36 * G.nf
    for nin in E.REDUCE_NIN:
        rows = E.reduce_case(tag, g2, nin)
        want = [E.reduce_model(G, r) for r in rows]
        nout = -(-nin // 4)
        for vm, name in ((1, "k_msm_vm_reduce"), (0, "k_msm_seg_reduce")):
            rnd = random.Random("reduce %s %d %d %d" % (tag, g2, nin, vm))
            uniq = {}
            for r in rows:
                for q in r:
                    if q not in uniq: uniq[q] = E.pack_proj(G, [E.represent(G, q, vm, rnd)])[0]
            arr = np.array([uniq[q] for r in rows for q in r], dtype=np.uint32)
            out = H.reduce(g2, vm, arr, nin, 2, jw)
            assert is_sentinel(H, out[2 * nout:]), (name, nin, "the sentinel behind nout")
            got = points(G, out[:2 * nout], vm)
            for w in range(2):
                for j in range(nout): assert got[w * nout + j] == want[w][j], (name, "nin", nin, "window", w, "group", j)


def jac_inf_words(G):
    one = E._w12(E.R384 % G.P)
    fe = one + [0] * 12 if G.g2 else one
    return np.array(fe + fe + [0] * (12 * G.nf), dtype=np.uint32)


@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
@pytest.mark.parametrize("c,nwin", E.FINISH_SHAPES, ids=["c%d-w%d" % s for s in E.FINISH_SHAPES])
def test_finish(tag, g2, c, nwin):
    H, G = harness(tag), E.group(tag, g2)
    jw = 36 * G.nf
    pw = plan_words(c, nwin, 64, 4)
    cases = {kind: E.finish_case(tag, g2, c, nwin, kind) for kind in E.FINISH_KINDS}
    want = {kind: E.horner(G, c, ws) for kind, ws in cases.items()}
    assert want["all_identity"] is None and (nwin == 1 or want["cancel"] is None) and want["random"] is not None
    rnd = random.Random("finish %s %d %d %d" % (tag, g2, c, nwin))
    for kind, ws in cases.items():
        # k_msm_finish_vm: one homogeneous sum per window
        seg = E.pack_proj(G, [E.represent(G, q, 1, rnd) for q in ws])
        win, out = H.finish(g2, 0, pw, seg, 1, jw)
        assert np.array_equal(win[:nwin], seg) and is_sentinel(H, win[nwin:]), ("k_msm_finish_vm", kind, "the window array: nwin copies, nothing behind them")
        assert is_sentinel(H, out[1:]), ("k_msm_finish_vm", kind, "slack")
        assert points(G, out[:1], 0)[0] == want[kind], ("k_msm_finish_vm", kind)
        if want[kind] is None: assert np.array_equal(out[0], jac_inf_words(G)), ("k_msm_finish_vm", kind, "the identity is jac_inf")
        # k_msm_finish: nseg Jacobian sums per window
        for nseg in (1, 4):
            parts = []
            for q in ws:
                if nseg == 1: parts.append(q); continue
                a, b = E.pool(tag, g2)[rnd.randrange(20)], E.pool(tag, g2)[rnd.randrange(20)]
                parts += [a, None, b, G.add(q, G.neg(G.add(a, b)))]
            seg = E.pack_proj(G, [E.represent(G, q, 0, rnd) for q in parts])
            win, out = H.finish(g2, 1, pw, seg, nseg, jw)
            assert is_sentinel(H, win[nwin:]) and is_sentinel(H, out[1:]), ("k_msm_finish", kind, nseg, "slack")
            assert points(G, win[:nwin], 0) == ws, ("k_msm_finish", kind, nseg, "window sums")
            assert points(G, out[:1], 0)[0] == want[kind], ("k_msm_finish", kind, nseg)
    # k_msm_finish_vm_batch: rows of window sums, four per block; five rows leave one active group and three idle ones in a second block
    kinds = E.FINISH_KINDS
    for rows in (1, 3, 4, 5):
        order = [kinds[(r + rows) % 4] for r in range(rows)]
        win = E.pack_proj(G, [E.represent(G, q, 1, rnd) for k in order for q in cases[k]])
        out = H.finish_batch(g2, pw, rows, win, jw)
        assert is_sentinel(H, out[rows:]), ("k_msm_finish_vm_batch", rows, "slack")
        got = points(G, out[:rows], 0)
        for r, k in enumerate(order):
            assert got[r] == want[k], ("k_msm_finish_vm_batch", "rows", rows, "row", r, k)
            if want[k] is None: assert np.array_equal(out[r], jac_inf_words(G)), ("k_msm_finish_vm_batch", "row", r, "the identity is jac_inf")
