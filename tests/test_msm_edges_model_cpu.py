"""CPU: the plain model of the Pippenger stages (tests/msm_edges.py) and the inputs of tests/test_gpu_msm_edges.py.

  * the composition of the stage models -- digits, sort, slot sums, grouping passes, merge, segment sums, 4-ary tree, Horner -- reproduces g1_msm / g2_msm of
    tests/model for 40 bases with random 255-bit scalars, on both curves and with every split;
  * every input set holds the edges it is there for, counted: the GPU test runs exactly these builders."""
import random

import numpy as np
import pytest

import fr_edges
import msm_edges as E

GROUPS = [(t, g) for t in E.TAGS for g in (0, 1)]
IDS = ["%s-%s" % (t, "g2" if g else "g1") for t, g in GROUPS]


@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
@pytest.mark.parametrize("c,ch,gmin", [(4, 2, 1), (5, 1, 2)])
def test_the_stage_models_compose_to_the_msm(tag, g2, c, ch, gmin):
    G, m = E.group(tag, g2), E.MODELS[tag]
    rnd = random.Random("msm_edges compose %s %d" % (tag, g2))
    bases = list(E.pool(tag, g2, E.N_GENERIC)[:39]) + [None]                     # 40 bases, one of them the identity
    scalars = [rnd.randrange(G.r >> 1, G.r) for _ in range(38)] + [G.r - 1, rnd.randrange(G.r >> 1, G.r)]        # full length: 255 bits (253 on BLS12-377)
    real = [(b, k) for b, k in zip(bases, scalars) if b is not None]
    expect = (m.g2_msm if g2 else m.g1_msm)([b for b, _ in real], [k for _, k in real])
    assert expect is not None
    for split in (1, G.split):
        assert E.pipeline_model(tag, g2, bases, scalars, split, c, ch, gmin) == expect, split
    if ch == 2: assert E.engine_passes(40, ch, gmin) >= 2                               # the grouping passes are part of the composition


@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
def test_images_are_the_endomorphisms(tag, g2):
    """the scalar-multiplication images are what the kernels form with one or two field products: phi(x, y) = (beta x, y) on G1 (same y, another x);
    on G2 the four images are distinct points of the curve"""
    G = E.group(tag, g2)
    q = E.pool(tag, g2)[1]
    imgs = [E.image(tag, g2, q, j) for j in range(G.split)]
    assert len(set(imgs)) == G.split and all(G.on_curve(i) for i in imgs)
    if not g2: assert imgs[1][1] == q[1] and imgs[1][0] != q[0] and pow(imgs[1][0] * pow(q[0], -1, G.P), 3, G.P) == 1
    assert G.mul(G.r, q) is None


def test_the_x0_point():
    for tag in E.TAGS:
        p = E.x0_point(tag, 0)
        assert p is not None and p[0] == 0 and p[1] != 0 and E.group(tag, 0).on_curve(p)
        assert E.group(tag, 0).mul(3, p) is None                                  # of order 3: outside the prime-order subgroup, so it enters unsplit sums only
        assert E.x0_point(tag, 1) is None                                         # b' is no square in Fp2 on either curve: the twist has no point with x = 0


def test_projection_round_trip():
    for tag, g2 in GROUPS:
        G = E.group(tag, g2)
        rnd = random.Random(5)
        for hom in (0, 1):
            for q in (E.pool(tag, g2)[2], None):
                t = E.represent(G, q, hom, rnd)
                assert t[2] != G.F.one and E.project(G, t, hom) == q
                assert E.project(G, E.unpack_proj(G, E.pack_proj(G, [t]))[0], hom) == q


# ---- the sort ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_sort_shapes_hold_their_edges():
    tiles = {(c, nwin, n): -(-n // E.sort_tile(nwin, n)) for c, nwin, n in E.SORT_SHAPES}
    assert tiles[(4, 2, 1025)] == 2 and tiles[(4, 3, 2049)] == 3 and tiles[(4, 2, 1024)] == 1 and tiles[(4, 2, 1023)] == 1
    assert 1025 - E.sort_tile(2, 1025) == 1 and 2049 - 2 * E.sort_tile(3, 2049) == 1           # the last tile holds exactly one term
    assert E.sort_tile(480, 40) == E.sort_tile(481, 40) == 1024 and 480 // 480 == 1 and 480 // 479 == 1      # either side of the nwin >= 480 branch
    assert (1 << 13) == 8192 and (8192 + 1023) // 1024 == 8                       # c = 13: the full counter array, per = 8 in k_msm_scan
    assert (1 << 11) // 1024 == 2 and (1 << 10) // 1024 == 1                      # c = 10 / 11: one / two counters per lane of the scan
    for c, nwin, n in E.SORT_SHAPES:
        nb = 1 << c
        for ch in E.SORT_CH:
            for pat in E.SORT_PATTERNS:
                d = E.sort_digits(c, nwin, n, ch, pat)
                assert d.shape == (nwin, n) and d.dtype == np.uint16 and int(d.max()) < nb
                hist, offs, so, spw, runs = E.sort_model(c, nwin, n, ch, d)
                assert (hist[:, 0] == 0).all() and int(hist.sum()) == int((d != 0).sum())
                assert all(sorted(v) == v and all(d[w, i] == b for i in v) for (w, b), v in runs.items())
                if pat == "zero": assert not runs
                if pat == "one": assert (hist[:, 1] == n).all() and int(spw[0]) == -(-n // ch)
                if pat == "top": assert (hist[:, nb - 1] == n).all()
                if pat == "last_only": assert int(hist.sum()) == nwin and all(v == [n - 1] for v in runs.values())
                if pat == "ch_edges" and n >= 3 * ch + 3:
                    got = set(hist[0, 1:4].tolist())
                    assert got == {ch - 1, ch, ch + 1}, (c, nwin, n, ch, got)
                if pat == "ch_edges" and ch == 64 and n >= 1025:                             # a bucket's terms are spread over the tiles
                    t = E.sort_tile(nwin, n)
                    assert any(min(v) < t <= max(v) for v in runs.values())


# ---- grouping and merge -----------------------------------------------------------------------------------------------------------------------------------------------
def test_group_sizes_sit_on_every_threshold():
    for gmin, sizes in E.GROUP_SIZES.items():
        assert len(sizes) == 15
        for s in (gmin, gmin + 1, 8 * gmin, 8 * gmin + 1, 64 * gmin, 64 * gmin + 1): assert s in sizes, (gmin, s)
    assert {8, 9, 64, 65, 512, 513, 577} <= set(E.GROUP_SIZES[1])                # also the sizes at which a group of 8 (64, 512) is exactly full
    # leaders: a bucket of exactly gmin * stride slots has none, one more has
    for gmin in (1, 2):
        for stride in (1, 8, 64):
            assert E.leaders(gmin * stride, gmin, stride) == {} and E.leaders(gmin * stride + 1, gmin, stride)
    assert E.leaders(17, 1, 1) == {0: list(range(8)), 8: list(range(8, 16)), 16: [16]}
    assert E.leaders(577, 1, 64) == {0: list(range(0, 512, 64)), 512: [512, 576]}
    assert E.merge_step(577, 1, 3) == 512 and E.merge_step(64, 1, 3) == 64 and E.merge_step(65, 1, 3) == 512 and E.merge_step(8, 1, 3) == 8 and E.merge_step(2, 2, 3) == 1
    assert E.engine_passes(1 << 20, 64, 16) == 3 and E.engine_passes(64, 4, 16) == 1 and E.engine_passes(40, 4, 16) == 0


@pytest.mark.parametrize("gmin", [1, 2])
def test_group_case_holds_cancelling_groups_doublings_and_identities(gmin):
    tag, g2 = "381", 0
    G = E.group(tag, g2)
    for c, nwin in [(4, 2), (5, 5)]:
        hist, vals, reps = E.group_case(tag, g2, c, nwin, gmin, 1)
        assert hist[0, 1:16].tolist() == E.GROUP_SIZES[gmin] and (hist[:, 0] == 0).all()
        if c == 5: assert hist[0, 31] == 9                                         # a bucket of the VM merge's second block (16 buckets per block)
        cancel = dbl = ident = 0
        for (w, d), v in vals.items():
            ident += sum(q is None for q in v)
            if len(v) > 8 and G.sum(v[:8]) is None and all(q is not None for q in v[:8]): cancel += 1
            if len(v) >= 16 and v[8] == v[9] and v[8] is not None: dbl += 1
            for (X, Y, Z), q in zip(reps[(w, d)], v): assert Z != G.F.one and (Z == G.F.zero) == (q is None)
        assert cancel >= 8 and dbl >= 6 and ident >= 100, (cancel, dbl, ident)
        # the passes compose: leaders only, and the merge of every pass count gives the bucket's sum
        for (w, d), v in vals.items():
            if w or len(v) > 130: continue
            for passes in range(4):
                cur = list(v)
                for j in range(passes):
                    nxt = E.group_pass(G, cur, len(cur), gmin, 8 ** j)
                    assert all(nxt[k] == cur[k] for k in range(len(cur)) if k not in E.leaders(len(cur), gmin, 8 ** j))
                    cur = nxt
                assert E.merged(G, cur, gmin, passes) == G.sum(v)


# ---- segments, reduce, finish ---------------------------------------------------------------------------------------------------------------------------------------
def test_segment_cases_hold_all_occupancy_patterns():
    nwin, occ = E.segment_case("381", 0, 16)
    pats = E.occupancy_patterns(nwin, 16, occ)
    assert {p for _, p in pats} == set(range(16))
    assert sum(1 for later, p in pats if later and p & 1) >= 6                  # a non-identity bucket 0 of a segment j >= 1
    assert all((w, 0) not in occ for w in range(nwin))                            # bucket 0 of the window stays empty, as the merge leaves it
    nwin, occ = E.segment_case("381", 0, 8192)
    assert nwin == 1 and {d // 4 for (_, d) in occ} == {0, 1, 2, 3, 1023, 1024, 2047} and len(occ) == 27
    G = E.group("381", 0)
    q = E.pool("381", 0)[0]
    assert E.segment_sum(G, [q, None, None, q], 3) == G.mul(12 + 15, q) and E.segment_sum(G, [q, q, None, None], 0) == q


def test_reduce_and_finish_cases():
    G = E.group("377", 1)
    assert E.REDUCE_NIN == [1, 2, 3, 4, 5, 16, 17, 2048]
    for nin in E.REDUCE_NIN:
        rows = E.reduce_case("377", 1, nin)
        assert len(rows) == 2 and all(len(r) == nin for r in rows)
        if nin >= 16: assert any(q is None for r in rows for q in r)
        if nin <= 17: assert len(E.reduce_model(G, rows[0])) == -(-nin // 4) and G.sum(E.reduce_model(G, rows[0])) == G.sum(rows[0])
    for c, nwin in E.FINISH_SHAPES:
        assert nwin <= 64 and nwin * c <= 260
        for kind in E.FINISH_KINDS:
            ws = E.finish_case("377", 1, c, nwin, kind)
            assert len(ws) == nwin
            if kind == "random": assert nwin == 1 or ws[-1] is not None
            if kind == "top_identity": assert ws[-1] is None
            if kind == "all_identity": assert all(q is None for q in ws)
            if kind == "cancel" and nwin > 1:
                assert ws[0] is not None and ws[1] is not None and E.horner(G, c, ws) is None
    q = E.pool("377", 1)[0]
    assert E.horner(G, 4, [q, q, None, q]) == G.mul(1 + 16 + 4096, q)


# ---- slot sums --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
def test_slot_cases_hold_the_named_slots(tag, g2):
    G = E.group(tag, g2)
    for split in (1, G.split):
        for ch in E.SLOT_CH:
            case = E.slot_case(tag, g2, split, ch)
            nreal, n, named, slots = case["nreal"], case["n"], case["named"], case["slots"]
            assert n == split * nreal and case["bases"][6] is None and sum(b is None for b in case["bases"]) == 1
            assert all(G.on_curve(b) for b in case["bases"])
            # the slots are exactly the layout's: every bucket's run cut into ceil(cnt / ch) pieces, numbered through the window
            for w in range(2):
                offs, so, ns, total = E.layout(case["hist"][w], ch)
                assert sorted(s for (ww, s) in slots if ww == w) == list(range(total))
                for d in range(16):
                    run = case["sorted"][w, offs[d]:offs[d] + int(case["hist"][w, d])].tolist()
                    assert [slots[(w, so[d] + k)] for k in range(ns[d])] == E.slot_terms(run, ch)
            exc = {name for name, ws in named.items() if E.slot_is_exceptional(tag, g2, case, slots[ws])}
            want = {"one_term", "exactly_ch", "ch_plus_1", "id_first", "id_middle", "id_last", "id_only", "id_only_2", "P_P", "P_negP", "P_negP_Q_R", "P_Q_PplusQ", "P_Q_negPplusQ"}
            if split > 1: want |= {"base_and_images", "image_doubling", "image_doubling_rev"}
            if case["x0"] is not None: want |= {"x0_first", "x0_alone", "x0_last"}
            assert set(named) == want and ((case["x0"] is not None) == (split == 1 and not g2))
            assert len(slots[named["exactly_ch"]]) == ch
            w, s = named["ch_plus_1"]
            assert len(slots[(w, s)]) == ch and len(slots[(w, s + 1)]) == 1        # a bucket of ch + 1 terms: its second slot has one
            if ch >= 4:
                assert exc == {"P_P", "P_negP", "P_negP_Q_R", "P_Q_PplusQ", "P_Q_negPplusQ"} | ({"image_doubling", "image_doubling_rev"} if split > 1 else set()), exc
                assert E.slot_value(tag, g2, case, slots[named["P_negP"]]) is None and E.slot_value(tag, g2, case, slots[named["P_Q_negPplusQ"]]) is None
                assert E.slot_value(tag, g2, case, slots[named["id_only_2"]]) is None
                assert E.slot_value(tag, g2, case, slots[named["P_Q_PplusQ"]]) == G.mul(2, case["bases"][4])
                if split > 1:
                    t = slots[named["image_doubling"]]
                    assert t == [8, nreal + 1] and case["bases"][8] == E.term_point(tag, g2, case["bases"], nreal, nreal + 1) and case["bases"][8] != case["bases"][1]
                    assert len(slots[named["base_and_images"]]) == split and "base_and_images" not in exc
            else:
                assert not exc and all(len(t) == 1 for t in slots.values())          # ch = 1: every slot is one term, nothing is exceptional


@pytest.mark.parametrize("tag,g2", GROUPS, ids=IDS)
def test_forced_flag_case(tag, g2):
    G = E.group(tag, g2)
    for split in (1, G.split):
        fc = E.forced_case(tag, g2, split)
        assert fc["max_slots"] == 567 and 2 * fc["max_slots"] == 1134 > 1024 and fc["n"] == 1100 == split * fc["nreal"]
        spw = fc["spw"].tolist()
        assert all(s <= fc["max_slots"] for s in spw) and spw[0] > 17 and spw[1] > 1024 - 567 + 1
        last = fc["max_slots"] + spw[1] - 1
        for f in E.FORCED_FLAT + [last]:
            w, s = divmod(f, fc["max_slots"])
            assert (w, s) in fc["slots"] and 1 <= len(fc["slots"][(w, s)]) <= 2
        assert (1, spw[1]) not in fc["slots"] and last > 1024
