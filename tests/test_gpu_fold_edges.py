"""GPU (-m gpu): every form of the resident fold (ripp_vec_fold -> fold_dev, the dispatch of every GIPA / TIPA / TPC prover) against the CPU oracle's plain
double-and-add fold, bit for bit, at the scalars where the recoders cut (tests/fold_edge_scalars.py) and with the degenerate rows a fold can meet:
hi, lo or both at infinity, lo == hi, lo == -hi, and per scalar lo == s hi (the fold's last addition is a doubling) and lo == -(s hi) (the result is the
point at infinity).  half = 70 is no multiple of 16 or 64: two ragged 64-lane blocks, a ragged VM block of 16 elements, a partly filled 256-lane block;
one more call per form at half = 261 crosses a 256-lane block.  The forms are selected with the per-call environment overrides and every case first
reads ripp_config_get and checks that the call about to run takes the form it names.  All points are in G1 / G2 proper (include/ripp_hip.h)."""
import os
import time

import numpy as np
import pytest

import fold_edge_scalars as FE

pytestmark = pytest.mark.gpu
HALF, HALF_WIDE = 70, 261
ROWS = "0: hi = inf, 1: lo = inf, 2: both inf, 3: lo == hi, 4: lo == -hi, half - 2: lo == s hi, half - 1: lo == -(s hi)"

# case -> (group, environment, the members of ripp_config the environment sets, the form fold_dev takes)
CASES = {
    "g1_vm": ("G1", {}, {}, "vm"),
    "g1_fq": ("G1", {"RIPP_VM_FOLD_MAX": "0"}, {"vm_fold_max": 0}, "fq"),
    "g1_32bit": ("G1", {"RIPP_VM_FOLD_MAX": "0", "RIPP_NO_FQ": "1"}, {"vm_fold_max": 0, "no_fq": 1}, "32bit"),
    "g1_plain": ("G1", {"RIPP_NO_ENDO": "1"}, {"no_endo": 1}, "plain"),
    "g2_plain": ("G2", {"RIPP_NO_ENDO": "1"}, {"no_endo": 1}, "plain"),
    "g2_vm": ("G2", {}, {}, "vm"),
    "g2_split_fq": ("G2", {"RIPP_VM_FOLD_MAX": "0"}, {"vm_fold_max": 0}, "split_fq"),
    "g2_split_32bit": ("G2", {"RIPP_VM_FOLD_MAX": "0", "RIPP_NO_FQ": "1"}, {"vm_fold_max": 0, "no_fq": 1}, "split_32bit"),
    "g2_one_lane": ("G2", {"RIPP_VM_FOLD_MAX": "0", "RIPP_GLS_SPLIT_MAX": "0"}, {"vm_fold_max": 0, "gls_split_max": 0}, "one_lane"),
    "g2_table": ("G2", {"RIPP_VM_FOLD_MAX": "0", "RIPP_GLS_SPLIT_MAX": "0", "RIPP_FOLD_TAB_MIN": "1"}, {"vm_fold_max": 0, "gls_split_max": 0, "fold_tab_min": 1}, "table_32bit"),
    "g2_table_fq": ("G2", {"RIPP_VM_FOLD_MAX": "0", "RIPP_GLS_SPLIT_MAX": "0", "RIPP_FOLD_TAB_MIN": "1", "RIPP_FQ_MIN": "1"},
                    {"vm_fold_max": 0, "gls_split_max": 0, "fold_tab_min": 1, "fq_min": 1}, "table_fq"),
    # the same tables built by the 32-bit k_odd_multiples instead of the carry-free one
    "g2_table_32bit_build": ("G2", {"RIPP_VM_FOLD_MAX": "0", "RIPP_GLS_SPLIT_MAX": "0", "RIPP_FOLD_TAB_MIN": "1", "RIPP_NO_FQ": "1"},
                             {"vm_fold_max": 0, "gls_split_max": 0, "fold_tab_min": 1, "no_fq": 1}, "table_32bit_all"),
}


def form_of(c, group, half):
    """the branch ripp_vec_fold / fold_dev (vec_api.inc, tipa_api.inc) takes for `half` outputs under the configuration c"""
    if c.no_endo: return "plain"
    if half <= c.vm_fold_max and not c.no_vm: return "vm"
    if group == "G1": return "32bit" if c.no_fq else "fq"
    if half <= c.gls_split_max: return "split_32bit" if c.no_fq else "split_fq"
    if half >= c.fold_tab_min and not c.no_fold_tables:
        if c.no_fq: return "table_32bit_all"
        return "table_fq" if half >= c.fq_min else "table_32bit"
    return "one_lane"


def _neg(o, pts):
    """-P for affine rows in Montgomery limbs (y -> p - y; the point at infinity (0, 0) stays)"""
    out = pts.copy(); w = pts.shape[1] // 2
    for row in out:
        for k in range(w, 2 * w, 6):
            m = sum(int(x) << (64 * i) for i, x in enumerate(row[k:k + 6]))
            m = (o.P - m) % o.P
            row[k:k + 6] = [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]
    return out


def _vectors(o, group, half, scalars):
    """hi, per scalar (lo, the oracle's fold): the special rows of the module docstring in a vector of subgroup points"""
    gen, fold = (o.gen_g1, o.fold_g1_a) if group == "G1" else (o.gen_g2, o.fold_g2_a)
    hi, lo = gen(0x70000 + half, half), gen(0x90000 + half, half)
    assert half >= 16 and hi.any(axis=1).all() and lo.any(axis=1).all()
    hi[0] = 0; lo[1] = 0; hi[2] = 0; lo[2] = 0; lo[3] = hi[3]; lo[4] = _neg(o, hi[4:5])[0]
    per = []
    for s in scalars:
        sm = o.fr_array([s])[0]
        l = lo.copy()
        sh = fold(hi[half - 2:], np.zeros_like(hi[half - 2:]), sm)             # s hi for the last two rows
        l[half - 2] = sh[0]; l[half - 1] = _neg(o, sh[1:2])[0]
        exp = fold(hi, l, sm)
        # the oracle itself meets the degenerate rows as intended (checked here once, so that the comparison below is with the right thing)
        assert not exp[2].any() and np.array_equal(exp[1], fold(hi[1:2], np.zeros_like(hi[1:2]), sm)[0]) and np.array_equal(exp[0], l[0]) and not exp[half - 1].any(), hex(s)
        per.append((s, sm, l, exp))
    return hi, per


@pytest.fixture(scope="module", params=["381", "377"])
def curve(request, engine, orc):
    if request.param == "381":
        E, o = engine, orc
    else:
        import orclib377 as o
        import ripp_amd.bls12_377 as E
        o.lib(); E.init(0)
    r, _, _ = FE.params(request.param)
    assert r == o.R
    S = FE.scalars(request.param)
    wide = [r - 1, 0xFFFFFFFF_00000000_FFFFFFFF, S[-1]]                       # r - 1, a 128-bit one, a full-width one (the inverse that closes S)
    assert wide[1] in S and wide[1] < 1 << 128 <= wide[2]
    t0 = time.time()
    data = {(g, h): _vectors(o, g, h, sc) for g in ("G1", "G2") for h, sc in ((HALF, S), (HALF_WIDE, wide))}
    print("oracle folds, BLS12-%s: %.2f s" % (request.param, time.time() - t0))
    return request.param, E, data


def _first_diff(got, exp):
    return int(np.nonzero((got != exp).any(axis=1))[0][0])


@pytest.mark.parametrize("case", list(CASES))
def test_fold_form_matches_oracle_at_edge_scalars(curve, case):
    name, E, data = curve
    group, env, members, form = CASES[case]
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = E.config_get()
        for k, v in members.items():
            assert getattr(c, k) == v, "%s: ripp_config.%s is %d, the case sets %d" % (case, k, getattr(c, k), v)
        for half in (HALF, HALF_WIDE):
            assert form_of(c, group, half) == form, "%s would run the %s form at half = %d" % (case, form_of(c, group, half), half)
        for half in (HALF, HALF_WIDE):
            hi, per = data[(group, half)]
            vhi = E.Vec.upload(group, hi)
            assert np.array_equal(vhi.download(), hi)
            for s, sm, lo, exp in per:
                vlo = E.Vec.upload(group, lo)
                got = vhi.fold(vlo, sm).download()
                assert np.array_equal(got, exp), "BLS12-%s %s half = %d: s = %s differs from the oracle first at row %d (%s)" % (name, case, half, hex(s), _first_diff(got, exp), ROWS)
                vlo.close()
            vhi.close()
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
