"""CPU: the host side of the Pippenger plan -- msm_tune_ok, msm_plan (ripp_amd/csrc/msm.hpp), msm_plan_batch (msm_batch.hpp) -- as a stand-alone program
(tests/host/msm_plan.cpp, built once with the ROCm clang++; it launches nothing and needs no device).

The tuning members ripp_config.msm_c / msm_ch / msm_gmin (RIPP_MSM_C / RIPP_MSM_CH / RIPP_MSM_GMIN) are public and go straight into the plan, and the kernels
are built for a range of them only: 64 windows (k_msm_finish[_vm] and the 64 entries of the window array), 8192 LDS counters of the sort, 16-bit digits.
msm_tune_ok is that range; the engine refuses a call outside it (tests/test_gpu_parity.py checks the refusal through the C ABI).  Here: every plan the
accepted corners can give stays inside what the kernels are built for, and the values named in the range's reasons are rejected."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CLANG = os.path.join(ROCM, "llvm", "bin", "clang++")

NREAL = [1, 2, 63, 64, 65, 1 << 10, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 26]
SPLITS = [1, 2, 4]
ROWS = [0, 1, 4, 1000]                       # 0: msm_plan
CORNERS = list(itertools.product([0, 4, 13], [0, 1, 65536], [0, 1, 65536]))          # (c, ch, gmin): every accepted corner, 0 = the plan's own choice
NBITS = {1: 255, 2: 128, 4: 64}
REJECTED = [(c, 0, 0) for c in (-3, 1, 3, 14, 17, 32)] + [(0, 2 ** 32 - 1, 0), (0, 0, 2 ** 32 - 1), (0, 65537, 0), (0, 0, 65537), (2, 4, 16), (-1, 0, 0)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("msm_plan") / "msm_plan")
    subprocess.check_call([CLANG, "-x", "hip", "--offload-arch=gfx950", "--rocm-path=" + ROCM, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "ripp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "msm_plan.cpp"), "-o", path, "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")])
    return path


def _run(exe, requests):
    text = "".join("%d %d %d %d %d %d\n" % r for r in requests)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(requests)
    return [tuple(int(x) for x in ln.split()) for ln in out]


def worst_slots(n, nb, ch):
    """the most slots one window can have: sum of ceil(cnt_d / ch) over the buckets 1 .. nb - 1 with sum cnt_d <= n.  A bucket's first term opens a slot and
    every further ch terms open one more, so the maximum puts one term into each of k = min(nb - 1, n) buckets and the other n - k anywhere."""
    k = min(nb - 1, n)
    return k + (n - k) // ch


def test_worst_slots_is_the_maximum_by_enumeration():
    for n, nb, ch in [(5, 4, 2), (6, 4, 1), (7, 3, 3), (4, 8, 2), (9, 4, 4)]:
        best = 0
        for cnt in itertools.product(range(n + 1), repeat=nb - 1):
            if sum(cnt) <= n: best = max(best, sum((c + ch - 1) // ch for c in cnt))
        assert best == worst_slots(n, nb, ch), (n, nb, ch)


def test_every_accepted_corner_gives_a_plan_the_kernels_are_built_for(exe):
    reqs = [(nreal, split, rows, c, ch, gmin) for nreal in NREAL for split in SPLITS for rows in ROWS for (c, ch, gmin) in CORNERS]
    seen_c, seen_nwin = set(), set()
    for req, res in zip(reqs, _run(exe, reqs)):
        nreal, split, rows, tc, tch, tgmin = req
        ok, c, nwin, nb, n, ch, seg, p_nreal, gmin, tile = res
        nbits = NBITS[split]
        assert ok == 1, req
        assert 4 <= c <= 13 and (tc == 0 or c == tc), (req, res)
        assert nb == 1 << c, (req, res)
        assert nwin * c >= nbits > (nwin - 1) * c, (req, res)
        assert nwin <= 64, (req, res)                                   # k_msm_finish_vm copies 64 windows, ms.win holds 64
        assert seg == 4 and nb % seg == 0, (req, res)                   # k_msm_vm_segments reads four buckets per segment
        assert ch >= 1 and (tch == 0 or ch == tch), (req, res)
        assert 1 <= gmin <= 65536 and (tgmin == 0 and gmin == 16 or gmin == tgmin), (req, res)
        assert n == split * nreal and p_nreal == nreal, (req, res)
        assert n // ch + min(nb, n) + 1 >= worst_slots(n, nb, ch), (req, res)       # max_slots of msm_launch / msm_batch_dev
        assert nb - 1 < 1 << 16, (req, res)                              # digits are uint16_t
        vw = nwin * max(rows, 1)                                         # virtual windows of the launch
        tiles = 1 if vw >= 480 else 480 // vw
        assert tile % 1024 == 0 and tile >= 1024 and tile * tiles >= n and (tile - 1024) * tiles < n, (req, res)
        seen_c.add(c); seen_nwin.add(nwin)
    assert {4, 13} <= seen_c and 64 in seen_nwin and 5 in seen_nwin, (seen_c, seen_nwin)         # c = 4 unsplit: 64 windows; c = 13 over 64 bits: 5


def test_the_plans_own_choices_without_tuning(exe):
    """the untuned plan: c within one of lg(n) - 6, ch a power of two in 4 .. 64, batch rows only lengthen the slots"""
    reqs = [(nreal, split, rows, 0, 0, 0) for nreal in NREAL for split in SPLITS for rows in ROWS]
    res = _run(exe, reqs)
    for req, r in zip(reqs, res):
        nreal, split, rows = req[:3]
        lg = (split * nreal).bit_length() - 1
        c0 = min(13, max(4, lg - 6))
        assert abs(r[1] - c0) <= 1 and r[5] in (4, 8, 16, 32, 64), (req, r)
        if rows:
            single = res[reqs.index((nreal, split, 0, 0, 0, 0))]
            assert r[1:5] == single[1:5] and r[5] >= single[5], (req, r, single)


def test_values_outside_the_range_are_rejected(exe):
    reqs = [(1 << 10, split, rows, c, ch, gmin) for (c, ch, gmin) in REJECTED for split in SPLITS for rows in (0, 4)]
    for req, res in zip(reqs, _run(exe, reqs)):
        assert res == (0,) * 10, (req, res)
    # ... and one member out of range is enough, whatever the others are
    reqs = [(64, 2, 0, 14, 4, 16), (64, 2, 0, 13, 65537, 16), (64, 2, 0, 13, 4, 65537), (64, 2, 0, 3, 1, 1)]
    assert all(r[0] == 0 for r in _run(exe, reqs))
    assert all(r[0] == 1 for r in _run(exe, [(64, 2, 0, 13, 65536, 65536), (64, 2, 0, 4, 1, 1)]))
