#!/usr/bin/env python3
"""A/B of the batched shared-base G1 MSM (ripp_msm_g1_batch_a, msm_batch.hpp) against the loop of single MSMs it replaces (rows calls of
ripp_msm_g1_a over the same bases), both from host slices: the bases and the scalars are uploaded by both sides.

  python tools/msm_batch_ab.py [--shapes 16x4096,64x16384,256x65536] [--reps 7]

The two forms alternate inside one process on one device (two warm-up passes each, then `reps` timed pairs); the points are compared after
normalisation.  Prints one line per shape: median and minimum of both, and the ratio of the medians."""
import argparse, ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x4096,64x16384,256x65536"); ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import ripp_amd as R
    from ripp_amd._lib import lib
    from ripp_amd.poly_commit import native as N
    R.init(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def loop(bases, sc):
        out = np.zeros((len(sc), 18), dtype=np.uint64)
        for r in range(len(sc)):
            assert lib().ripp_msm_g1_a(p(bases), p(sc[r]), ctypes.c_size_t(sc.shape[1]), p(out[r])) == 0
        return out

    print("# batched = ripp_msm_g1_batch_a, loop = rows x ripp_msm_g1_a; host slices on both sides; times in ms")
    print("rows,cols,batched_median,batched_min,loop_median,loop_min,ratio_loop_over_batched,chunks")
    for shape in args.shapes.split(","):
        rows, cols = (int(v) for v in shape.split("x"))
        bases = R.synth_g1(1000, cols); sc = np.ascontiguousarray(R.synth_fr(rows, rows * cols).reshape(rows, cols, 4))
        for _ in range(2):
            a = N.msm_g1_batch(bases, sc); b = loop(bases, sc)
        assert np.array_equal(R.normalize_batch_g1(a), R.normalize_batch_g1(b)), "batched and looped MSMs differ"
        tb, tl = [], []
        for _ in range(args.reps):
            t = time.perf_counter(); N.msm_g1_batch(bases, sc); tb.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); loop(bases, sc); tl.append((time.perf_counter() - t) * 1e3)
        med = lambda v: sorted(v)[len(v) // 2]
        print(f"{rows},{cols},{med(tb):.3f},{min(tb):.3f},{med(tl):.3f},{min(tl):.3f},{med(tl) / med(tb):.2f},{N.msm_batch_chunks()}"); sys.stdout.flush()
        R.release_scratch()


if __name__ == "__main__":
    main()
