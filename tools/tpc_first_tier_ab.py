#!/usr/bin/env python3
"""A/B of the two forms of a first-tier round's Pedersen commitments (ripp_amd/csrc/tpc_api.inc, tpc.hpp): ONE crossed two-row pass of the batched MSM
pipeline against two single MSMs on two streams, per round length 4096 .. 2, both in one process.

The library reads RIPP_TPC_CROSS_MIN once per call, so the two forms alternate run by run on one engine: `reps` proofs of n = 4096 each (after a warm-up
of both), the per-round figures from ripp_tpc_round_ms -- launch of the round's commitments and inner products to their arrival on the host.  Medians.

    python tools/tpc_first_tier_ab.py [reps] > profiles/tpc_first_tier_ab.txt
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    import ripp_amd as R
    from ripp_amd.poly_commit import native
    R.init(0)
    T = native.transparent
    n = 4096
    m, b, ck = R.synth_fr(1, n), R.synth_fr(2, n), R.synth_g1(700, n)
    forms = {"crossed": "2", "two MSMs": str(1 << 40)}
    samples = {k: [] for k in forms}; totals = {k: [] for k in forms}
    proofs = {}
    for it in range(reps + 2):
        for name, bound in forms.items():
            os.environ["RIPP_TPC_CROSS_MIN"] = bound
            proof, tr = T.scalar_prove(m, b, ck)
            proofs[name] = tr.tobytes()
            if it >= 2:
                ms = T.round_ms(); samples[name].append(ms); totals[name].append(sum(ms))
    del os.environ["RIPP_TPC_CROSS_MIN"]
    assert proofs["crossed"] == proofs["two MSMs"], "the two forms disagree"
    rounds = len(samples["crossed"][0])
    print(f"# first-tier round, commitments + inner products (ms, median of {reps} proofs of n = {n}; the forms alternate in one process)")
    print(f"# {'key length':>10}  {'crossed':>9}  {'two MSMs':>9}  {'crossed / two':>13}")
    for r in range(rounds):
        c = statistics.median(s[r] for s in samples["crossed"]); t = statistics.median(s[r] for s in samples["two MSMs"])
        print(f"  {n >> r:>10}  {c:>9.3f}  {t:>9.3f}  {c / t:>13.2f}")
    c, t = statistics.median(totals["crossed"]), statistics.median(totals["two MSMs"])
    print(f"  {'all rounds':>10}  {c:>9.3f}  {t:>9.3f}  {c / t:>13.2f}")


if __name__ == "__main__":
    main()
