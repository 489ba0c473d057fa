#!/usr/bin/env python3
"""A/B of the TIPA prover for scalar products (tipa/mod.rs:499-526), two forms alternating in one process per size n = 2^4 (the reference bench's LEN),
2^8, 2^10, 2^12, 2^14, 2^16:

    (b) two MSMs   ripp_tipa_scalar_prove with RIPP_TIPA_SCALAR_CROSS_MIN at "never": every round's two G2 and two G1 commitments as single MSMs on two side streams
    (c) crossed    ripp_tipa_scalar_prove with RIPP_TIPA_SCALAR_CROSS_MIN=2: every round's two G2 commitments as ONE crossed pass of the batched MSM pipeline in
                   its G2 form (tipa_scalar.hpp), then its two G1 commitments as one crossed pass of the G1 form

Wall time of the whole call, host slices in, proof out; `reps` timed proofs per form after a warm-up of two of each; median, minimum, maximum.  The tool
asserts that both forms give identical transcripts at every size.  The header of the output applies the rule that decides the default of
Engine::TIPA_SCALAR_CROSS_MIN.  Below the table: whole-call times of ripp_tipa_mexp_prove (default configuration) at n = 16 and 2^16 from the same process;
there is no earlier path of either prover to compare with.

    python tools/tipa_scalar_ab.py [reps] > profiles/tipa_scalar_ab.txt
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENV = "RIPP_TIPA_SCALAR_CROSS_MIN"
SIZES = [1 << 4, 1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16]
MEXP_SIZES = [1 << 4, 1 << 16]
NEVER = str(1 << 40)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    sizes = [int(s) for s in os.environ["TIPA_SCALAR_AB_SIZES"].split(",")] if os.environ.get("TIPA_SCALAR_AB_SIZES") else SIZES
    import ripp_amd as R
    from ripp_amd import api
    R.init(0)
    alpha, beta = R.synth_fr(91, 1)[0], R.synth_fr(92, 1)[0]
    rows, mexp_rows = [], []
    for n in sorted(set(sizes) | set(MEXP_SIZES)):
        srs = R.SRS.from_trapdoors(alpha, beta, n)
        ck_a, ck_b = srs.get_commitment_keys()
        ck_a, ck_b = R.normalize_batch_g2(ck_a), R.normalize_batch_g1(ck_b)                        # the C ABI takes affine keys: normalised once, outside the timing
        m_a, m_b = R.synth_fr(5, n), R.synth_fr(6, n)

        def scalar(bound):
            os.environ[ENV] = bound
            try:
                return R.TIPA_SCALAR.prove(srs, (m_a, m_b), (ck_a, ck_b))
            finally:
                del os.environ[ENV]

        if n in sizes:
            forms = {"b": lambda: scalar(NEVER), "c": lambda: scalar("2")}
            ms = {k: [] for k in forms}; out = {}
            for it in range(reps + 2):
                for k, fn in forms.items():
                    t0 = time.perf_counter(); out[k] = fn(); dt = (time.perf_counter() - t0) * 1e3
                    if it >= 2: ms[k].append(dt)
            for key in ("tr", "com_fr", "kzg_c", "base_a", "base_b"):
                assert out["b"][key].tobytes() == out["c"][key].tobytes(), f"n = {n}: the two forms disagree in {key}"
            rows.append((n, {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}))
        if n in MEXP_SIZES:
            one = api._fp_one()
            pts = np.zeros((n, 18), dtype=np.uint64); pts[:, :12] = R.synth_g1(1000, n); pts[:, 12:18] = one
            t = []
            for it in range(reps + 2):
                t0 = time.perf_counter(); R.TIPA_MEXP.prove(srs, (pts, m_b), (ck_a, ck_b)); dt = (time.perf_counter() - t0) * 1e3
                if it >= 2: t.append(dt)
            mexp_rows.append((n, statistics.median(t), min(t), max(t)))
        srs.close()

    # the rule: the default bound is the shortest measured n such that (c)'s median is below (b)'s minimum at that n and at every longer measured n
    bound = None
    for i in range(len(rows) - 1, -1, -1):
        if rows[i][1]["c"][0] < rows[i][1]["b"][1]: bound = rows[i][0]
        else: break
    print(f"# TIPA prover, scalar product (Pedersen keys in G2 and G1): wall ms per proof, {reps} timed proofs per form and size after 2 warm-up proofs, the two forms")
    print("# alternating in one process.  (b) ripp_tipa_scalar_prove with two single MSMs per group and round, (c) ripp_tipa_scalar_prove with the two G2")
    print("# commitments of a round as one crossed pass of the batched pipeline's G2 form and the two G1 commitments as one crossed pass of its G1 form.")
    print("# (b) and (c) gave identical transcripts, inner products, bases and KZG challenges at every size.")
    if bound is None:
        print("# Rule (default of TIPA_SCALAR_CROSS_MIN): there is NO measured length from which (c)'s median stays below (b)'s minimum up to the longest size,")
        print("#   so the default stays \"never\": every round runs two single MSMs per group unless RIPP_TIPA_SCALAR_CROSS_MIN says otherwise.")
    else:
        print(f"# Rule (default of TIPA_SCALAR_CROSS_MIN): (c)'s median is below (b)'s minimum at n = {bound} and at every longer measured size, and at no shorter")
        print(f"#   run of sizes, so the default is {bound}.")
    print(f"# {'n':>6}  {'(b) med':>9} {'min':>9} {'max':>9}  {'(c) med':>9} {'min':>9} {'max':>9}  {'c / b':>6}")
    for n, r in rows:
        b, c = r["b"], r["c"]
        print(f"  {n:>6}  {b[0]:>9.3f} {b[1]:>9.3f} {b[2]:>9.3f}  {c[0]:>9.3f} {c[1]:>9.3f} {c[2]:>9.3f}  {c[0] / b[0]:>6.2f}")
    print("#")
    print("# Whole-call times of the two new provers (no baseline: no earlier path exists).  ripp_tipa_scalar_prove: rows n = 16 and n = 65536 above, form (b) being the")
    print(f"# default unless the rule moved it.  ripp_tipa_mexp_prove, default configuration, {reps} timed proofs after 2 warm-up proofs in the same process:")
    print(f"# {'n':>6}  {'med':>9} {'min':>9} {'max':>9}")
    for n, med, lo, hi in mexp_rows:
        print(f"  {n:>6}  {med:>9.3f} {lo:>9.3f} {hi:>9.3f}")


if __name__ == "__main__":
    main()
