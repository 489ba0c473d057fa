#!/usr/bin/env python3
"""A/B of the GIPA prover for multiexponentiation products with a committed scalar vector (gipa.rs:499-530, benches/benches/gipa.rs case 2), three forms
alternating in one process per size n = 2^4 (the reference bench's LEN), 2^8, 2^10, 2^12, 2^14, 2^16:

    (a) generic   ripp_amd.gipa.GIPA(MultiexpIPG1, AFGHOCommitmentG1, PedersenCommitmentG1, IdentityCommitment(G1), resident=True).prove_with_aux:
                  the host loop of trait-level calls -- the baseline
    (b) native, four MSMs   ripp_gipa_mexp_prove with RIPP_GIPA_MEXP_BATCH_MIN at "never": every round's four G1 MSMs as single MSMs on two side streams
    (c) native, one pass    ripp_gipa_mexp_prove with RIPP_GIPA_MEXP_BATCH_MIN=2: every round's four G1 MSMs as one four-row pass of the batched pipeline

Wall time of the whole call, host slices in, proof out; `reps` timed proofs per form after a warm-up of two of each; median, minimum, maximum.  The header of
the output applies the two rules that decide the default of Engine::GIPA_MEXP_BATCH_MIN and whether the native prover may stand in for the generic one.

    python tools/gipa_mexp_ab.py [reps] > profiles/gipa_mexp_ab.txt
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENV = "RIPP_GIPA_MEXP_BATCH_MIN"
SIZES = [1 << 4, 1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16]
NEVER = str(1 << 40)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    sizes = [int(s) for s in os.environ["GIPA_MEXP_AB_SIZES"].split(",")] if os.environ.get("GIPA_MEXP_AB_SIZES") else SIZES
    import ripp_amd as R
    import ripp_amd.gipa as G
    from ripp_amd import api
    R.init(0)
    one = api._fp_one()
    gipa = G.GIPA(G.MultiexpIPG1, G.AFGHOCommitmentG1, G.PedersenCommitmentG1, G.IdentityCommitment(G.G1), resident=True)
    rows = []
    for n in sizes:
        a, m_b, ck_a, ck_b = R.synth_g1(1000, n), R.synth_fr(5, n), R.synth_g2(2000, n), R.synth_g1(10_000_000, n)
        m_a = np.zeros((n, 18), dtype=np.uint64); m_a[:, :12] = a; m_a[:, 12:18] = one
        ka = np.zeros((n, 36), dtype=np.uint64); ka[:, :24] = ck_a; ka[:, 24:30] = one             # the trait-level path takes projective keys
        kb = np.zeros((n, 18), dtype=np.uint64); kb[:, :12] = ck_b; kb[:, 12:18] = one

        def generic():
            return np.stack(gipa.prove_with_aux((m_a, m_b), (ka, kb, [None]))[1]["r_transcript"]).tobytes()

        def native(bound):
            os.environ[ENV] = bound
            try:
                return R.GIPA_MEXP.prove_with_aux(m_a, m_b, ck_a, ck_b)[1]["r_transcript"].tobytes()
            finally:
                del os.environ[ENV]

        forms = {"a": generic, "b": lambda: native(NEVER), "c": lambda: native("2")}
        ms = {k: [] for k in forms}; tr = {}
        for it in range(reps + 2):
            for k, fn in forms.items():
                t0 = time.perf_counter(); tr[k] = fn(); dt = (time.perf_counter() - t0) * 1e3
                if it >= 2: ms[k].append(dt)
        assert tr["b"] == tr["c"], f"n = {n}: the two native forms disagree"
        assert tr["a"] == tr["b"], f"n = {n}: the native prover and the generic path disagree"
        rows.append((n, {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}))

    # rule 1: the default bound is the smallest measured length from which (c)'s median is below (b)'s minimum there and at every longer measured length
    bound = None
    for i in range(len(rows) - 1, -1, -1):
        if rows[i][1]["c"][0] < rows[i][1]["b"][1]: bound = rows[i][0]
        else: break
    # rule 2: the native prover in that configuration is not slower than (a) at any measured size by more than (a)'s own min-max spread
    slower = []
    for n, r in rows:
        d = r["c"] if bound is not None and n >= bound else r["b"]
        if d[0] > r["a"][0] + (r["a"][2] - r["a"][1]): slower.append(n)
    print(f"# GIPA prover, multiexponentiation product with a committed scalar vector: wall ms per proof, {reps} timed proofs per form and size after 2 warm-up proofs,")
    print("# the three forms alternating in one process.  (a) generic host loop (ripp_amd/gipa.py, resident vectors), (b) ripp_gipa_mexp_prove with four single MSMs")
    print("# per round, (c) ripp_gipa_mexp_prove with the four MSMs of a round as one four-row pass of the batched pipeline.  (b) and (c) gave identical transcripts,")
    print("# equal to (a)'s, at every size.")
    if bound is None:
        print("# Rule 1 (default of GIPA_MEXP_BATCH_MIN): there is NO measured length from which (c)'s median stays below (b)'s minimum up to the longest size,")
        print("#   so the default stays \"never\": every round runs four single MSMs unless RIPP_GIPA_MEXP_BATCH_MIN says otherwise.")
    else:
        print(f"# Rule 1 (default of GIPA_MEXP_BATCH_MIN): (c)'s median is below (b)'s minimum at n = {bound} and at every longer measured size, and at no shorter")
        print(f"#   run of sizes, so the default is {bound}.")
    if slower:
        print(f"# Rule 2 (native default against the generic path): the native prover's median EXCEEDS (a)'s median by more than (a)'s min-max spread at n = {slower}.")
    else:
        print("# Rule 2 (native default against the generic path): at no measured size is the native prover's median above (a)'s median by more than (a)'s own")
        print("#   min-max spread.")
    print(f"# {'n':>6}  {'(a) med':>9} {'min':>9} {'max':>9}  {'(b) med':>9} {'min':>9} {'max':>9}  {'(c) med':>9} {'min':>9} {'max':>9}  {'b / a':>6} {'c / a':>6} {'c / b':>6}")
    for n, r in rows:
        a, b, c = r["a"], r["b"], r["c"]
        print(f"  {n:>6}  {a[0]:>9.3f} {a[1]:>9.3f} {a[2]:>9.3f}  {b[0]:>9.3f} {b[1]:>9.3f} {b[2]:>9.3f}  {c[0]:>9.3f} {c[1]:>9.3f} {c[2]:>9.3f}  {b[0] / a[0]:>6.2f} {c[0] / a[0]:>6.2f} {c[0] / b[0]:>6.2f}")


if __name__ == "__main__":
    main()
