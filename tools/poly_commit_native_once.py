#!/usr/bin/env python3
"""One native univariate polynomial commitment at a given degree -- setup, a warm-up commit and open, then `--reps` timed commits and opens -- for
profiling (`rocprofv3 --kernel-trace --stats -- python tools/poly_commit_native_once.py`) and as the shortest end-to-end example of
ripp_amd/poly_commit/native.py.  The evaluation the library returns is checked against Horner, the proof by the native verifier.  The last line is
one SHA-256 over every output (commitment, y_polynomial_comms, proof members, value), group elements normalised first: equal between two builds of
the library (RIPP_HIP_LIB selects another one) exactly when they compute the same values.

  python tools/poly_commit_native_once.py [--degree 1048575] [--reps 1]"""
import argparse, hashlib, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=(1 << 20) - 1); ap.add_argument("--reps", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import ripp_amd as R, ripp_amd.poly_commit as P
    from ripp_amd.poly_commit import native as N
    R.init(0)
    U = N.UnivariatePolynomialCommitment
    t = time.perf_counter(); srs = U.setup(P.frs([123456789])[0], P.frs([987654321])[0], args.degree); t_setup = time.perf_counter() - t
    c = R.synth_fr(29, args.degree + 1); z = P.frs([0x1234567890ABCDEF1234567890ABCDEF])[0]
    com, coms = U.commit(srs, c); proof, val = U.open(srs, c, coms, z)                              # warm-up: scratch allocation, code objects
    tc, to = [], []
    for _ in range(args.reps):
        t = time.perf_counter(); com, coms = U.commit(srs, c); tc.append(time.perf_counter() - t)
        t = time.perf_counter(); proof, val = U.open(srs, c, coms, z); to.append(time.perf_counter() - t)
    rinv = pow(1 << 256, -1, P.R_MOD); raw = c.tobytes(); acc = 0; zi = 0x1234567890ABCDEF1234567890ABCDEF % P.R_MOD
    for i in range(args.degree, -1, -1):
        acc = (acc * zi + int.from_bytes(raw[32 * i:32 * i + 32], "little") * rinv) % P.R_MOD
    assert np.array_equal(val, P.frs([acc])[0]), "evaluation differs from Horner"
    assert U.verify(srs.verifier_key(), args.degree, com, z, val, proof)
    print(f"degree {args.degree} (x_degree, y_degree) = {srs.degrees()}: setup {t_setup * 1e3:.1f} ms, commit {min(tc) * 1e3:.2f} ms, open {min(to) * 1e3:.2f} ms (min of {args.reps}; medians {statistics.median(tc) * 1e3:.3f} / {statistics.median(to) * 1e3:.3f} ms); "
          f"evaluation = Horner, proof accepted; device bytes {R.device_bytes()}")
    ip = proof["ip_proof"]
    g1 = np.concatenate([np.asarray(coms).reshape(-1, 18), ip["com_g1"], ip["base_a"][None], proof["y_eval_comm"][None], proof["kzg_proof"][None]])
    g2 = np.stack([ip["final_ck_a"], ip["opening_a"]])
    h = hashlib.sha256()
    for part in (np.asarray(com), R.normalize_batch_g1(g1), R.normalize_batch_g2(g2), ip["com_gt"], ip["tr"], ip["base_b"], ip["kzg_c"], np.asarray(val)):
        h.update(np.ascontiguousarray(part, dtype=np.uint64).tobytes())
    print(f"outputs sha256 {h.hexdigest()} ({len(g1)} G1, {len(g2)} G2 points normalised)")
    srs.close()


if __name__ == "__main__":
    main()
