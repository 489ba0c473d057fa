#!/usr/bin/env python3
"""Counterpart of the reference's `benches/benches/poly_commit.rs` (its measurement harness for the polynomial-commitment
applications): for degree = 4^(i+1) - 1, i < num_data_points, time setup / commit / open / verify of the three schemes and print the
reference's CSV columns (poly_commit.rs:43-47: trial, scheme, function, degree, time[ms]) plus a backend column.

  python tools/poly_commit_bench.py <num_trials> <num_data_points> [--cpu-max DEGREE] [--native]

The device rows call ripp_amd.poly_commit (libripp_hip.so); with --cpu-max the oracle-backed restatement (tests/model/poly_commit_oracle.py)
is timed beside them up to that degree and every commitment / verdict is cross-checked.  Times include this module's host-side integer <->
Montgomery conversions of the coefficients (a Rust host hands field elements over as they are).

--native adds the rows of the library's own entry points (ripp_kzg_* / ripp_pc_* / ripp_tpc_*: ripp_amd/poly_commit/native.py) with backend `mi355x-hip-native`, on the same
polynomials and points, next to the rows above.  Those calls take Montgomery limbs, so their times hold no conversion -- what a Rust or C caller sees.  Every native
commitment, proof and evaluation is cross-checked against the Python path's, and each verifier is run on the other side's proof."""
import argparse, csv, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "model"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("num_trials", type=int); ap.add_argument("num_data_points", type=int)
    ap.add_argument("--cpu-max", type=int, default=0, help="largest degree the CPU oracle rows are produced for (0 = none)")
    ap.add_argument("--native", action="store_true", help="also time the native entry points (backend mi355x-hip-native) and cross-check them against the Python path")
    args = ap.parse_args()
    import numpy as np
    import ripp_amd as R, ripp_amd.poly_commit as P
    R.init(0)
    NAT = "mi355x-hip-native"
    if args.native:
        from ripp_amd.poly_commit import native as N
        from ripp_amd.gipa import fr_to_int
    def same_g1(a, b): return np.array_equal(R.normalize_batch_g1(np.asarray(a).reshape(-1, 18)), R.normalize_batch_g1(np.asarray(b).reshape(-1, 18)))
    w = csv.writer(sys.stdout); w.writerow(["trial", "scheme", "function", "degree", "time", "backend"])
    def row(trial, scheme, fn, degree, t, backend="mi355x-hip"): w.writerow([trial, scheme, fn, degree, "%.3f" % (t * 1e3), backend]); sys.stdout.flush()
    def timed(f):
        t = time.perf_counter(); r = f(); return time.perf_counter() - t, r
    for degree in (4 ** (i + 1) - 1 for i in range(args.num_data_points)):
        rng = random.Random(0)
        alpha, beta = rng.randrange(1, P.R_MOD), rng.randrange(1, P.R_MOD)
        cpu = degree <= args.cpu_max
        if cpu:
            import orclib as o, poly_commit_oracle as PC
        # ---- KZG (poly_commit.rs:51-129)
        t, (powers, v_srs) = timed(lambda: P.KZG.setup(alpha, beta, degree)); row(1, "kzg", "setup", degree, t)
        if args.native:
            fa, fb = P.frs([alpha])[0], P.frs([beta])[0]
            t, nsrs = timed(lambda: N.KZG.setup(fa, fb, degree)); row(1, "kzg", "setup", degree, t, NAT)
            nv = nsrs.verifier_key(); assert np.array_equal(nsrs.kzg_powers(), powers)
        for i in range(1, args.num_trials + 1):
            p = [rng.randrange(P.R_MOD) for _ in range(degree + 1)]; z = rng.randrange(P.R_MOD); ev = P.evaluate(p, z)
            t, com = timed(lambda: P.KZG.commit(powers, p)); row(i, "kzg", "commit", degree, t)
            t, proof = timed(lambda: P.KZG.open(powers, p, z)); row(i, "kzg", "open", degree, t)
            t, ok = timed(lambda: all(P.KZG.verify(v_srs, com, z, ev, proof) for _ in range(5))); assert ok; row(i, "kzg", "verify", degree, t / 5)
            if args.native:
                c, fz = P.frs(p), P.frs([z])[0]                       # (a native caller holds limbs: the conversion is not part of its call)
                t, ncom = timed(lambda: N.KZG.commit(nsrs, c)); row(i, "kzg", "commit", degree, t, NAT)
                t, (nproof, nval) = timed(lambda: N.KZG.open(nsrs, c, fz)); row(i, "kzg", "open", degree, t, NAT)
                t, ok = timed(lambda: all(N.KZG.verify(nv, ncom, fz, nval, nproof) for _ in range(5))); assert ok; row(i, "kzg", "verify", degree, t / 5, NAT)
                assert same_g1(ncom, com) and same_g1(nproof, proof) and fr_to_int(nval) == ev
                assert P.KZG.verify(nv, ncom, z, ev, nproof) and N.KZG.verify(v_srs, com, fz, nval, proof)
            if cpu:
                epowers, ev_srs = PC.kzg_setup(alpha, beta, degree)
                t, ecom = timed(lambda: PC.kzg_commit(epowers, p)); row(i, "kzg", "commit", degree, t, "cpu-oracle")
                t, eproof = timed(lambda: PC.kzg_open(epowers, p, z)); row(i, "kzg", "open", degree, t, "cpu-oracle")
                t, ok = timed(lambda: PC.kzg_verify(ev_srs, com, z, ev, proof)); assert ok; row(i, "kzg", "verify", degree, t, "cpu-oracle")
                assert np.array_equal(o.g1_to_affine(ecom), o.g1_to_affine(com)) and np.array_equal(o.g1_to_affine(eproof), o.g1_to_affine(proof))
        # ---- IPA: the pairing-based univariate scheme (poly_commit.rs:131-203)
        U = P.UnivariatePolynomialCommitment
        t, srs = timed(lambda: U.setup(alpha, beta, degree)); row(1, "ipa", "setup", degree, t)
        v = srs[0].get_verifier_key()
        for i in range(1, args.num_trials + 1):
            p = [rng.randrange(P.R_MOD) for _ in range(degree + 1)]; z = rng.randrange(P.R_MOD); ev = P.evaluate(p, z)
            t, (com, coms) = timed(lambda: U.commit(srs, p)); row(i, "ipa", "commit", degree, t)
            t, proof = timed(lambda: U.open(srs, p, coms, z)); row(i, "ipa", "open", degree, t)
            t, ok = timed(lambda: all(U.verify(v, degree, com, z, ev, proof) for _ in range(5))); assert ok; row(i, "ipa", "verify", degree, t / 5)
            if cpu:
                xd, yd = U.bivariate_degrees(degree); s = PC.bi_setup(alpha, beta, xd, yd); ys = PC.split(p, xd, yd); pt = (pow(z, yd + 1, P.R_MOD), z)
                t, (ecom, ecoms) = timed(lambda: PC.bi_commit(s, ys)); row(i, "ipa", "commit", degree, t, "cpu-oracle")
                t, eproof = timed(lambda: PC.bi_open(s, ys, ecoms, pt)); row(i, "ipa", "open", degree, t, "cpu-oracle")
                t, ok = timed(lambda: PC.bi_verify(s["v"], com, pt, ev, proof)); assert ok; row(i, "ipa", "verify", degree, t, "cpu-oracle")
                assert np.array_equal(ecom, com) and np.array_equal(eproof["ip_proof"]["tr"], proof["ip_proof"]["tr"])
        if args.native and degree >= 1:
            nsrs.close()
            t, nsrs = timed(lambda: N.UnivariatePolynomialCommitment.setup(fa, fb, degree)); row(1, "ipa", "setup", degree, t, NAT)
            nv = nsrs.verifier_key(); NU = N.UnivariatePolynomialCommitment
            for i in range(1, args.num_trials + 1):
                p = [rng.randrange(P.R_MOD) for _ in range(degree + 1)]; z = rng.randrange(P.R_MOD); ev = P.evaluate(p, z)
                c, fz = P.frs(p), P.frs([z])[0]
                t, (ncom, ncoms) = timed(lambda: NU.commit(nsrs, c)); row(i, "ipa", "commit", degree, t, NAT)
                t, (nproof, nval) = timed(lambda: NU.open(nsrs, c, ncoms, fz)); row(i, "ipa", "open", degree, t, NAT)
                t, ok = timed(lambda: all(NU.verify(nv, degree, ncom, fz, nval, nproof) for _ in range(5))); assert ok; row(i, "ipa", "verify", degree, t / 5, NAT)
                com, coms = U.commit(srs, p); proof = U.open(srs, p, coms, z)
                assert np.array_equal(ncom, com) and same_g1(ncoms, coms) and fr_to_int(nval) == ev
                assert np.array_equal(nproof["ip_proof"]["tr"], proof["ip_proof"]["tr"]) and same_g1(nproof["kzg_proof"], proof["kzg_proof"]) and same_g1(nproof["y_eval_comm"], proof["y_eval_comm"])
                assert U.verify(nv, degree, ncom, z, ev, nproof) and NU.verify(v, degree, com, fz, nval, proof)
            nsrs.close()
        srs[0].close()
        # ---- transparent IPA (poly_commit.rs:205-277)
        T = P.transparent.UnivariatePolynomialCommitment
        t, ck = timed(lambda: T.setup(700, 900, degree)); row(1, "transparent_ipa", "setup", degree, t)
        for i in range(1, args.num_trials + 1):
            p = [rng.randrange(P.R_MOD) for _ in range(degree + 1)]; z = rng.randrange(P.R_MOD); ev = P.evaluate(p, z)
            t, (com, coms) = timed(lambda: T.commit(ck, p)); row(i, "transparent_ipa", "commit", degree, t)
            t, proof = timed(lambda: T.open(ck, p, coms, z)); row(i, "transparent_ipa", "open", degree, t)
            t, ok = timed(lambda: T.verify(ck, com, z, ev, proof)); assert ok; row(i, "transparent_ipa", "verify", degree, t)
            if args.native:
                if i == 1:
                    NT = N.transparent.UnivariatePolynomialCommitment
                    t, nck = timed(lambda: NT.setup(700, 900, degree)); row(1, "transparent_ipa", "setup", degree, t, NAT)
                    k1, k2 = nck.keys(); assert np.array_equal(k1, ck[0][:, :12]) and np.array_equal(k2, ck[1][:, :24])
                c, fz = P.frs(p), P.frs([z])[0]
                t, (ncom, ncoms) = timed(lambda: NT.commit(nck, c)); row(i, "transparent_ipa", "commit", degree, t, NAT)
                t, (nproof, nval) = timed(lambda: NT.open(nck, c, ncoms, fz)); row(i, "transparent_ipa", "open", degree, t, NAT)
                t, ok = timed(lambda: NT.verify(nck, ncom, fz, nval, nproof)); assert ok; row(i, "transparent_ipa", "verify", degree, t, NAT)
                assert np.array_equal(ncom, com) and same_g1(ncoms, coms) and fr_to_int(nval) == ev and same_g1(nproof["y_eval_comm"], proof["y_eval_comm"])
                for tier, left_g1 in (("second_tier_ip_proof", False), ("first_tier_ip_proof", True)):       # member for member
                    a, b = nproof[tier], proof[tier]; assert len(a["r_commitment_steps"]) == len(b["r_commitment_steps"])
                    for sa, sb in zip(a["r_commitment_steps"], b["r_commitment_steps"]):
                        for k in range(2):
                            assert same_g1(sa[k][0], sb[k][0]) if left_g1 else np.array_equal(sa[k][0], sb[k][0])
                            assert np.array_equal(sa[k][2][0], sb[k][2][0]) if left_g1 else same_g1(sa[k][2][0], sb[k][2][0])
                    assert (np.array_equal(a["r_base"][0], b["r_base"][0]) if left_g1 else same_g1(a["r_base"][0], b["r_base"][0])) and np.array_equal(a["r_base"][1], b["r_base"][1])
                assert T.verify(ck, ncom, z, ev, nproof) and NT.verify(nck, com, fz, nval, proof)         # each verifier on the other side's proof
        if args.native:
            nck.close()


if __name__ == "__main__":
    main()
