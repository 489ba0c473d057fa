#!/usr/bin/env python3
"""Timings of the bulk validation of untrusted points (include/ripp_hip.h, "validation of untrusted points"), per curve, at n = 2^14 and 2^20:

    ripp_validate_g1a / ripp_validate_g2a      n points of G1 / G2 proper from host slices: upload, one lane per point, flags back
    ripp_de_groth16_proofs                     n proof images (A, B, C), compressed and uncompressed: host parse on the library's workers + device check
    ripp_aggregate_proofs                      at n = 2^14, from the same run: the call the readers feed

Wall time of the whole call (every call ends in a device synchronise), host slices in, results out; `reps` timed calls after two warm-up calls, median /
minimum / maximum.  The compressed reader at 2^20 takes its square roots on the host and is timed ONCE (it runs for tens of seconds).  The split of a
reader's time: "device check" is the time of ripp_validate_g1a on the 2n parsed points A | C plus ripp_validate_g2a on the n points B -- the launches the
reader makes -- and "host parse" is the rest of the reader's median.  The proof images at 2^20 are the 2^14 distinct images of the smaller case, repeated.
No earlier path exists in the library to compare with; the host parse of chunk k + 1 is not overlapped with the device check of chunk k.

    python tools/validate_bench.py [reps] > profiles/validate_ab.txt
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [1 << 14, 1 << 20]
DISTINCT = 1 << 14


def timed(fn, reps, warm=2):
    for _ in range(warm): fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def fmt(t): return f"{t[0]:>11.3f} {t[1]:>11.3f} {t[2]:>11.3f}"


def device_name():
    """marketing name (where the box knows it), architecture and compute units of device 0: the HIP runtime's name, completed from rocminfo's first GPU agent"""
    import ctypes
    import re
    import subprocess
    name, arch, cus = "", "", ""
    try:
        buf = ctypes.create_string_buffer(256)
        if ctypes.CDLL("libamdhip64.so").hipDeviceGetName(buf, 256, 0) == 0: name = buf.value.decode().strip()
    except Exception:
        pass
    try:
        text = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
        agent = next(a for a in re.split(r"\*{3,}\s*\nAgent \d+", text) if re.search(r"Device Type:\s+GPU", a))
        arch = re.search(r"^\s*Name:\s+(gfx\w+)", agent, re.M).group(1)
        cus = re.search(r"Compute Unit:\s+(\d+)", agent).group(1)
        if not name: name = re.search(r"Marketing Name:[ \t]*(.*)", agent).group(1).strip()
    except Exception:
        pass
    return f"device 0: {name or 'no marketing name reported'}, {arch or 'architecture not reported'}, {cus or '?'} compute units"


def run(name, R, reps, sizes):
    R.init(0)
    print(f"# {name}")
    print(f"# {'call':<44} {'n':>8}  {'median ms':>11} {'min':>11} {'max':>11}  {'ns / point':>10}")
    a0, b0, c0 = R.synth_g1(1000, DISTINCT), R.synth_g2(2000, DISTINCT), R.synth_g1(3000, DISTINCT)
    images = {}
    for compress in (False, True):
        s1, s2 = (R.ser_g1_compressed, R.ser_g2_compressed) if compress else (R.ser_g1, R.ser_g2)
        images[compress] = b"".join(s1(a0[i]) + s2(b0[i]) + s1(c0[i]) for i in range(DISTINCT))
    for n in sizes:
        g1, g2 = R.synth_g1(1000, n), R.synth_g2(2000, n)
        for label, fn, pts in (("ripp_validate_g1a", R.validate_g1, g1), ("ripp_validate_g2a", R.validate_g2, g2)):
            assert fn(pts)[1] == 0
            t = timed(lambda: fn(pts), reps)
            print(f"  {label:<44} {n:>8}  {fmt(t)}  {t[0] * 1e6 / n:>10.1f}")
        del g1, g2
        rep = max(n // DISTINCT, 1)
        ac = np.concatenate([np.tile(a0, (rep, 1))[:n], np.tile(c0, (rep, 1))[:n]]); bb = np.tile(b0, (rep, 1))[:n]
        check = timed(lambda: (R.validate_g1(ac), R.validate_g2(bb)), reps)
        del ac
        for compress in (False, True):
            size = 192 if compress else 384
            data = np.frombuffer(images[compress][: min(n, DISTINCT) * size] * rep, dtype=np.uint8)
            once = compress and n > DISTINCT
            out = R.deserialize_groth16_proofs(data, compress=compress, n=n) if not once else None
            if out is not None: assert out[4] == 0 and np.array_equal(out[1], bb)
            t = timed(lambda: R.deserialize_groth16_proofs(data, compress=compress, n=n), 1 if once else reps, 0 if once else 1)
            kind = "compressed" if compress else "uncompressed"
            print(f"  {'ripp_de_groth16_proofs, ' + kind + (' (one call)' if once else ''):<44} {n:>8}  {fmt(t)}  {t[0] * 1e6 / (3 * n):>10.1f}")
            print(f"  {'    device check (A | C in G1, B in G2)':<44} {n:>8}  {fmt(check)}  {check[0] * 1e6 / (3 * n):>10.1f}")
            print(f"  {'    host parse (the rest of the median)':<44} {n:>8}  {max(t[0] - check[0], 0.0):>11.3f}")
            del data
        if n == DISTINCT:
            srs = R.SRS.from_trapdoors(R.synth_fr(11, 1)[0], R.synth_fr(12, 1)[0], n)
            t = timed(lambda: R.aggregate_proofs(srs, a0, b0, c0), reps)
            print(f"  {'ripp_aggregate_proofs':<44} {n:>8}  {fmt(t)}")
            srs.close()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    sizes = [int(s) for s in os.environ["VALIDATE_BENCH_SIZES"].split(",")] if os.environ.get("VALIDATE_BENCH_SIZES") else SIZES
    sys.stdout.reconfigure(line_buffering=True)
    import ripp_amd as R
    import ripp_amd.bls12_377 as R7
    if R.device_count() <= 0: raise SystemExit("validate_bench: no HIP device (there is nothing to measure without one)")
    print(f"# Bulk validation of untrusted points on {device_name()}: wall ms per call, {reps} timed calls after 2 warm-up calls (the compressed reader at 2^20: one call),")
    print("# host slices in, flags / points out, every call ending in a device synchronise.  Subgroup tests: phi(P) = [x^2 - 1]P on G1, psi(P) = [x]P on G2, one lane")
    print("# per point.  The byte readers parse on the library's host workers (square roots of compressed images included) and test the subgroup on the device;")
    print("# the parse of a chunk and the device check of the previous chunk do NOT overlap.  \"device check\" = ripp_validate_g1a over A | C + ripp_validate_g2a over B")
    print("# on the parsed points, \"host parse\" = the reader's median minus that.  No earlier path exists in the library to compare these with.")
    run("BLS12-381 (libripp_hip.so)", R, reps, sizes)
    run("BLS12-377 (libripp_hip_377.so)", R7, reps, sizes)


if __name__ == "__main__":
    main()
