"""CPU: the Blake2b challenges of ripp_amd/csrc/host_fs.hpp (the five GIPA instantiations, the KZG challenge point, the aggregation challenge) as
pure host code.  tests/host/fs_challenges.cpp is built stand-alone for each curve and every value it prints is compared with
  * a hashlib.blake2b model written here from the byte layouts (gipa.rs:235-258, tipa/mod.rs:194-209, groth16_aggregation.rs:105-116), and
  * tests/golden/fs_challenges_{381,377}.json: what the five per-instantiation challenge functions printed for the same driver before they became one.
The model rebuilds the driver's inputs from its rules (see the head of the driver)."""
import hashlib
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


def _curve(name):
    x = -0xD201000000010000 if name == "381" else 0x8508C00000000001          # the BLS12 parameter
    r = x**4 - x**2 + 1
    return (x - 1) ** 2 * r // 3 + x, r


class Model:
    def __init__(self, name):
        self.name, (self.P, self.R) = name, _curve(name)
        self.state = 0x5EED0001

    # ---- the driver's inputs
    def next64(self):
        m = (1 << 64) - 1
        self.state = (self.state + 0x9E3779B97F4A7C15) & m
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    def draw(self, mod):
        bits = mod.bit_length()
        v = sum(self.next64() << (64 * i) for i in range((bits + 63) // 64))
        return v & ((1 << (bits - 1)) - 1)

    def fp(self): return self.draw(self.P)
    def fr(self): return self.draw(self.R)

    def member(self, kind, v, j, twin):
        P, R = self.P, self.R
        if kind == "PH": return None
        if kind == "GT":
            if v == "edge" and j: return [P - 1] * 12
            if v in ("sign", "sign0") and j: return twin
            x = [self.fp() for _ in range(12)]
            if v == "edge": x[0:3] = [0, 1, P - 1]
            return x
        if kind == "G1":
            if v == "edge": return (P - 1, 1) if j else (0, 0)
            if v in ("sign", "sign0") and j: return (twin[0], -twin[1] % P)
            return (self.fp(), self.fp())
        if kind == "G2":
            if v == "edge": return ((P - 1, 0), (1, P - 1)) if j else ((0, 0), (0, 0))
            if v in ("sign", "sign0") and j: return (twin[0], (-twin[1][0] % P, -twin[1][1] % P))
            x = ((self.fp(), self.fp()), (self.fp(), self.fp()))
            return (x[0], (x[1][0], 0)) if v == "sign0" else x
        if kind == "FR":
            if v == "edge": return R - 1 if j else 0
            if v in ("sign", "sign0") and j: return twin
            return self.fr()
        raise KeyError(kind)

    # ---- serialize_uncompressed
    def ser(self, kind, x):
        P = self.P
        if kind == "PH": return bytes(32)                                    # SSMPlaceholderCommitment: Fr::zero()
        if kind == "FR": return x.to_bytes(32, "little")
        if kind == "GT": return b"".join(c.to_bytes(48, "little") for c in x)
        if self.name == "381":                                               # zcash layout: big-endian, c1 before c0, infinity = 0x40 in the FIRST byte
            if kind == "G1": return bytes([0x40]) + bytes(95) if x == (0, 0) else x[0].to_bytes(48, "big") + x[1].to_bytes(48, "big")
            if x == ((0, 0), (0, 0)): return bytes([0x40]) + bytes(191)
            return b"".join(c.to_bytes(48, "big") for c in (x[0][1], x[0][0], x[1][1], x[1][0]))
        # generic ark-ec layout: little-endian x then y, SWFlags in the two top bits of the LAST byte, also uncompressed
        if kind == "G1":
            if x == (0, 0): return bytes(95) + bytes([0x40])
            out = bytearray(x[0].to_bytes(48, "little") + x[1].to_bytes(48, "little"))
            if x[1] > -x[1] % P: out[-1] |= 0x80
            return bytes(out)
        if x == ((0, 0), (0, 0)): return bytes(191) + bytes([0x40])
        out = bytearray(b"".join(c.to_bytes(48, "little") for c in (x[0][0], x[0][1], x[1][0], x[1][1])))
        y, ny = x[1], (-x[1][0] % P, -x[1][1] % P)
        if (y[1], y[0]) > (ny[1], ny[0]): out[-1] |= 0x80                    # Fq2 orders by c1, then c0
        return bytes(out)

    # ---- the challenges
    @staticmethod
    def until(image, accept):
        nonce = 0
        while True:
            got = accept(hashlib.blake2b(nonce.to_bytes(8, "big") + image).digest())
            if got is not None: return got
            nonce += 1

    def from_random_bytes(self, dig):
        v = int.from_bytes(dig[:32], "little") & ((1 << self.R.bit_length()) - 1)
        return v if v < self.R else None

    def gipa(self, kinds, prev, s1, s2):
        image = (prev or 0).to_bytes(32, "little")
        for s in (s1, s2):
            image += self.ser(kinds[0], s[0]) + self.ser(kinds[1], s[1]) + (1).to_bytes(8, "little") + self.ser(kinds[2], s[2])
        c128 = self.until(image, lambda d: int.from_bytes(d[:16], "big") or None)
        return [pow(c128, -1, self.R), c128]                                 # c is the inverse, c_inv the raw value (gipa.rs:252-256)

    def kzg(self, first, ck_a, ck_b):
        image = first.to_bytes(32, "little") + self.ser("G2", ck_a) + (self.ser("G1", ck_b) if ck_b is not None else b"")
        return [self.until(image, self.from_random_bytes)]

    def agg(self, a, b, c):
        return [self.until(self.ser("GT", a) + self.ser("GT", b) + self.ser("GT", c), self.from_random_bytes)]

    def run(self):
        out = {}
        for name, kinds in (("tipp", ("GT", "GT", "GT")), ("ssm", ("GT", "PH", "G1")), ("mexp", ("GT", "G1", "G1")), ("scalar", ("G2", "G1", "FR")), ("scalar_ssm", ("G1", "PH", "FR"))):
            for v in ("first", "later", "edge", "sign", "sign0"):
                prev = {"first": None, "later": None, "edge": self.R - 1, "sign": 1, "sign0": 1}[v]
                if v == "later": prev = self.fr()
                s = [None, None]
                for j in range(2): s[j] = [self.member(k, v, j, s[0][i] if j else None) for i, k in enumerate(kinds)]
                out[f"{name}_{v}"] = self.gipa(kinds, prev, s[0], s[1])
        first, ka, kb = self.fr(), self.member("G2", "first", 0, None), self.member("G1", "first", 0, None)
        out["kzg_ab"] = self.kzg(first, ka, kb)
        out["kzg_a"] = self.kzg(first, ka, None)
        out["kzg_sign_ab"] = self.kzg(1, self.member("G2", "sign", 1, ka), self.member("G1", "sign", 1, kb))
        out["kzg_edge_ab"] = self.kzg(self.R - 1, self.member("G2", "edge", 0, None), self.member("G1", "edge", 0, None))
        out["kzg_edge_a"] = self.kzg(0, self.member("G2", "edge", 1, None), None)
        g = [self.member("GT", "first", 0, None) for _ in range(3)]
        out["agg"] = self.agg(*g)
        out["agg_edge"] = self.agg(self.member("GT", "edge", 0, None), self.member("GT", "edge", 1, None), g[2])
        return {k: ["0x%064x" % x for x in v] for k, v in out.items()}


@pytest.mark.parametrize("curve", ["381", "377"])
def test_challenges_match_model_and_recorded_values(curve, tmp_path):
    exe = str(tmp_path / ("fs_challenges_" + curve))
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-mbmi2", "-DRIPP_NO_B2S_ASM"] + (["-DRIPP_BLS12_377"] if curve == "377" else [])
                          + ["-I" + os.path.join(ROOT, "ripp_amd", "csrc"), os.path.join(ROOT, "tests", "host", "fs_challenges.cpp"), "-o", exe])
    got = {}
    for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        w = ln.split(); got[w[0]] = w[1:]
    with open(os.path.join(ROOT, "tests", "golden", "fs_challenges_%s.json" % curve)) as f: recorded = json.load(f)
    model = Model(curve).run()
    assert len(got) == 32 and set(got) == set(model) == set(recorded)
    for k in got:
        assert got[k] == model[k], (k, "driver vs model")
        assert got[k] == recorded[k], (k, "driver vs recorded")
