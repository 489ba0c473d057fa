"""CPU: the lane-parallel VM's layer tables (ripp_amd/csrc/vm_programs.inc) are re-derived and re-validated:
every program is list-scheduled, slot-allocated and EVALUATED with Python integers against the plain formulas
(line double/add, dense Fp12 product, homogeneous doubling and complete addition on G1 and G2), the bounds the device arithmetic
relies on are re-checked, and the committed header must be exactly what the generator emits."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


import pytest


@pytest.fixture(params=["bls12_381", "bls12_377"])
def curve(request):
    import vmgen
    vmgen.set_curve(request.param)
    yield request.param
    vmgen.set_curve("bls12_381")


def test_vm_schedules_validate_and_header_is_current(tmp_path, curve):
    """both curves: BLS12-377 has its own tables (u^2 = -5, xi = u, D-type twist with b' = 1/u carried times 5, b = 1)"""
    import vmgen
    progs = vmgen.validate()                       # asserts inside compare each schedule with the reference formulas
    assert {name for name, _ in progs} >= {"line_double", "line_add", "fp12_mul", "g1_hdbl", "g1_cadd", "g2_hdbl", "g2_cadd"}
    out = tmp_path / "vm_programs.inc"
    vmgen.emit(progs, str(out))
    committed = open(os.path.join(ROOT, vmgen.CURVE["header"])).read()
    assert out.read_text() == committed, vmgen.CURVE["header"] + " is stale: run python tools/vmgen.py"


def test_vm_layers_are_homogeneous_and_in_bounds(curve):
    """What vm.hpp::vm_run assumes about the tables: slot indices are bytes, a LIN op has at most 16 terms with |coefficient| <= 127 and a
    bias that fits 16 bits and covers its negative terms (values < 2p for program inputs and products, < 16p for unreduced LIN results),
    and a light LIN result stays below 16 p."""
    import vmgen
    import vm_model
    for (name, G), c in vmgen.validate().items():
        vm_model.check_contract(c)                 # the assertions live in tests/vm_model.py, where the model and the device tests use them too


def test_kaliski_fix_table():
    """KALISKI_FIX[k] = R^3 2^-k mod p (bls12_381/inv_table.inc), the constant that turns the almost-Montgomery inverse
    into the Montgomery form of a^-1; spot-check rows and the algorithm itself on integers."""
    p = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    R = 1 << 384
    rows = [l for l in open(os.path.join(ROOT, "ripp_amd", "csrc", "bls12_381", "inv_table.inc")) if l.startswith("{")]
    assert len(rows) == 769
    for k in (0, 1, 381, 500, 768):
        limbs = [int(x.rstrip("u"), 16) for x in rows[k].strip().rstrip(",").strip("{}").split(",")]
        assert sum(v << (32 * i) for i, v in enumerate(limbs)) == pow(R, 3, p) * pow(2, -k, p) % p
    import random
    rnd = random.Random(5)
    for a in [1, 2, p - 1] + [rnd.randrange(1, p) for _ in range(50)]:
        am = a * R % p
        u, v, r, s, k = p, am, 0, 1, 0
        while v > 0:
            if u % 2 == 0: u //= 2; s *= 2
            elif v % 2 == 0: v //= 2; r *= 2
            elif u > v: u = (u - v) // 2; r += s; s *= 2
            else: v = (v - u) // 2; s += r; r *= 2
            k += 1
            assert k <= 768
        r = r - p if r >= p else r
        assert (p - r) * (pow(R, 3, p) * pow(2, -k, p) % p) * pow(R, -1, p) % p == pow(a, -1, p) * R % p


def test_binary_gcd_inversion_model():
    """tools/inv_model.py restates the device inversion (fp_inv_bingcd) limb for limb on Python integers and asserts its invariants; the GPU
    tests compare the kernel itself with the host's Fermat inverse through every normalisation."""
    import inv_model
    assert inv_model.self_test(samples=300) == 26
