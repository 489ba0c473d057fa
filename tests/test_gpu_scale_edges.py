"""GPU (-m gpu): every form of the per-element G1 scaling (ripp_scale_g1_a -> Engine::scale_g1_dev: the field-VM kernel, the carry-free GLV kernel with its
fix-up pass, the 32-bit GLV kernel, the plain double-and-add) against the CPU oracle's scaling, bit for bit.  Scalars are per element, so one call covers the
edge list: S(curve) (tests/fold_edge_scalars.py) on a base point and on the point at infinity; one signed base-16 digit (scale.hpp: scale_bias / scale_digit)
at each of the 33 nibble positions in either GLV half; the maxima of the halves; zero scalars in the ragged tail.  n = 300 is no multiple of 16, 64 or 256.
Every case first reads ripp_config_get and checks that the call about to run takes the form it names.  All points are in G1 proper (include/ripp_hip.h)."""
import os
import random

import numpy as np
import pytest

import fold_edge_scalars as FE

pytestmark = pytest.mark.gpu
N = 300

# case -> (environment, the members of ripp_config it sets, the form scale_g1_dev takes)
CASES = {
    "vm": ({}, {}, "vm"),
    "fq": ({"RIPP_VM_SCALE_MAX": "0"}, {"vm_scale_max": 0}, "fq"),
    "32bit": ({"RIPP_VM_SCALE_MAX": "0", "RIPP_SCALE_NO_FQ": "1"}, {"vm_scale_max": 0, "scale_no_fq": 1}, "32bit"),
    "plain": ({"RIPP_NO_ENDO": "1"}, {"no_endo": 1}, "plain"),
}


def form_of(c, n):
    """the branch Engine::scale_g1_dev (engine.hip) takes for n elements under the configuration c"""
    if c.no_endo: return "plain"
    if n <= c.vm_scale_max and not c.no_vm: return "vm"
    return "32bit" if c.no_fq or c.scale_no_fq else "fq"


def _elements(curve, seed):
    """two lists of N (scalar, base: True = a point, False = infinity)"""
    r, _, lam = FE.params(curve)
    S = FE.scalars(curve)
    q = (r - 1) // lam
    rng = random.Random(seed)

    def pad(el):
        assert len(el) <= N - 8
        el += [(rng.randrange(r), True) for _ in range(N - 8 - len(el))]
        return el + [(0, True)] * 8                                             # zero scalars in the ragged tail

    a = [(s, True) for s in S] + [(s, False) for s in S]
    # one signed digit d at nibble j against one GLV base: k = d 16^j and k = (d 16^j) lambda, canonical (mod r: a negative d lands just below r)
    for j in range(33):
        for d in (-8, -1, 7):
            a += [(d * 16**j % r, True), (d * 16**j * lam % r, True)]
    a += [(lam - 1, True), (q * lam, True), (r - 1, True)]                      # the maxima: k1 = lambda - 1; k2 = floor((r - 1) / lambda), alone and with the largest k1 it admits
    # the same digits reached from non-negative halves: nibble 7 -> digit 7; nibble 8 -> digit -8 and a carry; nibble 15 -> digit -1 and a carry
    # (j = 32 holds the carry out of nibble 31 only: halves are below 2^128)
    b = []
    for j in range(32):
        for nib in (7, 8, 15):
            b += [(nib * 16**j % r, True), (nib * 16**j * lam % r, True)]
    b += [((1 << 128) - 1, True), (((1 << 128) - 1) % lam + min(q - 1, (1 << 128) - 1) * lam, True)]      # nibbles 15: carries through every position
    return pad(a), pad(b)


@pytest.fixture(scope="module", params=["381", "377"])
def curve(request, engine, orc):
    if request.param == "381":
        E, o = engine, orc
    else:
        import orclib377 as o
        import ripp_amd.bls12_377 as E
        o.lib(); E.init(0)
    r, _, _ = FE.params(request.param)
    assert r == o.R
    sets = []
    for t, el in enumerate(_elements(request.param, 0x5CA1E + int(request.param))):
        assert len(el) == N and all(0 <= s < r for s, _ in el)
        base = o.gen_g1(0x3000 + 1000 * t, N)
        for i, (_, on) in enumerate(el):
            if not on: base[i] = 0
        k = o.fr_array([s for s, _ in el])
        exp = o.scale_g1_a(base, k)
        assert not exp[[i for i, (s, on) in enumerate(el) if s == 0 or not on]].any() and exp[[i for i, (s, on) in enumerate(el) if s and on]].any(axis=1).all()
        sets.append(([s for s, _ in el], base, k, exp))
    return request.param, E, sets


@pytest.mark.parametrize("case", list(CASES))
def test_scale_form_matches_oracle_at_edge_scalars(curve, case):
    name, E, sets = curve
    env, members, form = CASES[case]
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = E.config_get()
        for k, v in members.items():
            assert getattr(c, k) == v, "%s: ripp_config.%s is %d, the case sets %d" % (case, k, getattr(c, k), v)
        for n in (N, 1):
            assert form_of(c, n) == form, "%s would run the %s form at n = %d" % (case, form_of(c, n), n)
        for t, (ss, base, ks, exp) in enumerate(sets):
            got = E.scale_g1_affine(base, ks)
            bad = np.nonzero((got != exp).any(axis=1))[0]
            assert not len(bad), "BLS12-%s %s, set %d: element %d, k = %s (base %s) differs from the oracle; %d elements differ" % (
                name, case, t, bad[0], hex(ss[bad[0]]), "at infinity" if not base[bad[0]].any() else "a point", len(bad))
        # one-element calls: a single ragged block
        ss, base, ks, exp = sets[0]
        r, _, lam = FE.params(name)
        for s in (r - 1, lam, (r - 1) // lam * lam, (1 << 128) - 1, 0):
            i = ss.index(s)
            got = E.scale_g1_affine(base[i:i + 1], ks[i:i + 1])
            assert np.array_equal(got, exp[i:i + 1]), "BLS12-%s %s, n = 1: k = %s differs from the oracle" % (name, case, hex(s))
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
