"""The lane-spread Poseidon generation (poseidon_wide.hpp: 16 witnesses x 4 lanes per wavefront) and the device's Montgomery square, on the CPU
through tests/hostsim (the product's own kernels compiled for the host against the HIP-on-fibers shim, test infrastructure)."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from tests import evaluator_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POB_FIX = "ProofOfBurn(4, 4, 5, 20, 31, 2, 10 ** 18, 10 ** 19)"


@pytest.fixture(scope="module")
def pkg():
    """proof_of_burn_amd with libpob_hostsim.so in place of libpob_hip.so (restored afterwards)"""
    from tests.hostsim import build as hb
    import proof_of_burn_amd
    from proof_of_burn_amd import witness as W
    lib = hb.build()
    old = (W.LIB_PATH, W._lib)
    W.LIB_PATH, W._lib = lib, None
    yield proof_of_burn_amd
    W.LIB_PATH, W._lib = old


def _case(name):
    with open(os.path.join(ROOT, "tests", "golden", "suites.json")) as f:
        s = next(s for s in json.load(f) if s["name"] == name)
    return next(c for c in s["cases"] if c["expected"] is not None)


def check_fr_sqr(lib):
    """fr_sqr (product scanning, each cross product once and doubled) against fr_mul(a, a) and against a * a * 2^-256 mod p through pob_debug_fr_sqr: zero, one,
    the limb boundaries, values next to p and to 2^253, values that make the final conditional subtraction run and not run, and random values"""
    from proof_of_burn_amd import witness as W
    P = W.P
    rinv = pow(2 ** 256, P - 2, P)
    rng = random.Random(5)
    xs = [0, 1, 2, 3, P - 1, P - 2, P - 3, (P - 1) // 2, (P + 1) // 2, 2 ** 253, 2 ** 253 - 1, 2 ** 253 % P, 2 ** 128, 2 ** 128 - 1, 2 ** 127 + 1]
    xs += [2 ** (32 * k) - 1 for k in range(1, 8)] + [2 ** (32 * k) for k in range(1, 8)] + [P - 2 ** (32 * k) for k in range(1, 8)]
    xs += [2 ** 256 % P, 2 ** 512 % P]
    # values whose product-scanning result lands in [p, 2p) before the final subtraction (most random values do not)
    nprime = -pow(P, -1, 2 ** 256) % 2 ** 256
    over = [x for x in (rng.randrange(P) for _ in range(4000)) if (x * x + (x * x * nprime % 2 ** 256) * P) >> 256 >= P]
    assert len(over) >= 16
    xs += over[:64]
    xs += [rng.randrange(P) for _ in range(300)] + [rng.randrange(2 ** 32) for _ in range(20)] + [P - 1 - rng.randrange(2 ** 64) for _ in range(20)]
    buf = b"".join(x.to_bytes(32, "little") for x in xs)
    a, b = ctypes.create_string_buffer(len(buf)), ctypes.create_string_buffer(len(buf))
    assert lib.pob_debug_fr_sqr(0, buf, len(xs), a, b) == 0
    assert a.raw == b.raw, "fr_sqr(a) != fr_mul(a, a)"
    for k, x in enumerate(xs):
        assert int.from_bytes(a.raw[32 * k:32 * k + 32], "little") == x * x * rinv % P, (k, x)


def test_fr_sqr_equals_fr_mul_of_a_value_with_itself(pkg):
    """the shim runs fr_sqr's schedule with the C form of its multiply-add step (tests/test_fr_sqr_gpu.py: the device's inline-asm form)"""
    check_fr_sqr(pkg.load_library())


def _pos_layout(T, n):
    """wire offsets inside a Poseidon(T-1) block of n wires (gadgets.hpp pos_wires: head 4T+1 | 4 full rounds of 8T | rp partial rounds of 4+2T | 3 full rounds | tail 5T+1)"""
    rp = (n - 65 * T - 2) // (4 + 2 * T)
    assert (4 * T + 1) + 56 * T + rp * (4 + 2 * T) + (5 * T + 1) == n
    full1 = [4 * T + 1 + 8 * T * r for r in range(4)]
    part = [4 * T + 1 + 32 * T + (4 + 2 * T) * r for r in range(rp)]
    full2 = [part[-1] + 4 + 2 * T + 8 * T * r for r in range(3)]
    tail = full2[-1] + 8 * T
    return rp, full1, part, full2, tail


def _element4_words(T, n):
    """(T = 5) wires that only lane 1's second element (element 4) stores: head inputs / Ark0, S-box and Ark / Mix of a full round in each half, MixS.in[4] and the
    deferred MixS.out[4] (stored a round late; the last one after the partial-round loop), the tail's S-box and MixLast.in[4]"""
    rp, full1, part, full2, tail = _pos_layout(T, n)
    ks = [4, T + 4, 2 * T + 5, 3 * T + 5]
    for off in (full1[0], full1[3], full2[1]):
        ks += [off + 16, off + 17, off + 18, off + 19, off + 4 * T + 4, off + 5 * T + 4, off + 6 * T + 4, off + 7 * T + 4]
    for r in (0, 1, rp // 2, rp - 1):
        ks += [part[r] + 8, part[r] + 4 + T + 4]
    ks += [tail + 16, tail + 17, tail + 18, tail + 19, tail + 4 * T + 5]
    return ks


def _slice_masks(rng, count):
    """lane masks of a 64-witness group with witnesses in all four 16-witness slices (every lane position inside a slice over the set)"""
    out = [(1 << 0) | (1 << 17) | (1 << 34) | (1 << 51), (1 << 15) | (1 << 16) | (1 << 47) | (1 << 48) | (1 << 63)]
    while len(out) < count:
        m = int(rng.integers(1, 2 ** 63))
        for sl in range(4):
            m |= 1 << (16 * sl + int(rng.integers(0, 16)))
        out.append(m)
    return out[:count]


@pytest.mark.parametrize("main,case,T", [("Spend(31)", "test_spend", 4), (POB_FIX, "test_proof_of_burn", 4), (POB_FIX, "test_proof_of_burn", 5)])
def test_store_fault_in_a_poseidon_block_flags_exactly_the_masked_witnesses(pkg, main, case, T):
    """pob_debug_store_fault on FR words of the first Poseidon block of width T (generated by k_pos_chain with the evaluation riding, poseidon_wide.hpp): a batch of 64
    witnesses fills one group, four 16-witness wavefronts of 4 lanes each.  Masks with witnesses in all four slices: exactly the witnesses of the mask are flagged, at the
    corrupted word's own wire.  Words drawn from the head, the full rounds, the partial rounds and the tail; for T = 5 (ProofOfBurn's burn-address hash, Poseidon(4)) every
    kind of store of the second element lane 1 holds, the deferred MixS.out[4] included.  Then a clean generation reports nothing"""
    calc = pkg.WitnessCalculator(main, max_batch=64)
    calc.set_inorder(7)
    ok = _case(case)["input"]
    name = f"poseidon.t{T}"
    n = next(k for k in range(1, 1 << 14) if _ref(calc, name, k) is None)
    rng = np.random.default_rng(29 + T)
    rp, full1, part, full2, tail = _pos_layout(T, n)
    ks = [0, 1, 2, 3, 4, n // 3, n // 2, part[0] + 1, part[-1] + 4, tail, n - 2, n - 1] + rng.integers(0, n, 6).tolist()
    if T == 5:
        ks += _element4_words(T, n)
    ks = sorted(set(ks))
    for k, mask in zip(ks, _slice_masks(rng, len(ks))):
        cls, idx, wire = _ref(calc, name, k)
        assert cls == EC.FR
        assert calc.store_fault(idx, mask, cls=cls) == calc.UNKNOWN_WIRE
        res = calc.calculate([ok] * 64, check=True)
        got = [r.bad_wire for r in res]
        assert got == [wire if (mask >> j) & 1 else None for j in range(64)], (T, k, hex(mask), wire, got)
    res = calc.calculate([ok] * 64, check=True)
    assert all(r.ok and r.bad_wire is None and r.check_status == 0 for r in res)
    calc.close()


def _ref(calc, name, k):
    try:
        return calc.debug_ref(name, k)
    except KeyError:
        return None
