"""Shared bodies of the store-slot tests of the lane-spread Poseidon generation (poseidon_wide.hpp).  They run on the GPU (`tests/test_pos_slots_gpu.py`,
`-m gpu`) and on the CPU through the HIP-on-fibers shim (`tests/test_pos_slots_cpu.py`): the same product code either way.

A block's words leave in slots: in one slot every lane of a witness's 4-lane group stores one word, and a word may leave from a lane that does not hold its
element (lane 0's S-box words of a partial round, element 4's words for T = 5).  With the evaluation riding, a batch of slots is stored, then loaded back,
then compared.  What must not change: every word is stored, loaded back and compared with the value stored, and a mismatch is reported at the word's own
wire for exactly the witnesses concerned.  pob_debug_store_fault is the probe: the named word reaches memory with bit 0 flipped for the witnesses of a mask.

Batch 64 in mode set_inorder(7): one group, four 16-witness wavefronts -- the smallest shape in which every lane role and every slot exists.
"""
from __future__ import annotations

import json
import os

import numpy as np

from tests import evaluator_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEND = "Spend(31)"
POB = "ProofOfBurn(4, 4, 5, 20, 31, 2, 10 ** 18, 10 ** 19)"
CASE = {SPEND: "test_spend", POB: "test_proof_of_burn"}
# every (main, T) for which debug_ref names a block "poseidon.t{T}" (checked by blocks_named_are_these)
BLOCKS = [(SPEND, 4), (POB, 3), (POB, 4), (POB, 5)]
# ProofOfBurn's blocks that write a copy of the hash outside the block (the caller's copy): T -> the main's signal.  The main's field-element signals take FR ranks in
# declaration order from the commitment's (debug_ref "commitment"): commitment, burnKey, actualBalance, intendedBalance, revealAmount, burnExtraCommitment,
# _proofExtraCommitment, remainingCoin, nullifier (proof_of_burn.circom).  A wrong rank here fails the test: nothing would be flagged at the block's first wire.
ALSO_RANK_AFTER_COMMITMENT = {(POB, 4): 7, (POB, 3): 8}


def ok_input(main):
    with open(os.path.join(ROOT, "tests", "golden", "suites.json")) as f:
        s = next(s for s in json.load(f) if s["name"] == CASE[main])
    return next(c for c in s["cases"] if c["expected"] is not None)["input"]


def ref(calc, name, k):
    try:
        return calc.debug_ref(name, k)
    except KeyError:
        return None


def block_len(calc, T):
    return next(k for k in range(1, 1 << 14) if ref(calc, f"poseidon.t{T}", k) is None)


def layout(T, n):
    """wire offsets inside a Poseidon(T-1) block of n wires (head 4T+1 | 4 full rounds of 8T | rp partial rounds of 4+2T | 3 full rounds | tail 5T+1)"""
    rp = (n - 65 * T - 2) // (4 + 2 * T)
    assert (4 * T + 1) + 56 * T + rp * (4 + 2 * T) + (5 * T + 1) == n
    full1 = [4 * T + 1 + 8 * T * r for r in range(4)]
    part = [4 * T + 1 + 32 * T + (4 + 2 * T) * r for r in range(rp)]
    full2 = [part[-1] + 4 + 2 * T + 8 * T * r for r in range(3)]
    tail = full2[-1] + 8 * T
    return rp, full1, part, full2, tail


def words(T, n, reduced=False):
    """the words to fault, by region.  Full set: the head, full rounds 0 and 3 (the P matrix), partial rounds 0, 1 and rp - 1 (for T = 5 round rp - 1's MixS.out[4] is the
    deferred word stored behind the loop, rounds 0 and 1's are stored a round late), the first full round of the second half, the tail.  Reduced (the shim): every word of
    partial round 1, the last partial round and full round 3, plus the head and the tail"""
    rp, full1, part, full2, tail = layout(T, n)
    pw, fw = 4 + 2 * T, 8 * T
    ks = list(range(0, 4 * T + 1))
    if reduced:
        ks += list(range(full1[3], full1[3] + fw))
        ks += list(range(part[1], part[1] + pw)) + list(range(part[rp - 1], part[rp - 1] + pw))
    else:
        ks += list(range(full1[0], full1[0] + fw)) + list(range(full1[3], full1[3] + fw))
        for r in (0, 1, rp - 1):
            ks += list(range(part[r], part[r] + pw))
        ks += list(range(full2[0], full2[0] + fw))
    ks += list(range(tail, n))
    assert len(set(ks)) == len(ks) and max(ks) == n - 1
    return ks


def slice_masks(rng, count):
    """lane masks of a 64-witness group with witnesses in all four 16-witness slices (every lane position inside a slice over the set)"""
    out = [(1 << 0) | (1 << 17) | (1 << 34) | (1 << 51), (1 << 15) | (1 << 16) | (1 << 47) | (1 << 48) | (1 << 63)]
    while len(out) < count:
        m = int(rng.integers(1, 2 ** 63))
        for sl in range(4):
            m |= 1 << (16 * sl + int(rng.integers(0, 16)))
        out.append(m)
    return out[:count]


def open_calc(pkg, main, n=64, inorder=7):
    calc = pkg.WitnessCalculator(main, max_batch=n)
    calc.set_inorder(inorder)
    return calc


def flagged(calc, inputs):
    return [r.bad_wire for r in calc.calculate(inputs, check=True)]


def assert_clean(calc, inputs):
    res = calc.calculate(inputs, check=True)
    assert all(r.ok and r.bad_wire is None and r.check_status == 0 for r in res)


def blocks_named_are_these(pkg):
    for main in (SPEND, POB):
        calc = open_calc(pkg, main)
        try:
            got = [(main, T) for T in (3, 4, 5) if ref(calc, f"poseidon.t{T}", 0) is not None]
            assert got == [b for b in BLOCKS if b[0] == main]
        finally:
            calc.close()


def also_word(calc, main, T):
    """(FR rank, wire the report must name) of the caller's copy of the block's hash, or None"""
    d = ALSO_RANK_AFTER_COMMITMENT.get((main, T))
    if d is None:
        return None
    cls, idx, _ = calc.debug_ref("commitment", 0)
    assert cls == EC.FR
    return idx + d, ref(calc, f"poseidon.t{T}", 0)[2]


def check_store_faults(pkg, main, T, reduced=False):
    """one mask per word, witnesses in all four slices: exactly the masked witnesses are flagged, at the word's own wire (the caller's copy: at the block's first wire);
    then a clean generation reports nothing"""
    calc = open_calc(pkg, main)
    try:
        inputs = [ok_input(main)] * 64
        name = f"poseidon.t{T}"
        n = block_len(calc, T)
        ks = words(T, n, reduced)
        sites = []
        for k in ks:
            cls, idx, wire = ref(calc, name, k)
            assert cls == EC.FR
            sites.append((f"word {k}", idx, wire))
        also = also_word(calc, main, T)
        if also is not None:
            sites.append(("the caller's copy", also[0], also[1]))
        rng = np.random.default_rng(41 + T)
        wrong = []
        for (what, idx, wire), mask in zip(sites, slice_masks(rng, len(sites))):
            assert calc.store_fault(idx, mask, cls=EC.FR) == calc.UNKNOWN_WIRE
            got = flagged(calc, inputs)
            if got != [wire if (mask >> j) & 1 else None for j in range(64)]:
                wrong.append((what, hex(mask), wire, sorted(set(g for g in got if g is not None)), sum(g is not None for g in got)))
        assert not wrong, (main, T, len(wrong), wrong[:8])
        assert_clean(calc, inputs)
    finally:
        calc.close()


def slot_pairs(T, n):
    """pairs of words of ONE round that share a store slot, and pairs in neighbouring slots of one batch (poseidon_wide.hpp: the slot tables at posw_full and at the
    partial-round loop), as offsets k inside the block"""
    rp, full1, part, full2, tail = layout(T, n)
    p = part[2]
    if T == 5:
        share = [(p + 1, p + 2), (p + 2, p + 3), (p + 1, part[1] + 8), (p, p + 4 + T + 4),          # Sigma.in | in2 | in4 | round 1's deferred MixS.out[4]; Sigma.out | MixS.in[4]
                 (full1[1] + 16, full1[1] + 6 * T + 4), (full1[1] + 5 * T + 4, full1[1] + 7 * T + 4), (full1[1] + 17, full1[1] + 18), (full1[1] + 18, full1[1] + 19)]      # element 4's moved words of a full round
        near = [(p + 1, p), (p, p + 4 + T), (p + 4 + T + 4, p + 4 + T + 1), (p + 4 + T + 3, p + 4 + 3),
                (full1[1] + 3, full1[1] + 17), (full1[1] + 6 * T + 1, full1[1] + 16), (full1[1] + 6 * T + 4, full1[1] + 4 * T + 4)]
    else:
        share = [(p + 1, p + 2), (p + 3, p), (p + 1, p)]                                             # Sigma.in | in2 | in4 | out in one slot
        near = [(p, p + 4 + T), (p + 3, p + 4 + T + 2), (p + 4 + T + 1, p + 4 + 1)]
    share.append((tail + 4 * T, 0))                                                                   # MixLast.out | out: the hash's copies in one slot
    share.append((tail + 4 * T, T))                                                                   # ... | PoseidonEx.out
    return share, near


def check_two_faults_in_one_round(pkg, main, T):
    """two words that share a slot, or sit in neighbouring slots of one batch, faulted one after the other (one fault can be armed at a time) with OVERLAPPING masks: each
    run reports its own word's wire on exactly its mask -- a slot's compare does not smear over the lanes or slots beside it -- and over the two runs the lower wire is
    what a witness of both masks was told at least once"""
    calc = open_calc(pkg, main)
    try:
        inputs = [ok_input(main)] * 64
        name = f"poseidon.t{T}"
        n = block_len(calc, T)
        share, near = slot_pairs(T, n)
        ma = (1 << 1) | (1 << 18) | (1 << 35) | (1 << 52) | (1 << 63)
        mb = (1 << 1) | (1 << 19) | (1 << 35) | (1 << 48) | (1 << 63)
        for ka, kb in share + near:
            (_, ia, wa), (_, ib, wb) = ref(calc, name, ka), ref(calc, name, kb)
            assert calc.store_fault(ia, ma, cls=EC.FR) == calc.UNKNOWN_WIRE
            ga = flagged(calc, inputs)
            assert calc.store_fault(ib, mb, cls=EC.FR) == calc.UNKNOWN_WIRE
            gb = flagged(calc, inputs)
            assert ga == [wa if (ma >> j) & 1 else None for j in range(64)], (T, ka, kb, ga)
            assert gb == [wb if (mb >> j) & 1 else None for j in range(64)], (T, ka, kb, gb)
            for j in range(64):
                if (ma >> j) & (mb >> j) & 1:
                    assert min(ga[j], gb[j]) == min(wa, wb)
        assert_clean(calc, inputs)
    finally:
        calc.close()


def check_two_groups(pkg, main, T):
    """batch 128, a fault armed in group 1: group 0 is clean, group 1 flags exactly its mask"""
    calc = open_calc(pkg, main, n=128)
    try:
        inputs = [ok_input(main)] * 128
        n = block_len(calc, T)
        rp, full1, part, full2, tail = layout(T, n)
        mask = (1 << 0) | (1 << 21) | (1 << 42) | (1 << 63)
        for k in (part[0] + 2, part[rp - 1] + 4 + (4 if T == 5 else 1), full1[3] + (17 if T == 5 else 5), n - 1):
            _, idx, wire = ref(calc, f"poseidon.t{T}", k)
            assert calc.store_fault(idx, mask, group=1, cls=EC.FR) == calc.UNKNOWN_WIRE
            got = flagged(calc, inputs)
            assert got[:64] == [None] * 64, (T, k, got[:64])
            assert got[64:] == [wire if (mask >> j) & 1 else None for j in range(64)], (T, k, got[64:])
        assert_clean(calc, inputs)
    finally:
        calc.close()


def check_payloads(pkg, main, inorder):
    """the .wtns payloads of witnesses 0, 17 and 63 of the clean batch equal the oracle's"""
    from tests import oracle_ffi as O
    calc = open_calc(pkg, main, inorder=inorder)
    try:
        inp = ok_input(main)
        assert_clean(calc, [inp] * 64)
        want = O.run(main, inp).witness_numpy().copy()
        for idx in (0, 17, 63):
            got = calc.witness_payload(idx)
            assert got.size == want.size
            if not np.array_equal(got, want):
                d = np.nonzero((got.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1))[0]
                raise AssertionError(f"{main} inorder {inorder} witness {idx}: {d.size} wires differ from the oracle's, first {d[:8].tolist()}")
    finally:
        calc.close()
