"""Shared bodies of the audit-mode tests (pob_set_audit / pob_audit_last / pob_debug_value_fault).  They run on the CPU through the HIP-on-fibers shim
(tests/test_audit_hostsim_cpu.py) and on the GPU (tests/test_audit_gpu.py, `-m gpu`): the same product code, the same shapes.

Shapes: Spend(31) with 130 witnesses -- groups of 64, 64 and 2: the smallest circuit with Poseidon blocks, Num2BigEndianBytes, a sponge and round blocks, a group index
other than 0 and a partial last group -- and the fixture instantiation of ProofOfBurn with 65 witnesses (two groups), which reaches every evaluation family's launch with a
first group other than 0.

A riding calculator (set_inorder(7)) compares every store with the value the generator computed: a generator that computes a wrong value stores it, loads it back and finds
nothing.  value_fault makes exactly that happen; the audit window is what sees it.  The expected verdicts never come from the audit itself: a second constraint_check on the
same batch runs every launch over every group (the first one cleared the handle's "rode" state; audit_last then reports (0, G), asserted), i.e. the stand-alone evaluator
over the same resident vector.
"""
from __future__ import annotations

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POB_FIX = "ProofOfBurn(4, 4, 5, 20, 31, 2, 10 ** 18, 10 ** 19)"
SM, FR = 1, 2
NEAR = 16384              # a reported wire lies at or shortly before the armed one (tests/evaluator_cases.py named_pokes)
FAMILY_SEED = 20          # case 3's sample (chosen on the shim: see check_every_family)
FAMILY_HITS = 15          # covered words per storage class


def spend_inputs(n: int = 130) -> list:
    with open(os.path.join(ROOT, "tests", "golden", "test_spend_input.json")) as f:
        base = json.load(f)
    out = []
    for i in range(n):
        d = dict(base)
        d["withdrawnBalance"] = str(321 + i)
        d["extraCommitment"] = 999 + 7 * i
        out.append(d)
    return out


def verdicts(res) -> list:
    return [(r.status, r.outputs, r.check_status, r.bad_wire) for r in res]


def flagged(res) -> list:
    return [i for i, r in enumerate(res) if r.bad_wire is not None or r.check_status != 0]


def window(calc) -> tuple:
    a = calc.audit_last()
    return a["first_group"], a["n_groups"]


def standalone(calc, groups: int) -> list:
    """the stand-alone evaluator over the resident vector: a second constraint_check on the same batch runs everything"""
    calc.constraint_check()
    res = calc.results(with_check=True)
    assert window(calc) == (0, groups)
    return res


# ---------------------------------------------------------------------------------------------------------------- 1. window bookkeeping
def check_window_bookkeeping(pkg):
    inputs = spend_inputs()
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=130)
    calc.set_inorder(7)
    assert window(calc) == (0, 0)                            # before any check
    want = verdicts(calc.calculate(inputs, check=True))
    assert window(calc) == (0, 0) and calc.audit_last()["audited_batches"] == 0          # audit off

    def run(n=130):
        assert verdicts(calc.calculate(inputs[:n], check=True)) == want[:n]
        return window(calc)

    calc.set_audit(1)
    assert [run() for _ in range(4)] == [(0, 1), (1, 1), (2, 1), (0, 1)]
    assert calc.audit_last()["audited_batches"] == 4 and calc.audit_last()["audited_groups"] == 4
    calc.set_audit(2)
    assert [run() for _ in range(3)] == [(0, 2), (2, 1), (0, 2)]
    assert calc.audit_last()["audited_batches"] == 3 and calc.audit_last()["audited_groups"] == 5          # the totals restart with set_audit and add up
    calc.set_audit(1, period=2)
    assert [run() for _ in range(4)] == [(0, 1), (0, 0), (1, 1), (0, 0)]
    assert calc.audit_last()["audited_batches"] == 2 and calc.audit_last()["audited_groups"] == 2
    calc.set_audit(1000)
    assert run() == (0, 3) and run() == (0, 3)
    assert calc.audit_last()["audited_batches"] == 2 and calc.audit_last()["audited_groups"] == 6
    calc.set_audit(1)
    assert [run(), run()] == [(0, 1), (1, 1)]                # the cursor stands at 2 ...
    assert run(64) == (0, 1)                                 # ... which a batch of one group does not have: it restarts
    assert run() == (0, 1)                                   # (that batch's window reached ITS group count: the cursor returned to 0)
    assert calc.lib.pob_set_audit(calc.h, 1, 0) == -1        # period 0: POB_E_ARG
    calc.set_audit(0)
    assert run() == (0, 0)
    # a second check on the same batch evaluates everything (what the other cases use as their reference)
    assert verdicts(standalone(calc, 3)) == want
    calc.close()
    # a track-schedule handle and an in-order one whose evaluation does not ride: every check evaluates every group, whatever is set
    for mode in (None, 3):
        calc = pkg.WitnessCalculator("Spend(31)", max_batch=130)
        if mode is not None:
            calc.set_inorder(mode)
        for groups in (0, 1, 1000):
            calc.set_audit(groups)
            assert verdicts(calc.calculate(inputs, check=True)) == want
            a = calc.audit_last()
            assert (a["first_group"], a["n_groups"], a["audited_batches"], a["audited_groups"]) == (0, 3, 0, 0), (mode, groups, a)
        calc.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the gap and its closure
def poseidon_state_element(calc) -> int:
    """an FR element in the middle of the first Poseidon block (pob_debug_ref names its wires) that the hook covers: the hook names its wire, the block's wire of that rank"""
    _, f0, w0 = calc.debug_ref("poseidon", 0)
    ranks, k = [], 0
    while True:
        try:
            calc.debug_ref("poseidon", k)                    # (KeyError behind the block's last wire)
        except KeyError:
            break
        w = calc.value_fault(f0 + k, 0)                      # (mask 0: a coverage probe, arms nothing)
        if w is not None:
            assert w == w0 + k, (k, w, w0)
            ranks.append(f0 + k)
        k += 1
    assert len(ranks) > 20, (k, len(ranks))
    return ranks[len(ranks) // 2]


def check_gap_and_closure(pkg):
    inputs = spend_inputs()
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=130)
    calc.set_inorder(7)
    clean = calc.calculate(inputs, check=True)
    assert all(r.ok for r in clean) and not flagged(clean)
    f = poseidon_state_element(calc)
    # (a) audit off: a wrong commitment in clean records
    wire = calc.value_fault(f, 0b101, group=1)
    res = calc.calculate(inputs, check=True)
    assert window(calc) == (0, 0)
    assert all(r.ok and r.check_status == 0 and r.bad_wire is None for r in res)
    moved = [i for i, (a, b) in enumerate(zip(res, clean)) if a.outputs != b.outputs]
    print(f"value fault at FR rank {f} (wire {wire}), group 1, lanes 0 and 2, audit off: commitments moved for {moved}, flagged {flagged(res)}")
    assert moved == [64, 66]
    ref = standalone(calc, 3)                                # what the evaluator makes of that vector
    assert flagged(ref) == [64, 66] and all(wire - NEAR <= ref[i].bad_wire <= wire for i in (64, 66)), [(i, ref[i].bad_wire, ref[i].check_status) for i in flagged(ref)]
    calc.set_audit(1)
    # (b) the window on group 0: still clean
    assert calc.value_fault(f, 0b101, group=1) == wire
    res = calc.calculate(inputs, check=True)
    assert window(calc) == (0, 1) and not flagged(res) and [r.outputs for r in res] == [r.outputs for r in ref]
    # (c) the window on group 1: exactly witnesses 64 and 66, with the stand-alone evaluator's verdicts
    assert calc.value_fault(f, 0b101, group=1) == wire
    res = calc.calculate(inputs, check=True)
    assert window(calc) == (1, 1)
    print(f"window on group 1: flagged {[(i, res[i].bad_wire, res[i].check_status) for i in flagged(res)]}")
    assert flagged(res) == [64, 66] and verdicts(res) == verdicts(ref)
    assert verdicts(standalone(calc, 3)) == verdicts(ref)
    # (d) group 2 (two witnesses), lane 1, the window on group 2: exactly witness 129 (lanes 2.. of the partial group are neither read nor flagged)
    assert calc.value_fault(f, 0b10, group=2) == wire
    res = calc.calculate(inputs, check=True)
    assert window(calc) == (2, 1)
    ref2 = standalone(calc, 3)
    assert flagged(res) == [129] and verdicts(res) == verdicts(ref2) and wire - NEAR <= res[129].bad_wire <= wire
    assert res[129].outputs != clean[129].outputs and [r.outputs for r in res[:129]] == [r.outputs for r in clean[:129]]
    # (e) the next, clean batch reports nothing
    res = calc.calculate(inputs, check=True)
    assert window(calc) == (0, 1) and verdicts(res) == verdicts(clean)
    # what the hook refuses, and how the mirror tells it apart
    assert calc.value_fault(0, 1, cls=0) is None                                     # BIT words
    rc = calc.lib.pob_debug_value_fault(calc.h, FR, 0, int(calc.info.n_fr), 1, None)
    assert rc == -1 and "no such word" in calc.lib.pob_strerror(calc.h).decode()
    assert calc.value_fault(poseidon_block_first(calc), 1) is None                   # the block's `out` copy of the hash: not a state element
    calc.close()


def poseidon_block_first(calc) -> int:
    cls, idx, _ = calc.debug_ref("poseidon", 0)
    assert cls == FR
    return idx


# ---------------------------------------------------------------------------------------------------------------- 3. every family through a window
def fixture_batch(n: int = 65):
    from proof_of_burn_amd import inputs as gen
    from proof_of_burn_amd.witness import parse_main
    return gen.synthetic_batch(n, depth=4, params=tuple(parse_main(POB_FIX)[1])).inputs


def check_every_family(pkg, seed: int = FAMILY_SEED, hits: int = FAMILY_HITS):
    """fixture, 65 witnesses: SM and FR words drawn with a fixed seed, each armed in group 1, lane 0 (witness 64).  Per word three batches: the whole-batch audit, the window
    on group 0 (no more than the whole-batch audit flags, never a witness of group 0) and the window on group 1 (the whole-batch audit's records).  A word whose whole-batch audit is clean too is "generator-consistent"
    (no riding put stores it, or the unit does not read back what put returns and recomputes nothing from it): counted, reported, at most half of the sample."""
    inputs = fixture_batch()
    calc = pkg.WitnessCalculator(POB_FIX, max_batch=65)
    calc.set_inorder(7)
    clean = calc.calculate(inputs, check=True)
    assert all(r.ok for r in clean) and not flagged(clean)
    rng = np.random.default_rng(seed)
    sizes = calc.class_sizes()
    sample = []
    for cls in (SM, FR):
        got = 0
        for idx in rng.permutation(sizes[cls]).tolist():
            if calc.value_fault(idx, 0, cls=cls) is None:     # a word the hook refuses
                continue
            sample.append((cls, idx))
            got += 1
            if got == hits:
                break
        assert got == hits
    whole = {}
    calc.set_audit(1000)
    for cls, idx in sample:
        assert calc.value_fault(idx, 1, group=1, cls=cls) is not None
        whole[cls, idx] = calc.calculate(inputs, check=True)
        assert window(calc) == (0, 2)
    calc.set_audit(1)
    consistent = []
    for cls, idx in sample:
        ref = whole[cls, idx]
        assert all(i >= 64 for i in flagged(ref)), (cls, idx, flagged(ref))
        calc.value_fault(idx, 1, group=1, cls=cls)
        res = calc.calculate(inputs, check=True)
        # (the window on group 0 sees nothing of group 1; what may still be flagged there is what every batch gets for all groups: a failing assert downstream of the wrong
        #  value, the sponge chains' and the RLP family's evaluation -- a subset of the whole-batch audit's verdicts)
        assert window(calc) == (0, 1) and set(flagged(res)) <= set(flagged(ref)), (cls, idx, flagged(res), flagged(ref))
        calc.value_fault(idx, 1, group=1, cls=cls)
        res = calc.calculate(inputs, check=True)
        assert window(calc) == (1, 1) and verdicts(res) == verdicts(ref), (cls, idx, flagged(res), flagged(ref))
        if not flagged(ref):
            consistent.append((cls, idx))
    print(f"every family through a window, seed {seed}: {len(sample)} covered words, {len(consistent)} generator-consistent: {consistent}")
    assert 2 * len(consistent) <= len(sample)
    assert verdicts(calc.calculate(inputs, check=True)) == verdicts(clean)
    calc.close()


# ---------------------------------------------------------------------------------------------------------------- 4. same records on honest and failing inputs
def check_same_records(pkg):
    import random
    from proof_of_burn_amd import inputs as gen
    from tests.test_gpu_parity import _mutations
    params = (4, 4, 5, 20, 31, 2, 10 ** 18, 10 ** 19)
    base = gen.synthetic_batch(1, depth=2, seed=101, distinct_keys=1, params=params).inputs[0]
    cases = [c[1] for c in _mutations(base, random.Random(5))]
    groups = (len(cases) + 63) // 64
    ref = pkg.WitnessCalculator(POB_FIX, max_batch=len(cases))
    want = verdicts(ref.calculate(cases, check=True))        # the track schedule's separate evaluation pass
    ref.close()
    assert sum(1 for w in want if w[0] != 0) > 20 and sum(1 for w in want if w[0] == 0) > 5
    calc = pkg.WitnessCalculator(POB_FIX, max_batch=len(cases))
    calc.set_inorder(7)
    for audit, win in ((0, (0, 0)), (1, (0, 1)), (1000, (0, groups))):
        calc.set_audit(audit)
        got = verdicts(calc.calculate(cases, check=True))
        assert window(calc) == win
        assert got == want, (audit, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:4])
    calc.close()


# ---------------------------------------------------------------------------------------------------------------- 5. mode 5
def check_mode5(pkg):
    """set_inorder(5): the round blocks and the input rows ride, the G units do not: the window adds the round kernel and the input check only.  A corrupted STORE in a round
    block of group 1 (store_fault) is reported by the riding launch; the window's round kernel finds the same word at the same wire: once, the same records"""
    inputs = spend_inputs()
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=130)
    calc.set_inorder(5)
    clean = calc.calculate(inputs, check=True)
    assert not flagged(clean)
    rng = np.random.default_rng(3)
    bit_index = next(i for i in rng.integers(0, int(calc.info.n_bit), 400).tolist() if calc.store_fault(i, 0, group=1) != calc.UNKNOWN_WIRE)
    lanes = 0b1001
    want = calc.store_fault(bit_index, lanes, group=1)
    off = calc.calculate(inputs, check=True)
    assert window(calc) == (0, 0) and flagged(off) == [64, 67] and all(off[i].bad_wire == want for i in (64, 67))
    calc.set_audit(1)
    assert verdicts(calc.calculate(inputs, check=True)) == verdicts(clean) and window(calc) == (0, 1)
    assert calc.store_fault(bit_index, lanes, group=1) == want
    res = calc.calculate(inputs, check=True)
    assert window(calc) == (1, 1) and verdicts(res) == verdicts(off)
    assert calc.store_fault(bit_index, lanes, group=1) == want       # ... and with the window elsewhere
    res = calc.calculate(inputs, check=True)
    assert window(calc) == (2, 1) and verdicts(res) == verdicts(off)
    assert verdicts(calc.calculate(inputs, check=True)) == verdicts(clean)
    calc.close()
