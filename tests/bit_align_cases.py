"""Shared bodies of the line-alignment tests of the BIT storage.  They run on the GPU (`tests/test_bit_align_gpu.py`, `-m gpu`) and on the CPU through the
HIP-on-fibers shim (`tests/test_bit_align_cpu.py`): same product code either way.

The sponge kernels access the BIT slab as wave-wide rows of 64 eight-byte words.  The planner pads the BIT cursor so that every sponge's stored region
(`kb.absorb`) and every KeccakBytes.inBlocks array (`kb.inBlocks`) start at a rank that is a multiple of 16 words (one 128-byte line), and the groups' slabs
lie `bit_stride` words apart -- a multiple of 16 too, and no longer the number of stored BIT wires, `n_bit`.  The padding words belong to no wire.
"""
from __future__ import annotations

import numpy as np

from tests import chain_alias_cases as CA
from tests import oracle_ffi as O

LINE = 16                                         # 8-byte words per 128-byte line
SPEND = "Spend(31)"
POB_FIX = "ProofOfBurn(4, 4, 5, 20, 31, 2, 10 ** 18, 10 ** 19)"
PROD = "ProofOfBurn(16, 4, 16, 50, 31, 2, 10 ** 19, 10 ** 20)"
# stored BIT wires per instantiation as the unpadded layout counted them (the production figure is the one README and bench.py's wire_classes report)
N_BIT = {SPEND: 175_219, POB_FIX: 4_054_656, PROD: 13_496_196}
N = 130                                           # three groups of 64 witnesses: the third holds witnesses 128 and 129
# circuit constants (keccak.circom): wires of an Absorb block ahead of its round blocks, wires of a KeccakfRound block; what an Absorb block stores ahead of its
# round blocks (midRound[0..24]) and per round block (76 gate-output arrays of 64)
AB_ROUNDS_W, ROUND_WIRES = 5888 + 17 * 384 + 43200, 102656
AB_DIRECT, KR_BITS = 25 * CA.STATE, 76 * 64


def kb_refs(calc):
    """(inBlocks rank, absorb rank, absorb wire) of every KeccakBytes instance of the calculator's main"""
    out = []
    while True:
        try:
            c1, src, _ = calc.debug_ref("kb.inBlocks", len(out))
            c2, ab, abs_w = calc.debug_ref("kb.absorb", len(out))
        except KeyError:
            return out
        assert c1 == calc.CLASS_BIT and c2 == calc.CLASS_BIT
        out.append((src, ab, abs_w))


def pad_runs(calc):
    """(first rank, words) of every run of padding words of the BIT slab, in rank order"""
    out = []
    while True:
        try:
            cls, at, n = calc.debug_ref("bit.pad", len(out))
        except KeyError:
            return out
        assert cls == calc.CLASS_BIT and n > 0
        out.append((at, n))


def check_layout(pkg, main):
    """the alignment invariants of one instantiation, and that the count of stored BIT wires is what it was"""
    from proof_of_burn_amd import witness as W
    info = W.plan_info(main)
    n_bit, stride = int(info.n_bit), int(info.bit_stride)
    assert n_bit == N_BIT[main]
    assert n_bit + int(info.n_sm) + int(info.n_fr) + int(info.n_derived) + int(info.n_alias) + 1 == int(info.n_witness)
    assert stride % LINE == 0 and n_bit <= stride < n_bit + 400
    assert int(info.group_bytes) == stride * 8 + int(info.n_sm) * 256 + int(info.n_fr) * 2048
    calc = pkg.WitnessCalculator(main, max_batch=1)
    try:
        assert int(calc.info.bit_stride) == stride and int(calc.info.n_bit) == n_bit
        refs = kb_refs(calc)
        assert len(refs) == int(info.n_sponges) > 0
        for k, (src, ab, _) in enumerate(refs):
            assert src % LINE == 0, (main, k, "inBlocks", src)
            assert ab % LINE == 0, (main, k, "absorb", ab)
            assert src < stride and ab < stride
        pads = pad_runs(calc)
        assert sum(n for _, n in pads) == stride - n_bit
        # a run of padding ends where an inBlocks array or the next group's slab begins, or -- a sponge's -- ahead of the 251 BIT wires of Pad's Divide(16) +
        # AssertLessEqThan(16), the last stored BIT wires before the sponge (circuits.hpp kb_head)
        ends = {src for src, _, _ in refs} | {ab - 251 for _, ab, _ in refs} | {stride}
        for at, n in pads:
            assert 0 < n < LINE and (at + n) in ends, (main, at, n)
        # the ranks the corruption tests of the evaluator poke (100, n_bit // 2, n_bit - 5000) are stored words: none of them is padding
        for idx in (100, n_bit // 2, n_bit - 5000):
            assert not any(at <= idx < at + n for at, n in pads), (main, idx)
        return pads, stride
    finally:
        calc.close()


def check_padding_is_unknown(pkg, main):
    """pob_debug_store_fault answers for a padding word what it answers for a word no riding launch is known to store: armed without a wire"""
    calc = pkg.WitnessCalculator(main, max_batch=1)
    try:
        calc.set_inorder(7)
        pads = pad_runs(calc)
        assert pads
        for at, n in pads:
            for idx in (at, at + n - 1):
                assert calc.store_fault(idx, 0) == calc.UNKNOWN_WIRE, (main, idx)
        assert calc.lib.pob_debug_xor_bits(calc.h, 0, int(calc.info.bit_stride), 1) != 0           # the first word past the slab: refused
    finally:
        calc.close()


def open_three_groups(pkg, inorder: int):
    main, inp = CA.batch_inputs(2)
    inputs = [inp[i % len(inp)] for i in range(N)]
    calc = pkg.WitnessCalculator(main, max_batch=N)
    if inorder:
        calc.set_inorder(inorder)
    res = calc.calculate(inputs, check=True)
    assert all(r.ok and r.check_status == 0 and r.bad_wire is None for r in res)
    return calc, main, inputs


_oracle_cache: dict = {}


def oracle_payload(main, inp):
    key = (main, repr(sorted(inp.items())))
    if key not in _oracle_cache:
        _oracle_cache[key] = O.run(main, inp).witness_numpy().copy()
    return _oracle_cache[key]


def check_payloads(calc, main, inputs):
    """the full payload of one witness of each of the three groups against the oracle's"""
    buf = np.empty(32 * calc.nwitness, dtype=np.uint8)
    for idx in (3, 64 + 17, 129):
        ref = oracle_payload(main, inputs[idx])
        got = calc.witness_payload(idx, out=buf)
        assert got.size == ref.size
        if not np.array_equal(got, ref):
            d = np.nonzero((got.reshape(-1, 32) != ref.reshape(-1, 32)).any(axis=1))[0]
            raise AssertionError(f"{main} witness {idx}: {d.size} wires differ from the oracle's, first {d[:8].tolist()}")


def _flagged(calc):
    return {k: r.bad_wire for k, r in enumerate(calc.results(with_check=True)) if r.bad_wire is not None or r.check_status != 0}


def check_group2_faults(calc, inorder: int):
    """one stored round-block word and one midRound word of GROUP 2 reach memory corrupted for witness 129 (lane 1); witness 128 (the same group) and every witness of
    the other groups are the controls.  The round block's word: through pob_debug_store_fault where the generation carries its evaluation (inorder 7), through
    pob_debug_xor_bits + the evaluation's launch in the track schedule, where the hook does not exist.  The midRound word: through pob_debug_xor_bits in both -- the sponge
    chain's launch has no corrupted-store form (pob_debug_store_fault arms nothing for its words), its evaluation is a launch of pob_constraint_check.  Expected wires:
    the round block's first, the Absorb block's first."""
    src, ab, abs_w = kb_refs(calc)[0]
    absorb_wires = CA._absorb_wires()
    lanes, victim = 1 << 1, 129
    # round 5 of block 1, stored array 33, word 7
    rank_r = ab + CA.ABSORB_STORED + AB_DIRECT + 5 * KR_BITS + 64 * 33 + 7
    want_r = abs_w + absorb_wires + AB_ROUNDS_W + 5 * ROUND_WIRES
    if inorder & 4:
        assert calc.store_fault(rank_r, lanes, group=2) == want_r
        calc.generate(); calc.constraint_check()
        got = _flagged(calc)
        calc.generate(); calc.constraint_check()                           # the next generation stores the right word
    else:
        calc.lib.pob_debug_xor_bits(calc.h, 2, rank_r, lanes); calc.constraint_check()
        got = _flagged(calc)
        calc.lib.pob_debug_xor_bits(calc.h, 2, rank_r, lanes); calc.constraint_check()
    print(f"inorder {inorder}: round-block word (group 2, BIT rank {rank_r}): flagged {got}, expected wire {want_r}")
    assert got == {victim: want_r}
    assert _flagged(calc) == {}
    # midRound[0][9], word 21, of block 1: related to block 0's midRound[24] and inBlocks by the chain's evaluation (flagged at the Absorb block's first wire, the lowest)
    rank_m = ab + CA.ABSORB_STORED + 64 * 9 + 21
    want_m = abs_w + absorb_wires
    calc.lib.pob_debug_xor_bits(calc.h, 2, rank_m, lanes); calc.constraint_check()
    got = _flagged(calc)
    calc.lib.pob_debug_xor_bits(calc.h, 2, rank_m, lanes); calc.constraint_check()
    print(f"inorder {inorder}: midRound word (group 2, BIT rank {rank_m}): flagged {got}, expected wire {want_m}")
    assert got == {victim: want_m}
    assert _flagged(calc) == {}
