"""Shared bodies of the sponge-chain alias tests.  They run on the GPU (`tests/test_chain_alias_gpu.py`, `-m gpu`) and on the CPU through the
HIP-on-fibers shim (`tests/test_chain_alias_cpu.py`): same product code either way.

The sponge chain stores only gate outputs -- per Absorb block Keccakf's midRound[0..24] -- and every other wire of Keccak / Final / Absorb /
Keccakf ahead of the round blocks is an alias the emitter expands: a copy of a midRound[0] / midRound[24] word, of the previous block's
midRound[24] (zero for block 0) or of KeccakBytes.inBlocks.  Two mains cover both paths of that map: KeccakBytes(1) (one block: s = zero) and
KeccakBytes(2) (s of block 1 = block 0's midRound[24], selector rows >= 1).  Wire indices come from the circuit model (the templates
restated from the reference, independent of the library's layout); the oracle is the checker.
"""
from __future__ import annotations

import json
import os

import numpy as np

from tests import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 65                                            # two groups of 64 witnesses, the second with one live lane
# circuit constants (keccak.circom): a state is 25 lanes of 64 bits, a permutation 24 rounds; a round block has 76 gate-output arrays of 64
# (20 Xor5 partials, 5 D, 25 theta, 25 chi-AND, chi.out[0] before iota) -- what a block keeps: 25 states + 24 x 76 arrays
STATE = 25 * 64
ABSORB_STORED = 25 * STATE + 24 * 76 * 64
# what the 1:1 layout stored on top of that, per permutation: Final.s[b] + Absorb.s (2 x 25 arrays), per absorbed lane Keccak.in, Final.in, Absorb.block and the
# XorArray's out, a, b + 64 triples (9 x 17), Absorb.aux + Keccakf.in (2 x 25; midRound[0] stays), Keccakf.out + Absorb.out (2 x 25): 303 arrays; Final.s[n] per sponge
COPIES_PER_PERM = (2 * 25 + 9 * 17 + 2 * 25 + 2 * 25) * 64
COPIES_PER_SPONGE = STATE
assert COPIES_PER_PERM == 303 * 64


def suite(name):
    with open(os.path.join(ROOT, "tests", "golden", "suites.json")) as f:
        return next(s for s in json.load(f) if s["name"] == name)


def batch_inputs(mb: int):
    """65 inputs: the valid cases of the committed KeccakBytes(mb) suite, cycled"""
    s = suite(f"test_keccak_{mb}")
    ok = [c["input"] for c in s["cases"] if c["expected"] is not None]
    assert ok
    return s["main"], [ok[i % len(ok)] for i in range(N)]


class Wires:
    """wire indices of KeccakBytes(mb) as main, from the circuit model's component tree"""

    def __init__(self, mb: int):
        from proof_of_burn_amd.circuit_model.keccak import KeccakBytes
        self.mb = mb
        self.main = KeccakBytes.get(mb)

    def at(self, path, sig: str, flat: int = 0) -> int:
        t, base = self.main, 1
        for name in path:
            c = next(c for c in t.children if c.name == name)
            base += c.offset
            t = c.tpl
        s = t.sigs[sig]
        assert 0 <= flat < s.size
        return base + s.offset + flat

    KECCAK = ("Keccak_484",)
    FINAL = ("Keccak_484", "Final_380")

    def absorb(self, b):
        return self.FINAL + (f"Absorb_344[{b}]",)

    def keep_list(self):
        """wire 0 + at least one wire of every aliased array kind, in every block"""
        n, k = self.mb, {0}
        for j in (0, 63, 64 * 16 + 5, 64 * 17, STATE - 1):
            k.add(self.at(self.FINAL, "s", j))                                   # Final.s[0]: zero
            for b in range(1, n):
                k.add(self.at(self.FINAL, "s", b * STATE + j))                   # Final.s[k > 0]
            k.add(self.at(self.FINAL, "s", n * STATE + j))                       # Final.s[n]
        for b in range(n):
            A = self.absorb(b)
            for j in (0, 70, 1087):
                k.add(self.at(self.KECCAK, "in", 1088 * b + j))
                k.add(self.at(self.FINAL, "in", 1088 * b + j))
                k.add(self.at(A, "block", j))
            for j in (0, 64 * 3 + 9, 64 * 16 + 63, 64 * 17 + 1, STATE - 1):
                for sig in ("out", "s", "aux"):
                    k.add(self.at(A, sig, j))
                k.add(self.at(A + ("Keccakf_322",), "in", j))
                k.add(self.at(A + ("Keccakf_322",), "out", j))
                k.add(self.at(A + ("Keccakf_322",), "midRound", j))
                k.add(self.at(A + ("Keccakf_322",), "midRound", 24 * STATE + j))
            for i in (0, 7, 16):
                X = A + (f"XorArray_317[{i}]",)
                for bit in (0, 33, 63):
                    for sig in ("out", "a", "b"):
                        k.add(self.at(X, sig, bit))
                        k.add(self.at(X + (f"XOR_82[{bit}]",), sig))             # the interleaved (o, a, b) triple
        return np.array(sorted(k), dtype=np.uint32)


def open_batch(pkg, mb: int, inorder: int = 0, n: int = N):
    main, inputs = batch_inputs(mb)
    inputs = inputs[:n]
    calc = pkg.WitnessCalculator(main, max_batch=n)
    if inorder:
        calc.set_inorder(inorder)
    res = calc.calculate(inputs, check=True)
    assert all(r.ok and r.check_status == 0 and r.bad_wire is None for r in res)
    return calc, main, inputs


def check_payloads(pkg, mb: int):
    """full and reduced payloads of witnesses of both groups against the oracle's"""
    calc, main, inputs = open_batch(pkg, mb)
    try:
        W = Wires(mb)
        assert calc.nwitness == 1 + W.main.n_wires
        keep = W.keep_list()
        for idx in (1, N - 1):
            ref = O.run(main, inputs[idx]).witness_numpy().copy()
            got = calc.witness_payload(idx)
            assert got.size == ref.size
            if not np.array_equal(got, ref):
                d = np.nonzero((got.reshape(-1, 32) != ref.reshape(-1, 32)).any(axis=1))[0]
                raise AssertionError(f"{main} witness {idx}: {d.size} wires differ from the oracle's, first {d[:8].tolist()}")
            red = calc.witness_payload_reduced(idx, keep)
            assert np.array_equal(red.reshape(-1, 32), ref.reshape(-1, 32)[keep]), f"{main} witness {idx}: reduced payload"
            # the state entering block 0 is zero, the state leaving the last block is not: the keep list does see both kinds of source
            assert not ref.reshape(-1, 32)[W.at(W.FINAL, "s", 0):W.at(W.FINAL, "s", 0) + STATE].any()
            assert ref.reshape(-1, 32)[W.at(W.FINAL, "s", mb * STATE):W.at(W.FINAL, "s", mb * STATE) + STATE].any()
    finally:
        calc.close()


def detection_sites(calc):
    """(what, BIT rank) of the stored words the chain's evaluation relates, on KeccakBytes(2)"""
    BIT = calc.CLASS_BIT
    cls, ab, abs_w = calc.debug_ref("kb.absorb", 0)
    cls2, src, _ = calc.debug_ref("kb.inBlocks", 0)
    assert cls == BIT and cls2 == BIT
    sites = []
    for b in (0, 1):
        base = ab + b * ABSORB_STORED
        sites.append((f"midRound[0][3] of block {b}", base + 64 * 3 + 11))       # i < 17: s ^ inBlocks
        sites.append((f"midRound[0][20] of block {b}", base + 64 * 20 + 40))     # i >= 17: s
    sites.append(("midRound[24][6] of block 0", ab + 24 * STATE + 64 * 6 + 2))
    sites.append(("midRound[24][19] of block 0", ab + 24 * STATE + 64 * 19 + 60))
    sites.append(("inBlocks of block 0", src + 64 * 2 + 7))
    sites.append(("inBlocks of block 1", src + 1088 + 64 * 16 + 1))
    return sites, abs_w


def check_detection(pkg, inorder: int):
    """one stored bit of witness 1 flipped at a time: witness 1 and only witness 1 is flagged (witnesses 0 and 2 are the controls), at a wire of the sponge"""
    calc, main, inputs = open_batch(pkg, 2, inorder, n=3)
    try:
        sites, abs_w = detection_sites(calc)
        W = Wires(2)
        lo = W.at((), "inBlocks", 0)                                             # the sponge's wires: KeccakBytes.inBlocks .. the end of the last Absorb block
        hi = W.at(W.absorb(1), "out", 0) + _absorb_wires()
        assert abs_w == W.at(W.absorb(0), "out", 0)
        bad = []
        for what, rank in sites:
            calc.lib.pob_debug_xor_bits(calc.h, 0, rank, 1 << 1)
            calc.constraint_check()
            res = calc.results(with_check=True)
            calc.lib.pob_debug_xor_bits(calc.h, 0, rank, 1 << 1)
            flagged = [k for k, r in enumerate(res) if r.bad_wire is not None or r.check_status != 0]
            bw = res[1].bad_wire
            print(f"inorder {inorder}: {what} (BIT rank {rank}): flagged {flagged}, bad_wire {bw}")
            if flagged != [1] or bw is None or not (lo <= bw < hi):
                bad.append((what, rank, flagged, bw, (lo, hi)))
        calc.constraint_check()
        assert all(r.bad_wire is None and r.check_status == 0 for r in calc.results(with_check=True)), "the restored vector evaluates clean"
        assert not bad, bad
    finally:
        calc.close()


def _absorb_wires() -> int:
    from proof_of_burn_amd.circuit_model.keccak import Absorb
    return Absorb.get().n_wires


def expected_n_bit_drop(info) -> int:
    """stored BIT wires the alias layout saves against the 1:1 layout, from the sponge list the library reports"""
    return COPIES_PER_PERM * int(info.n_perms) + COPIES_PER_SPONGE * int(info.n_sponges)
