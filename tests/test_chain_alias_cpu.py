"""The sponge chain's alias layout on the CPU (tests/hostsim: HIP-on-fibers shim): what the emitter expands from the stored gate outputs equals the
oracle's witness, the chain's evaluation flags a flip of every stored word it relates, and the layout shrank by what the copies took.  The GPU twin
is test_chain_alias_gpu.py; the bodies are tests/chain_alias_cases.py."""
import json
import os

import pytest

from tests import chain_alias_cases as CA

PROD = "ProofOfBurn(16, 4, 16, 50, 31, 2, 10 ** 19, 10 ** 20)"


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


@pytest.mark.parametrize("mb", [1, 2])
def test_payloads_equal_the_oracles(pkg, mb):
    """KeccakBytes(1): one block, s = zero; KeccakBytes(2): s of block 1 = block 0's midRound[24], selector rows >= 1.  65 witnesses; the full payload and the reduced
    payload over a keep list with wires of every aliased array kind, for a witness of each group"""
    CA.check_payloads(pkg, mb)


@pytest.mark.parametrize("inorder", [0, 7])
def test_chain_evaluation_flags_every_related_word(pkg, inorder):
    """midRound[0][i] (i < 17 and i >= 17) of both blocks, midRound[24] of block 0, inBlocks: each flip flags witness 1 alone, at a wire of the sponge"""
    CA.check_detection(pkg, inorder)


def test_production_layout_lost_the_copies(pkg):
    """n_bit of the production main = the 1:1 layout's recorded figure - (303 arrays per permutation + Final.s[n] per sponge)"""
    from proof_of_burn_amd import witness as W
    info = W.plan_info(PROD)
    with open(os.path.join(CA.ROOT, "profiles", "round6_bench_default.json")) as f:
        before = int(json.load(f)["config"]["wire_classes"]["stored_bit"])               # the 1:1 layout, as benchmarked
    assert int(info.n_perms) == 84
    assert int(info.n_bit) == before - CA.expected_n_bit_drop(info)
    assert int(info.n_bit) + int(info.n_sm) + int(info.n_fr) + int(info.n_derived) + int(info.n_alias) + 1 == int(info.n_witness)
