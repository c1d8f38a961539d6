"""The store slots of the lane-spread Poseidon generation on the CPU (tests/hostsim: the product's kernels compiled for the host against the HIP-on-fibers
shim; the quad moves take their C form there).  The bodies are tests/pos_slots_cases.py; the GPU twin, test_pos_slots_gpu.py, faults the full word set."""
import pytest

from tests import pos_slots_cases as PS


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


def test_debug_ref_names_these_blocks(pkg):
    PS.blocks_named_are_these(pkg)


@pytest.mark.slow
@pytest.mark.parametrize("main,T", PS.BLOCKS)
def test_store_fault_word_by_word(pkg, main, T):
    """the reduced set: every word of the head, full round 3, partial round 1, the last partial round and the tail, and the caller's copy (a generation of 64
    ProofOfBurn witnesses takes the shim most of a second: about a minute per width there, ten seconds for Spend)"""
    PS.check_store_faults(pkg, main, T, reduced=True)


@pytest.mark.parametrize("main,T", [(PS.SPEND, 4), (PS.POB, 3), (PS.POB, 5)])
def test_two_faults_in_one_round(pkg, main, T):
    PS.check_two_faults_in_one_round(pkg, main, T)


@pytest.mark.parametrize("main,T", [(PS.SPEND, 4), (PS.POB, 5)])
def test_fault_in_the_second_group(pkg, main, T):
    PS.check_two_groups(pkg, main, T)


@pytest.mark.parametrize("inorder", [1, 7])
@pytest.mark.parametrize("main", [PS.SPEND, PS.POB])
def test_payloads_equal_the_oracles(pkg, main, inorder):
    PS.check_payloads(pkg, main, inorder)
