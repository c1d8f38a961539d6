"""GPU run of the store-slot tests of the lane-spread Poseidon generation (`pytest -m gpu`): libpob_hip.so on the device.  The bodies are
tests/pos_slots_cases.py; the CPU twin is test_pos_slots_cpu.py."""
import pytest

from tests import pos_slots_cases as PS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import proof_of_burn_amd
    return proof_of_burn_amd


def test_debug_ref_names_these_blocks(pkg):
    PS.blocks_named_are_these(pkg)


@pytest.mark.parametrize("main,T", PS.BLOCKS)
def test_store_fault_word_by_word(pkg, main, T):
    """every word of the head, full rounds 0 and 3, partial rounds 0, 1 and rp - 1, the first full round of the second half and the tail, and the caller's copy"""
    PS.check_store_faults(pkg, main, T)


@pytest.mark.parametrize("main,T", PS.BLOCKS)
def test_two_faults_in_one_round(pkg, main, T):
    PS.check_two_faults_in_one_round(pkg, main, T)


@pytest.mark.parametrize("main,T", PS.BLOCKS)
def test_fault_in_the_second_group(pkg, main, T):
    PS.check_two_groups(pkg, main, T)


@pytest.mark.parametrize("inorder", [1, 7])
@pytest.mark.parametrize("main", [PS.SPEND, PS.POB])
def test_payloads_equal_the_oracles(pkg, main, inorder):
    PS.check_payloads(pkg, main, inorder)
