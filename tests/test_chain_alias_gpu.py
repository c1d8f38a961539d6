"""GPU twin of test_chain_alias_cpu.py (`pytest -m gpu`): the sponge chain's alias layout through libpob_hip.so on the device."""
import pytest

from tests import chain_alias_cases as CA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import proof_of_burn_amd
    return proof_of_burn_amd


@pytest.mark.parametrize("mb", [1, 2])
def test_payloads_equal_the_oracles(pkg, mb):
    CA.check_payloads(pkg, mb)


@pytest.mark.parametrize("inorder", [0, 7])
def test_chain_evaluation_flags_every_related_word(pkg, inorder):
    CA.check_detection(pkg, inorder)
