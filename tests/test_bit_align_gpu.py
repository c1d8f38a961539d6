"""GPU twin of test_bit_align_cpu.py (`pytest -m gpu`): three groups of KeccakBytes(2) through libpob_hip.so on the device, in bench.py's in-order schedule and in the
track schedule -- the payload of one witness per group against the oracle's, and one corrupted round-block word and one corrupted midRound word of group 2 flagged for
exactly the witness concerned, at the expected wire."""
import pytest

from tests import bit_align_cases as BA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import proof_of_burn_amd
    return proof_of_burn_amd


@pytest.mark.parametrize("inorder", [7, 0])
def test_three_groups_payloads_and_group2_faults(pkg, inorder):
    calc, main, inputs = BA.open_three_groups(pkg, inorder)
    try:
        BA.check_payloads(calc, main, inputs)
        BA.check_group2_faults(calc, inorder)
    finally:
        calc.close()
