"""The device's Montgomery square (fr_dev.hpp fr_sqr: the inline-asm v_mad_u64_u32 steps) on the GPU, against fr_mul(a, a) and a * a * 2^-256 mod p."""
import pytest

from tests.test_poseidon_lanes_cpu import check_fr_sqr


@pytest.mark.gpu
def test_device_fr_sqr_equals_fr_mul_of_a_value_with_itself():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import proof_of_burn_amd
    check_fr_sqr(proof_of_burn_amd.load_library())
