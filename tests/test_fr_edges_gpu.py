"""The device forms of the field arithmetic (fr_dev.hpp, the bodies under __HIP_DEVICE_COMPILE__: product scanning with the inline-asm multiply-add step, the
Kaliski almost-inverse with batched shifts and its table, the Fermat ladder) on the GPU at their rare branches, against Python's big integers.  Inputs and checks:
tests/fr_edge_cases.py, shared with tests/test_fr_edges_cpu.py, which also shows (on the model of the inversion) what the inputs reach."""
import pytest

from tests import fr_edge_cases as E


def _lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import proof_of_burn_amd
    return proof_of_burn_amd.load_library()


@pytest.mark.gpu
def test_device_inversions_on_the_edge_set():
    """one launch of ~830 threads over the whole set (wave placement is part of the set), both outputs against pow"""
    E.check_fr_inv(_lib(), E.inv_targets())


@pytest.mark.gpu
def test_device_inversions_on_partial_wavefronts():
    """n = 1, 37, 64 + 37: the kernel returns early for t >= n and the loop's __any runs on the rest of the wavefront"""
    lib = _lib()
    for call in E.inv_partial_calls():
        E.check_fr_inv(lib, call)


@pytest.mark.gpu
def test_device_field_operations():
    E.check_fr_ops(_lib())
