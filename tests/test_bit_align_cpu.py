"""Line-aligned BIT storage on the CPU (tests/hostsim: HIP-on-fibers shim): every sponge's stored region, every KeccakBytes.inBlocks array and the group stride are
multiples of 16 words for Spend(31), the fixture instantiation and production, the count of stored BIT wires is what it was, the padding words belong to no wire, and a
batch of three groups -- the stride at work -- emits the oracle's payload.  The GPU twin is test_bit_align_gpu.py; the bodies are tests/bit_align_cases.py."""
import pytest

from tests import bit_align_cases as BA


@pytest.fixture(scope="module")
def pkg():
    """proof_of_burn_amd with libpob_hostsim.so in place of libpob_hip.so (restored afterwards)"""
    from tests.hostsim import build as hb
    import proof_of_burn_amd
    from proof_of_burn_amd import witness as W
    lib = hb.build()
    old = (W.LIB_PATH, W._lib, dict(W._plan_cache))
    W.LIB_PATH, W._lib = lib, None
    W._plan_cache.clear()
    yield proof_of_burn_amd
    W.LIB_PATH, W._lib = old[0], old[1]
    W._plan_cache.clear(); W._plan_cache.update(old[2])


@pytest.mark.parametrize("main", [BA.SPEND, BA.POB_FIX, BA.PROD])
def test_sponges_inblocks_and_stride_are_line_aligned(pkg, main):
    """abs_b and the inBlocks base of every KeccakBytes instance and the group stride: multiples of 16; n_bit and the class identity unchanged; the padding runs end where an
    aligned array begins, sum to stride - n_bit (under 400 words) and miss the ranks the evaluator's corruption tests poke"""
    BA.check_layout(pkg, main)


@pytest.mark.parametrize("main", [BA.SPEND, BA.POB_FIX])
def test_padding_words_are_unknown_words(pkg, main):
    BA.check_padding_is_unknown(pkg, main)


def test_three_groups_emit_the_oracles_payload(pkg):
    """KeccakBytes(2), 130 witnesses: the full payload of one witness per group"""
    calc, main, inputs = BA.open_three_groups(pkg, 0)
    try:
        BA.check_payloads(calc, main, inputs)
    finally:
        calc.close()
