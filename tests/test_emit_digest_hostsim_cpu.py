"""Emission digests on the CPU shim (tests/hostsim: the product's own kernels and host scheduler on fibers): every emission path -- single witness canonical and
packed, O0 and reduced, with pob_emit_queue, group emission, both self-checks, the site tables and five kinds of emission interleaved on one handle -- hands out the
bytes recorded in tests/golden/emit_digests.json (tests/emit_digest_cases.py).  The GPU version lives in test_emit_digest_gpu.py."""
import pytest

from tests import emit_digest_cases as DC
from tests.test_packed_hostsim_cpu import pkg  # noqa: F401  (the shim in place of libpob_hip.so)


@pytest.fixture(scope="module")
def digests(pkg):  # noqa: F811
    calc, keep = DC.calculator(pkg)
    got = DC.compute(calc, keep)
    calc.close()
    return got


@pytest.mark.parametrize("section", DC.SECTIONS)
def test_emission_digests_equal_the_recorded_ones(digests, section):
    DC.check_section(digests, section)
