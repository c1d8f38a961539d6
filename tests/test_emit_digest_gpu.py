"""Emission digests on the MI355X (`pytest -m gpu`): the calls of test_emit_digest_hostsim_cpu.py against the device build -- the same bytes, self-check counts and
site tables as tests/golden/emit_digests.json records (tests/emit_digest_cases.py)."""
import pytest

from tests import emit_digest_cases as DC
from tests.test_packed_gpu import pkg  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def digests(pkg):  # noqa: F811
    calc, keep = DC.calculator(pkg)
    got = DC.compute(calc, keep)
    calc.close()
    return got


@pytest.mark.parametrize("section", DC.SECTIONS)
def test_emission_digests_equal_the_recorded_ones(digests, section):
    DC.check_section(digests, section)
