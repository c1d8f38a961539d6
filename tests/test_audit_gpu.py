"""Audit mode on the MI355X (`pytest -m gpu`): the cases of tests/audit_cases.py -- window bookkeeping, the generator fault that riding cannot see and the window that flags
it, every evaluation family launched with a first group other than 0, the same records with and without the audit, mode 5 -- through the same functions as
tests/test_audit_hostsim_cpu.py.  The hooks corrupt data, never an address."""
import pytest

from tests import audit_cases as AC
from tests.test_packed_gpu import pkg  # noqa: F401

pytestmark = pytest.mark.gpu


def test_window_bookkeeping_on_the_device(pkg):  # noqa: F811
    AC.check_window_bookkeeping(pkg)


def test_a_generator_fault_leaves_riding_records_clean_and_the_audit_window_flags_it_on_the_device(pkg):  # noqa: F811
    AC.check_gap_and_closure(pkg)


def test_every_evaluation_family_through_a_window_with_a_first_group_other_than_zero_on_the_device(pkg):  # noqa: F811
    AC.check_every_family(pkg)


def test_same_records_with_and_without_the_audit_on_the_mutation_set_on_the_device(pkg):  # noqa: F811
    AC.check_same_records(pkg)


def test_mode_5_window_reports_a_corrupted_round_block_store_once_on_the_device(pkg):  # noqa: F811
    AC.check_mode5(pkg)
