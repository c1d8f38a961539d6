"""Audit mode (pob_set_audit / pob_audit_last) and the generator fault that shows what it is for (pob_debug_value_fault), on the CPU shim: the product's own kernels and host
scheduler on fibers.  The cases live in tests/audit_cases.py; tests/test_audit_gpu.py runs the same functions on the device."""
from tests import audit_cases as AC
from tests.test_packed_hostsim_cpu import pkg  # noqa: F401  (the shim in place of libpob_hip.so)


def test_window_bookkeeping(pkg):  # noqa: F811
    AC.check_window_bookkeeping(pkg)


def test_a_generator_fault_leaves_riding_records_clean_and_the_audit_window_flags_it(pkg):  # noqa: F811
    AC.check_gap_and_closure(pkg)


def test_every_evaluation_family_through_a_window_with_a_first_group_other_than_zero(pkg):  # noqa: F811
    AC.check_every_family(pkg)


def test_same_records_with_and_without_the_audit_on_the_mutation_set(pkg):  # noqa: F811
    AC.check_same_records(pkg)


def test_mode_5_window_reports_a_corrupted_round_block_store_once(pkg):  # noqa: F811
    AC.check_mode5(pkg)
