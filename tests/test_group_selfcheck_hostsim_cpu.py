"""The self-check of group emissions (pob_emit_group_selfcheck) on the CPU shim: the group kernels of k_selfcheck_group.hip evaluate the derived wires' relations on every
selected witness' window of the group's canonical scratch.  Spend(31) batch of 70 (tests/group_emit_cases.py: witness 9 failed, group 1 has six lanes).  Every expectation
comes from the single-witness checked packed emission of the same library (tests/group_selfcheck_cases.py).  Spend(31) has no SubstringCheck, so its M table is empty (asserted
here); the M kernels run on the fixture instantiation in test_group_selfcheck_gpu.py.

The xor cases corrupt the `inv` wire of an IsZero site.  in * inv === 1 - out and in * out === 0 hold for ANY inv when the operand is zero, so each site is armed in a lane
whose operand is not zero; where a site's operand is zero in every free lane, its `out` wire is corrupted instead (wrong whatever the operand), at the same site."""
import ctypes

import numpy as np
import pytest

from tests import group_emit_cases as GC
from tests import group_selfcheck_cases as SC
from tests.test_packed_hostsim_cpu import pkg  # noqa: F401  (the shim in place of libpob_hip.so)

ALL1 = (1 << 6) - 1
TWO = [3, 40]
XOR_LANES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 40, 63]


@pytest.fixture(scope="module")
def spend(pkg):  # noqa: F811
    from proof_of_burn_amd.circuit_model.circuits import circuit
    from proof_of_burn_amd.circuit_model.o1 import reduce_map
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=128)
    res = calc.calculate(GC.spend_batch(), check=True)
    assert [i for i, r in enumerate(res) if not r.ok] == [GC.BAD]
    m = reduce_map(circuit("Spend(31)"))
    state = {"fresh": True, "cache": {}}
    yield calc, m, np.ascontiguousarray(m.keep, dtype=np.uint32), state
    calc.close()


def test_states_come_first(spend):
    calc, _, keep, state = spend
    SC.check_states(calc, keep, state["fresh"])
    state["fresh"] = False


@pytest.mark.parametrize("form,win", [("O0", 100_000), ("O0", "whole"), ("reduced", "whole"), ("reduced", 30_000), ("alias", "whole"), ("alias", 30_000)])
def test_clean_group_emission_is_clean_counts_as_the_single_path_and_changes_no_byte(spend, form, win):
    calc, m, keep, state = spend
    state["fresh"] = False
    kp = None if form == "O0" else keep
    w = (calc.nwitness if kp is None else len(kp)) if win == "whole" else win
    calc.emit_selfcheck_alias(m if form == "alias" else None)
    try:
        cache = state["cache"].setdefault(form, {})
        SC.check_clean(calc, 1, None, ALL1, w, kp, 64 + 3, cache)
        SC.check_clean(calc, 0, TWO, SC.mask_of(TWO), w, kp, 3, cache)
    finally:
        calc.emit_selfcheck_alias(None)


@pytest.mark.parametrize("form", ["O0", "alias"])
def test_poked_lanes_are_flagged_at_the_single_paths_wire(spend, form):
    calc, m, keep, state = spend
    state["fresh"] = False
    calc.emit_selfcheck_alias(m if form == "alias" else None)
    try:
        SC.check_pokes(calc, 1, None, ALL1, [3, 5], 100_000 if form == "O0" else 30_000, None if form == "O0" else keep)
    finally:
        calc.emit_selfcheck_alias(None)


def test_every_kernel_at_a_named_site(spend):
    calc, m, keep, state = spend
    state["fresh"] = False
    z, ms, cs = calc.debug_selfcheck_sites()
    assert ms.shape == (0, 3)                           # Spend(31) has no SubstringCheck: no M sites
    assert len(z) > 100 and len(cs) > 100 and np.all(np.diff((z & 0x7FFFFFFF).astype(np.int64)) > 0) and np.any(z >> 31)      # (Spend(31)'s IsZeros are all IsEqual children)
    wins, _ = GC.group_windows(calc, 0, 0, None, XOR_LANES)
    value = SC.value_lookup(calc, wins)
    SC.check_xor_sites(calc, 0, XOR_LANES, value, SC.pick_z_sites(z), [0, len(cs) // 2, len(cs) - 1], z, cs)
    SC.check_window_edge(calc, 0, XOR_LANES[:3], value, calc.nwitness, z, cs, 100_000)
    calc.emit_selfcheck_alias(m)
    try:
        SC.check_reduced_out(calc, 0, XOR_LANES[:3], z, keep, calc._sc_alias)
    finally:
        calc.emit_selfcheck_alias(None)


def test_empty_mask(pkg):  # noqa: F811
    """a group without a good witness: lanes = 0 selects nothing, the result names the empty mask and every entry is unselected"""
    bad = dict(GC.spend_batch()[GC.BAD])
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=64)
    assert not calc.calculate([bad], check=True)[0].ok
    _, used, r = SC.group_result(calc, 0, 0, None, None)
    assert used == 0 and r == {"lanes": 0, "checked": 0, "skipped": 0, "first_bad_wire": {}}
    m, c, s, w = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7), (ctypes.c_uint32 * 64)()
    assert calc.lib.pob_emit_group_selfcheck_result(calc.h, ctypes.byref(m), ctypes.byref(c), ctypes.byref(s), w) == 0 and m.value == 0 and list(w) == [SC.NONE] * 64
    calc.close()
