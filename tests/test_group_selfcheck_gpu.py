"""The self-check of group emissions (pob_emit_group_selfcheck) on the MI355X (`pytest -m gpu`): the Spend(31) cases of test_group_selfcheck_hostsim_cpu.py on the device,
through the same functions, and the fixture instantiation -- the smallest circuit with a SubstringCheck and therefore M sites -- at a window that is no multiple of 64:
four lanes of group 0 and both of group 1, O0 and reduced, clean, counted as the single path counts, every M kernel reached at a named site through the xor hook, poked
lanes flagged at the single path's wire.  The reference is always the single-witness checked packed emission (tests/group_selfcheck_cases.py).  The hooks corrupt data in a
scratch buffer or the resident vector, never an address."""
import time

import numpy as np
import pytest

from tests import group_emit_cases as GC
from tests import group_selfcheck_cases as SC
from tests import test_group_selfcheck_hostsim_cpu as H
from tests.test_packed_gpu import pkg  # noqa: F401
from tests.test_packed_hostsim_cpu import POB_FIX

pytestmark = pytest.mark.gpu
FIX_WIN = 1_000_003
FIX_LANES = [0, 17, 41, 63]


def test_group_selfcheck_spend_on_the_device(pkg):  # noqa: F811
    from proof_of_burn_amd.circuit_model.circuits import circuit
    from proof_of_burn_amd.circuit_model.o1 import reduce_map
    t0 = time.time()
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=128)
    res = calc.calculate(GC.spend_batch(), check=True)
    assert [i for i, r in enumerate(res) if not r.ok] == [GC.BAD]
    m = reduce_map(circuit("Spend(31)"))
    spend = (calc, m, np.ascontiguousarray(m.keep, dtype=np.uint32), {"fresh": True, "cache": {}})
    H.test_states_come_first(spend)
    for form, win in (("O0", 100_000), ("O0", "whole"), ("reduced", "whole"), ("reduced", 30_000), ("alias", "whole"), ("alias", 30_000)):
        H.test_clean_group_emission_is_clean_counts_as_the_single_path_and_changes_no_byte(spend, form, win)
    for form in ("O0", "alias"):
        H.test_poked_lanes_are_flagged_at_the_single_paths_wire(spend, form)
    H.test_every_kernel_at_a_named_site(spend)
    calc.close()
    H.test_empty_mask(pkg)
    print(f"group self-check GPU test, Spend(31): {time.time() - t0:.0f} s")


def test_group_selfcheck_fixture_on_the_device(pkg):  # noqa: F811
    from proof_of_burn_amd import inputs as gen
    from proof_of_burn_amd.circuit_model import keepmap
    from proof_of_burn_amd.witness import parse_main
    t0 = time.time()
    batch = gen.synthetic_batch(66, depth=4, params=tuple(parse_main(POB_FIX)[1]))
    calc = pkg.WitnessCalculator(POB_FIX, max_batch=128)
    assert all(r.ok for r in calc.calculate(batch.inputs, check=True))
    keep, _ = keepmap.load(POB_FIX)
    z, ms, cs = calc.debug_selfcheck_sites()
    assert len(ms) > 0 and len(z) > 50_000
    cache = {}
    wins = None
    for kp in (None, keep):
        got, r0 = SC.check_clean(calc, 0, FIX_LANES, SC.mask_of(FIX_LANES), FIX_WIN, kp, 41, cache)
        wins = wins or got
        _, r1 = SC.check_clean(calc, 1, None, 0b11, FIX_WIN, kp, 41, cache)
        assert (r0["checked"], r0["skipped"]) == (r1["checked"], r1["skipped"])
    # every M kernel at a named site: M[k+1] of the first, the middle and the last step of the recurrence, one emission each, in lane 17 alone
    for i in (0, len(ms) // 2, len(ms) - 1):
        wire = int(ms[i][0])
        calc.debug_group_emit_xor(17, wire, byte=0, mask=1)
        _, _, r = SC.group_result(calc, 0, FIX_WIN, None, FIX_LANES)
        print(f"M site {i} (wire {wire}): {r['first_bad_wire']}")
        assert r["first_bad_wire"] == {l: (wire if l == 17 else None) for l in FIX_LANES}, (i, wire, r)
    # a bare IsZero (Spend(31) has none) and an IsEqual child, inv corrupted in a lane whose operand is not zero
    bare, child = np.nonzero((z >> 31) == 0)[0], np.nonzero(z >> 31)[0]
    print(f"fixture: {len(bare)} bare IsZero sites, {len(child)} IsEqual children, {len(ms)} M sites, {len(cs)} copy sites")
    SC.check_xor_sites(calc, 0, FIX_LANES, SC.value_lookup(calc, wins), [int(a[len(a) // 2]) for a in (bare, child) if len(a)], [], z, cs, win=FIX_WIN)
    SC.check_pokes(calc, 0, FIX_LANES, SC.mask_of(FIX_LANES), [0, 63], FIX_WIN, None)
    # The reduced kernels on this circuit.  Under the stored keep map (no alias map) no site has all of its own wires kept -- the clean runs above count 0 checked -- and the
    # M wires are linear, so the map drops them: both lists are empty, stated here.  A map that also keeps the wires of every M step and of the IsZero sites around
    # KeccakBytes.inLen puts those sites on the lists (a site whose own wires are all kept needs no alias): k_selfcheck_group_zr / _mr see them clean, count as the single
    # path counts, name the corrupted M step and the corrupted IsZero site.
    zr, mr = calc.debug_selfcheck_reduced_lists()
    assert len(zr) == 0 and len(mr) == 0, (len(zr), len(mr))
    # ... so the poke of inLen in lanes 0 and 63 under the stored map: the group path reports what the single path reports for those witnesses -- nothing, asserted
    cls, idx, _ = calc.debug_ref("kb.inLen", 0)
    for l in (0, 63):
        calc.poke(cls, idx, l, 1, group=0)
    try:
        _, _, r = SC.group_result(calc, 0, FIX_WIN, keep, FIX_LANES)
        want = {l: SC.single_result(calc, l, FIX_WIN, keep)["first_bad_wire"] for l in (0, 63)}
    finally:
        for l in (0, 63):
            calc.poke(cls, idx, l, 1, group=0)
    print(f"pokes in lanes 0 and 63, reduced form with the stored map: group {r['first_bad_wire']}, single {want}")
    assert want == {0: None, 63: None} and r["first_bad_wire"] == {l: want.get(l) for l in FIX_LANES}, (r, want)
    _, _, inlen_wire = calc.debug_ref("kb.inLen", 0)
    near = z[((z & 0x7FFFFFFF) >= inlen_wire) & ((z & 0x7FFFFFFF) < inlen_wire + 200_000)]
    extra = np.concatenate([np.array(SC.z_wires(s), dtype=np.uint32) for s in near] + [ms[:, 0], ms[:, 0] - 1, ms[:, 1]])
    keep2 = np.union1d(keep, extra).astype(np.uint32)
    SC.check_clean(calc, 0, FIX_LANES, SC.mask_of(FIX_LANES), FIX_WIN, keep2, 41, cache)
    zr, mr = calc.debug_selfcheck_reduced_lists()
    print(f"fixture, keep map + {len(keep2) - len(keep)} wires: {len(zr)} IsZero sites and {len(mr)} M steps on the reduced lists")
    assert len(zr) == len(near) > 0 and len(mr) == len(ms)
    for i in (0, len(ms) // 2, len(ms) - 1):
        wire = int(ms[i][0])
        calc.debug_group_emit_xor(17, wire, byte=0, mask=1)
        _, _, r = SC.group_result(calc, 0, FIX_WIN, keep2, FIX_LANES)
        print(f"reduced form, M site {i} (wire {wire}): {r['first_bad_wire']}")
        assert r["first_bad_wire"] == {l: (wire if l == 17 else None) for l in FIX_LANES}, (i, wire, r)
    # k_selfcheck_group_zr: `out` of the first and of the last listed IsZero site corrupted in lanes 0 and 63 (wrong whatever the operand); each names its site's first
    # listed wire.  (A poked inLen is NOT visible in this form without an alias map, to either path -- asserted above.
    # The IsZero sites stay consistent among themselves, all derived from the poked value; what the poke breaks is their copy constraints against the stored isEq bits,
    # which the reduced form counts as skipped.  The Spend(31) cases flag that poke in the reduced form through an alias map.)
    expect = {0: int(near[0]) & 0x7FFFFFFF, 63: int(near[-1]) & 0x7FFFFFFF}
    for l, w in expect.items():
        calc.debug_group_emit_xor(l, w, byte=0, mask=1)
    _, _, r = SC.group_result(calc, 0, FIX_WIN, keep2, FIX_LANES)
    print(f"reduced form, out wires {expect} corrupted: {r['first_bad_wire']}")
    assert r["first_bad_wire"] == {l: expect.get(l) for l in FIX_LANES}, r
    calc.close()
    print(f"group self-check GPU test, fixture: {time.time() - t0:.0f} s")
