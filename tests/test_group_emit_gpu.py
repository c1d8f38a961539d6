"""Group emission on the MI355X (`pytest -m gpu`): the packed windows of every selected witness of a group of 64 from ONE pass over the resident vector
(pob_emit_begin_group_packed) against the single-witness packed path of the same library -- which test_packed_gpu.py pins to the oracle -- byte for byte for Spend(31)
and the fixture instantiation, by digest and size for one production group; a few lanes also against the encoder on the oracle's values.  The CPU-shim versions of the
Spend checks live in test_group_emit_hostsim_cpu.py."""
import time

import numpy as np
import pytest

from tests import group_emit_cases as GC
from tests import oracle_ffi as O
from tests.test_packed_gpu import PROD, pkg  # noqa: F401
from tests.test_packed_hostsim_cpu import POB_FIX

pytestmark = pytest.mark.gpu
ALL0 = (1 << 64) - 1 - (1 << GC.BAD)
ALL1 = (1 << 6) - 1


def test_group_spend_on_the_device(pkg, tmp_path):  # noqa: F811
    from proof_of_burn_amd.circuit_model import keepmap
    t0 = time.time()
    inputs = GC.spend_batch()
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=128)
    res = calc.calculate(inputs, check=True)
    assert [i for i, r in enumerate(res) if not r.ok] == [GC.BAD]
    keep, _ = keepmap.load("Spend(31)")
    for kp in (None, keep):
        whole = calc.nwitness if kp is None else len(kp)
        cache = {}
        for win in (0, 100_000, whole):
            g0 = GC.check_group_against_single(calc, 0, win, kp, ALL0, cache=cache)
            g1 = GC.check_group_against_single(calc, 1, win, kp, ALL1, cache=cache)
            for g, l in GC.ORACLE_LANES:
                GC.check_lane_against_oracle("Spend(31)", inputs[64 * g + l], (g0 if g == 0 else g1)[l], kp)
    GC.check_states(calc, keep)
    assert GC.check_wtns(calc, 1, None, None, tmp_path) == ALL1
    assert GC.check_wtns(calc, 0, [0, GC.BAD + 1, 63], keep, tmp_path) == (1 << 0) | (1 << (GC.BAD + 1)) | (1 << 63)
    calc.close()
    print(f"group GPU test, Spend(31): {time.time() - t0:.0f} s")


def test_group_fixture_on_the_device(pkg):  # noqa: F811
    from proof_of_burn_amd import inputs as gen
    from proof_of_burn_amd.circuit_model import keepmap
    from proof_of_burn_amd.witness import parse_main
    t0 = time.time()
    params = tuple(parse_main(POB_FIX)[1])
    batch = gen.synthetic_batch(66, depth=4, params=params)
    calc = pkg.WitnessCalculator(POB_FIX, max_batch=128)
    assert all(r.ok for r in calc.calculate(batch.inputs, check=True))
    keep, _ = keepmap.load(POB_FIX)
    for kp in (None, keep):
        for win in (0, 1_000_003):                                  # the default window and one that is no multiple of 64
            g0 = GC.check_group_against_single(calc, 0, win, kp, (1 << 64) - 1)
            GC.check_group_against_single(calc, 1, win, kp, 0b11)
        GC.check_lane_against_oracle(POB_FIX, batch.inputs[41], g0[41], kp)
    calc.close()
    print(f"group GPU test, fixture: {time.time() - t0:.0f} s")


def test_group_production_by_digest(pkg):  # noqa: F811
    """one production group of 64, O0 and reduced at the default window: per lane and window the digest and size of the single-witness packed path, and the group's
    device-to-host bytes equal the sum of the 64 single emissions'"""
    from proof_of_burn_amd import inputs as gen
    from proof_of_burn_amd.circuit_model import keepmap
    t0 = time.time()
    keep, _ = keepmap.load(PROD)
    batch = gen.synthetic_batch(64, depth=10, seed=0xB0B, distinct_keys=2)
    calc = pkg.WitnessCalculator(PROD, max_batch=64)
    assert all(r.ok for r in calc.calculate(batch.inputs, check=True))
    for name, kp in (("O0", None), ("reduced", keep)):
        got = {}
        for w0, wn, views in calc.group_packed_windows(0, 0, keep=kp):
            for l, v in views.items():
                got.setdefault(l, []).append((w0, wn, O.payload_digest(v), int(v.size)))
        assert calc.group_lanes == (1 << 64) - 1 and sorted(got) == list(range(64))
        total = 0
        for l in range(64):
            want = [(w0, wn, O.payload_digest(v), int(v.size)) for w0, wn, v in calc.packed_windows(l, 4 << 20, keep=kp)]      # (the group path's default window)
            assert got[l] == want, (name, l)
            total += sum(w[3] for w in want)
        s0, _, d2h = calc.emit_throughput_group(0, 1, 0, keep=kp)
        assert d2h == total, (name, d2h, total)
        print(f"production {name}: group of 64 in {s0 * 1e3:.0f} ms ({s0 * 1e3 / 64:.2f} ms per witness), {d2h} B device-to-host")
    calc.close()
    print(f"group GPU test, production: {time.time() - t0:.0f} s")
