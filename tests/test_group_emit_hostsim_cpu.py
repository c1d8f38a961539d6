"""Group emission on the CPU shim (tests/hostsim: the product's own kernels and host scheduler on fibers): the packed windows of every selected witness of a group of 64,
made by ONE pass over the resident vector (pob_emit_begin_group_packed), are byte for byte the windows the single-witness packed path hands out for each of those
witnesses, O0 and reduced, at window sizes that put partial blocks at every window edge; five lanes are also compared with the encoder on the oracle's values.  Spend(31)
takes every path of the group emitter: one sponge with its round blocks (direct tag planes, run edges), Poseidon, FR / SM / derived wires and inverses.  The GPU versions
live in test_group_emit_gpu.py.
Not covered here: SubstringCheck (U_SC_RANGE's per-witness inverses in the group emitter) -- Spend(31) has none and the smallest circuit that has one, the fixture
instantiation, is 64.4 M wires x 64 witnesses, hours on fibers; test_group_emit_gpu.py runs it on the fixture and the production circuit.  Spend's payload fits one
default window, so window sizes 0 and `whole` are the one-window case and 100 000 the multi-window one; the single path's windows are computed once per effective size."""
import pytest

from tests import group_emit_cases as GC
from tests.test_packed_hostsim_cpu import pkg  # noqa: F401  (the shim in place of libpob_hip.so)

ALL0 = (1 << 64) - 1 - (1 << GC.BAD)       # group 0 without the failed witness
ALL1 = (1 << 6) - 1                        # group 1: witnesses 64..69


@pytest.fixture(scope="module")
def spend(pkg):  # noqa: F811
    from proof_of_burn_amd.circuit_model import keepmap
    inputs = GC.spend_batch()
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=128)
    res = calc.calculate(inputs, check=True)
    assert [i for i, r in enumerate(res) if not r.ok] == [GC.BAD]
    keep, nw = keepmap.load("Spend(31)")
    assert nw == calc.nwitness
    yield calc, inputs, keep
    calc.close()


@pytest.mark.parametrize("form", ["O0", "reduced"])
def test_group_windows_equal_the_single_path_and_the_oracle(spend, form):
    calc, inputs, keep = spend
    kp = None if form == "O0" else keep
    whole = calc.nwitness if kp is None else len(kp)
    cache = {}
    for win in (0, 100_000, whole):
        g0 = GC.check_group_against_single(calc, 0, win, kp, ALL0, cache=cache)          # lanes=0 skips the failed witness and reports it absent
        g1 = GC.check_group_against_single(calc, 1, win, kp, ALL1, cache=cache)
        for g, l in GC.ORACLE_LANES:
            GC.check_lane_against_oracle("Spend(31)", inputs[64 * g + l], (g0 if g == 0 else g1)[l], kp)


def test_group_masks_refusals_and_kind_rules(spend):
    calc, _, keep = spend
    GC.check_states(calc, keep)


def test_group_wtns_files_equal_the_single_paths(spend, tmp_path):
    calc, _, keep = spend
    assert GC.check_wtns(calc, 1, None, None, tmp_path) == ALL1
    assert GC.check_wtns(calc, 0, [0, GC.BAD + 1, 63], keep, tmp_path) == (1 << 0) | (1 << (GC.BAD + 1)) | (1 << 63)
    with pytest.raises(RuntimeError):
        calc.write_wtns_group(0, {GC.BAD: str(tmp_path / "no.wtns")}, lanes=[GC.BAD])
    assert not (tmp_path / "no.wtns").exists()
