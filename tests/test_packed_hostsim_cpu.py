"""Packed emission windows on the CPU shim (tests/hostsim: the product's own pack kernels and host scheduler on fibers): every packed window the library hands out
is byte-identical to the numpy encoder's output (tests/packed_format.py) for the oracle's canonical values of that window -- the FORMAT is pinned, not only the
round trip --, the native expansion gives the oracle's payload, the .wtns files equal the canonical paths', and the bytes the library counts as copied
device-to-host are the format's formula.  The GPU versions live in test_packed_gpu.py."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import oracle_ffi as O
from tests import packed_format as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POB_FIX = "ProofOfBurn(4, 4, 5, 20, 31, 2, 10 ** 18, 10 ** 19)"
E_STATE = -4


def _suite(name):
    with open(os.path.join(ROOT, "tests", "golden", "suites.json")) as f:
        return next(s for s in json.load(f) if s["name"] == name)


@pytest.fixture(scope="module")
def pkg():
    """proof_of_burn_amd with libpob_hostsim.so in place of libpob_hip.so (restored afterwards)"""
    from tests.hostsim import build as hb
    import proof_of_burn_amd
    from proof_of_burn_amd import witness as W
    lib = hb.build()
    old = (W.LIB_PATH, W._lib)
    W.LIB_PATH, W._lib = lib, None
    yield proof_of_burn_amd
    W.LIB_PATH, W._lib = old


def check_packed_windows(calc, idx, payload, keep, window_wires):
    """every packed window of witness idx against the encoder on the oracle's values; -> the windows' total size"""
    want = payload.reshape(-1, 32) if keep is None else payload.reshape(-1, 32)[keep]
    pos = total = 0
    for w0, wn, view in calc.packed_windows(idx, window_wires, keep=keep):
        exp = PF.encode(want[w0:w0 + wn], first_wire=w0)
        assert w0 == pos and view.size == exp.size == PF.packed_size(*PF.counts_of(want[w0:w0 + wn])), (window_wires, w0, wn, view.size, exp.size)
        assert np.array_equal(view, exp), (window_wires, w0, int(np.nonzero(view != exp)[0][0]))
        pos += wn
        total += view.size
    assert pos == want.shape[0]
    return total


def check_payload_and_bytes(calc, idx, payload, keep, window_wires, expect_total):
    want = payload if keep is None else payload.reshape(-1, 32)[keep].ravel()
    assert np.array_equal(calc.witness_payload_packed(idx, keep=keep, window_wires=window_wires), want)
    out = np.empty(want.size, dtype=np.uint8)
    sec_pinned, sec_expanded, d2h = calc.emit_throughput_packed(idx, 1, window_wires, keep=keep, out=out)
    assert d2h == expect_total and sec_pinned > 0 and sec_expanded > 0, (d2h, expect_total)
    assert np.array_equal(out, want)                                  # (the measurement's second pass expands into the caller's buffer)


def _wtns_equal(calc, idx, keep, tmp_path):
    a, b = str(tmp_path / "packed.wtns"), str(tmp_path / "canonical.wtns")
    calc.write_wtns_packed(idx, a, keep=keep)
    if keep is None:
        calc.write_wtns(idx, b)
    else:
        calc.write_wtns_reduced(idx, b, keep)
    with open(a, "rb") as fa, open(b, "rb") as fb:
        da, db = fa.read(), fb.read()
    assert len(da) == 76 + 32 * (calc.nwitness if keep is None else len(keep)) and da == db


def test_packed_spend_windows_payload_wtns_and_states(pkg, tmp_path):
    from proof_of_burn_amd.circuit_model import keepmap
    s = _suite("test_spend")
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=4)
    res = calc.calculate([c["input"] for c in s["cases"]], check=True)
    ref = O.run("Spend(31)", s["cases"][0]["input"]).witness_numpy().copy()
    ref3 = O.run("Spend(31)", s["cases"][3]["input"]).witness_numpy().copy()
    keep, nw = keepmap.load("Spend(31)")
    assert nw == calc.nwitness and res[0].ok and res[3].ok
    for kp in (None, keep):
        totals = [check_packed_windows(calc, 0, ref, kp, win) for win in (0, 100_000, calc.nwitness if kp is None else len(kp))]
        n, ns, nwide = PF.counts_of(ref if kp is None else ref.reshape(-1, 32)[kp])
        assert totals[2] == totals[0] == PF.packed_size(n, ns, nwide)      # (the default window holds all of Spend(31))
        assert totals[1] > totals[0] and totals[0] * 30 < 32 * n             # more windows: more headers and padding; 36-100 x below canonical
        check_payload_and_bytes(calc, 0, ref, kp, 100_000, totals[1])
        check_payload_and_bytes(calc, 3, ref3, kp, 0, check_packed_windows(calc, 3, ref3, kp, 0))
        _wtns_equal(calc, 0, kp, tmp_path)
    # the two kinds of emission do not mix
    lib, p, n64 = calc.lib, ctypes.c_void_p(), [ctypes.c_uint64() for _ in range(3)]
    by = ctypes.byref
    assert lib.pob_emit_begin_packed(calc.h, 0, None, 0, 100_000) == 0
    assert lib.pob_emit_next(calc.h, by(p), by(n64[0]), by(n64[1])) == E_STATE
    assert lib.pob_emit_next_packed(calc.h, by(p), by(n64[2]), by(n64[0]), by(n64[1])) == 0 and n64[1].value == 100_000      # ... and the packed emission goes on
    assert lib.pob_emit_begin(calc.h, 0, 100_000) == 0
    assert lib.pob_emit_next_packed(calc.h, by(p), by(n64[2]), by(n64[0]), by(n64[1])) == E_STATE
    assert lib.pob_emit_next(calc.h, by(p), by(n64[0]), by(n64[1])) == 0 and n64[1].value == 100_000
    assert lib.pob_emit_begin_packed(calc.h, 0, None, 5, 0) != 0      # a length without a map
    # a failed witness is refused, packed or not, announced or not
    bad_idx = next(i for i, r in enumerate(res) if not r.ok)
    for kp in (None, keep):
        with pytest.raises(RuntimeError):
            next(calc.packed_windows(bad_idx, keep=kp))
        with pytest.raises(RuntimeError):
            calc.write_wtns_packed(bad_idx, str(tmp_path / "no.wtns"), keep=kp)
    assert not os.path.exists(str(tmp_path / "no.wtns"))
    with pytest.raises(RuntimeError):                                 # the reduced form's map validation
        next(calc.packed_windows(0, keep=np.array([1, 2, 3], dtype=np.uint32)))
    calc.close()


def test_packed_emit_queue_and_selfcheck(pkg):
    s = _suite("test_spend")
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=4)
    assert [r.ok for r in calc.calculate([c["input"] for c in s["cases"]], check=True)][0]
    ref = O.run("Spend(31)", s["cases"][0]["input"]).witness_numpy().copy()
    ref3 = O.run("Spend(31)", s["cases"][3]["input"]).witness_numpy().copy()
    # two packed emissions in flight: witness 3's first window is packed behind witness 0's last ones, three slots rotate
    for win in (100_000, 1_000_000, 1_700_000):
        calc.emit_queue(3)
        for idx, want, nxt in ((0, ref, None), (3, ref3, 0), (0, ref, None)):
            pos = 0
            for w0, wn, view in calc.packed_windows(idx, win):
                if w0 == 0 and nxt is not None:
                    calc.emit_queue(nxt)
                assert w0 == pos and np.array_equal(view, PF.encode(want[32 * w0:32 * (w0 + wn)], first_wire=w0)), (win, idx, w0)
                pos += wn
            assert pos == calc.nwitness
    # a packed and a canonical emission: the first window made for the announced witness is of the OTHER kind and must not be used
    for win in (1_000_000, 1_700_000):
        calc.emit_queue(3)
        for _ in calc.packed_windows(0, win):
            pass
        got = np.concatenate([v.copy() for _, v in calc.witness_windows(3, window_wires=win)])
        assert np.array_equal(got, ref3), win
        calc.emit_queue(0)
        for _ in calc.witness_windows(3, window_wires=win):
            pass
        assert check_packed_windows(calc, 0, ref, None, win) > 0
    assert np.array_equal(calc.witness_payload_packed(3), ref3) and np.array_equal(calc.witness_payload(0), ref)
    # the emit-time self-check reads the canonical window before the pack pass: a packed emission reports what the canonical one reports
    calc.emit_selfcheck(True)
    assert np.array_equal(calc.witness_payload(0), ref)
    clean = calc.emit_selfcheck_result()
    assert np.array_equal(calc.witness_payload_packed(0), ref)
    assert calc.emit_selfcheck_result() == clean and clean["first_bad_wire"] is None and clean["checked"] > 1000
    cls, idx, wire = calc.debug_ref("kb.inLen", 0)
    calc.poke(cls, idx, 0, 1)
    canon = calc.witness_payload(0)
    r_canon = calc.emit_selfcheck_result()
    packed = calc.witness_payload_packed(0)
    r_packed = calc.emit_selfcheck_result()
    assert r_canon["first_bad_wire"] is not None and wire < r_canon["first_bad_wire"] < wire + 40_000 and r_packed == r_canon, (wire, r_canon, r_packed)
    assert np.array_equal(packed, canon) and not np.array_equal(packed, ref)
    calc.poke(cls, idx, 0, 1)
    assert np.array_equal(calc.witness_payload_packed(0), ref) and calc.emit_selfcheck_result()["first_bad_wire"] is None
    calc.emit_selfcheck(False)
    calc.close()


@pytest.mark.slow
def test_packed_fixture_windows_payload_and_wtns(pkg, tmp_path):
    from proof_of_burn_amd.circuit_model import keepmap
    s = _suite("test_proof_of_burn")
    calc = pkg.WitnessCalculator(POB_FIX, max_batch=4)
    inp = s["cases"][0]["input"]
    assert all(r.ok for r in calc.calculate([inp], check=True))
    ref = O.run(POB_FIX, inp).witness_numpy()
    keep, nw = keepmap.load(POB_FIX)
    assert nw == calc.nwitness == ref.size // 32
    for kp in (keep, None):
        whole = calc.nwitness if kp is None else len(kp)
        totals = {win: check_packed_windows(calc, 0, ref, kp, win) for win in (0, 100_000, whole)}
        n, ns, nwide = PF.counts_of(ref if kp is None else ref.reshape(-1, 32)[kp])
        assert totals[whole] == PF.packed_size(n, ns, nwide)
        if kp is not None:                                            # 5.08 MB of tags and values for the reduced witness of the fixture, plus chunk index and padding
            assert (n, ns, nwide) == (6_409_856, 42_896, 103_345) and totals[whole] == 32 + PF._pad32(16 * 100_154) + PF._pad32(8 * 1_565) + PF._pad32(4 * 42_896) + 32 * 103_345 == 5_093_664
        else:
            assert (n, ns, nwide) == (64_355_038, 175_781, 104_444)
        check_payload_and_bytes(calc, 0, ref, kp, whole, totals[whole])
        check_payload_and_bytes(calc, 0, ref, kp, 0, totals[0])
    _wtns_equal(calc, 0, keep, tmp_path)
    _wtns_equal(calc, 0, None, tmp_path)
    calc.close()
