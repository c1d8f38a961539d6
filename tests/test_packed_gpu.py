"""Packed emission windows on the MI355X (`pytest -m gpu`): the pack kernels' output is byte-identical to the numpy encoder's (tests/packed_format.py) on the oracle's
values, window by window, for Spend(31) and the fixture instantiation, O0 and reduced; and for ONE production witness, O0 and reduced, by digest per window against
an oracle run that a worker process makes beside the GPU.  The CPU-shim versions of these checks live in test_packed_hostsim_cpu.py."""
import json
import os
import time

import numpy as np
import pytest

from tests import oracle_ffi as O
from tests import packed_format as PF
from tests.test_packed_hostsim_cpu import POB_FIX, _wtns_equal, check_packed_windows, check_payload_and_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROD = "ProofOfBurn(16, 4, 16, 50, 31, 2, 10 ** 19, 10 ** 20)"


def _suite(name):
    with open(os.path.join(ROOT, "tests", "golden", "suites.json")) as f:
        return next(s for s in json.load(f) if s["name"] == name)


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import proof_of_burn_amd
    return proof_of_burn_amd


def test_packed_spend_on_the_device(pkg, tmp_path):
    from proof_of_burn_amd.circuit_model import keepmap
    t0 = time.time()
    s = _suite("test_spend")
    calc = pkg.WitnessCalculator("Spend(31)", max_batch=4)
    res = calc.calculate([c["input"] for c in s["cases"]], check=True)
    ref = O.run("Spend(31)", s["cases"][0]["input"]).witness_numpy().copy()
    ref3 = O.run("Spend(31)", s["cases"][3]["input"]).witness_numpy().copy()
    keep, _ = keepmap.load("Spend(31)")
    for kp in (None, keep):
        whole = calc.nwitness if kp is None else len(kp)
        totals = {win: check_packed_windows(calc, 0, ref, kp, win) for win in (0, 100_000, whole)}
        assert totals[whole] == PF.packed_size(*PF.counts_of(ref if kp is None else ref.reshape(-1, 32)[kp]))
        check_payload_and_bytes(calc, 0, ref, kp, 100_000, totals[100_000])
        calc.emit_queue(0)                                           # two packed emissions in flight, then a canonical one behind a packed announcement
        check_payload_and_bytes(calc, 3, ref3, kp, 100_000, check_packed_windows(calc, 3, ref3, kp, 100_000))
        assert check_packed_windows(calc, 0, ref, kp, 100_000) == totals[100_000]
        calc.emit_queue(3)
        for _ in calc.packed_windows(0, 1_000_000, keep=kp):
            pass
        got = np.concatenate([v.copy() for _, v in calc.witness_windows(3, window_wires=1_000_000, keep=kp)])
        assert np.array_equal(got, ref3 if kp is None else ref3.reshape(-1, 32)[kp].ravel())
        _wtns_equal(calc, 0, kp, tmp_path)
    bad_idx = next(i for i, r in enumerate(res) if not r.ok)
    with pytest.raises(RuntimeError):
        next(calc.packed_windows(bad_idx))
    # the emit-time self-check sees the canonical window in front of the pack pass
    calc.emit_selfcheck(True)
    cls, idx, wire = calc.debug_ref("kb.inLen", 0)
    calc.poke(cls, idx, 0, 1)
    canon = calc.witness_payload(0)
    r_canon = calc.emit_selfcheck_result()
    packed = calc.witness_payload_packed(0)
    assert calc.emit_selfcheck_result() == r_canon and r_canon["first_bad_wire"] is not None and np.array_equal(packed, canon)
    calc.poke(cls, idx, 0, 1)
    assert np.array_equal(calc.witness_payload_packed(0), ref) and calc.emit_selfcheck_result()["first_bad_wire"] is None
    calc.close()
    print(f"packed GPU test, Spend(31): {time.time() - t0:.0f} s")


def test_packed_fixture_on_the_device(pkg, tmp_path):
    from proof_of_burn_amd.circuit_model import keepmap
    t0 = time.time()
    s = _suite("test_proof_of_burn")
    calc = pkg.WitnessCalculator(POB_FIX, max_batch=4)
    inp = s["cases"][0]["input"]
    assert all(r.ok for r in calc.calculate([inp, inp], check=True))
    ref = O.run(POB_FIX, inp).witness_numpy()
    keep, _ = keepmap.load(POB_FIX)
    for kp in (keep, None):
        whole = calc.nwitness if kp is None else len(kp)
        totals = {win: check_packed_windows(calc, 1, ref, kp, win) for win in (0, 100_000, whole)}
        n, ns, nwide = PF.counts_of(ref if kp is None else ref.reshape(-1, 32)[kp])
        assert totals[whole] == PF.packed_size(n, ns, nwide)
        assert (n, ns, nwide) == ((6_409_856, 42_896, 103_345) if kp is not None else (64_355_038, 175_781, 104_444))
        check_payload_and_bytes(calc, 1, ref, kp, 0, totals[0])
        _wtns_equal(calc, 0, kp, tmp_path)
    calc.close()
    print(f"packed GPU test, fixture: {time.time() - t0:.0f} s")


def _window_digests(vals, window):
    out = []
    for w0 in range(0, vals.shape[0], window):
        enc = PF.encode(vals[w0:w0 + window], first_wire=w0)
        out.append((O.payload_digest(enc), int(enc.size)) + PF.counts_of(vals[w0:w0 + window]))
    return out


def _prod_worker(args):
    """in a worker process: the oracle's production witness -> per default window the digest, size and counts of its packed form, O0 and reduced, and the payloads' digests"""
    main, inp, keep, win_o0, win_red = args
    r = O.run(main, inp)
    assert not r.failed
    v = r.witness_numpy().reshape(-1, 32)
    o0 = _window_digests(v, win_o0)
    d_o0 = O.payload_digest(r.witness_numpy())
    red = np.ascontiguousarray(v[keep])
    O.lib().oracle_free()
    return o0, d_o0, _window_digests(red, win_red), O.payload_digest(red)


def test_packed_production_witness_by_digest(pkg):
    """one production witness, O0 (26 windows of 8 Mi wires) and reduced (two windows of 16 Mi kept wires): every packed window's digest and size equal those of the
    encoder's output on the oracle's values; the native expansion of the transfer gives the oracle's payload.  Prints the byte counts that profiles/emit_packed.txt quotes."""
    from proof_of_burn_amd import inputs as gen
    from proof_of_burn_amd.circuit_model import keepmap
    t0 = time.time()
    keep, _ = keepmap.load(PROD)
    batch = gen.synthetic_batch(2, depth=10, seed=0xB0B, distinct_keys=2)
    win_o0, win_red = 8 << 20, 1 << 24
    with O.OraclePool(procs=2) as pool:
        job = pool.pool.apply_async(_prod_worker, ((PROD, batch.inputs[1], keep, win_o0, win_red),))
        calc = pkg.WitnessCalculator(PROD, max_batch=2)
        res = calc.calculate(batch.inputs, check=True)
        assert all(r.ok and r.check_status == 0 and r.bad_wire is None for r in res)
        got = {}
        for name, kp, win in (("O0", None, win_o0), ("reduced", keep, win_red)):
            got[name] = [(w0, wn, O.payload_digest(view), int(view.size)) for w0, wn, view in calc.packed_windows(1, win, keep=kp)]
        buf = np.empty(32 * calc.nwitness, dtype=np.uint8)
        t1 = time.time()
        sec_pinned, sec_expanded, d2h_o0 = calc.emit_throughput_packed(1, 1, win_o0, out=buf)
        dig_o0 = O.payload_digest(buf)
        red_buf = buf[:32 * len(keep)]
        _, _, d2h_red = calc.emit_throughput_packed(1, 1, win_red, keep=keep, out=red_buf)
        dig_red = O.payload_digest(red_buf)
        t_gpu = time.time() - t1
        o0, d_o0, red, d_red = job.get(900)
    for name, want, total in (("O0", o0, calc.nwitness), ("reduced", red, len(keep))):
        assert len(got[name]) == len(want), name
        pos = 0
        for (w0, wn, dig, size), (wdig, wsize, n, ns, nwide) in zip(got[name], want):
            assert (w0, wn, size) == (pos, n, wsize) and dig == wdig, (name, w0, wn, size, wsize)
            pos += wn
        assert pos == total
        nbytes = sum(w[1] for w in want)
        print(f"production {name}: {total} wires, value 2..2^32-1: {sum(w[3] for w in want)}, wider: {sum(w[4] for w in want)}, canonical {32 * total} B, "
              f"packed {nbytes} B in {len(want)} windows ({32 * total / nbytes:.1f} x)")
        assert (d2h_o0 if name == "O0" else d2h_red) == nbytes, name
    assert dig_o0 == d_o0 and dig_red == d_red
    calc.close()
    print(f"packed GPU test, production: {time.time() - t0:.0f} s (of which {t_gpu:.1f} s the two expanded emissions and their digests)")
