"""Shared by the group-emission tests (CPU shim and GPU): the Spend(31) batch of 70 with one failing input, and the comparison of a group emission with the single-witness
packed path of the same library, window by window and byte for byte."""
import ctypes

import numpy as np

from tests import oracle_ffi as O
from tests import packed_format as PF

E_STATE = -4
GROUP_DEFAULT_WINDOW = 4 << 20      # window_wires = 0 of pob_emit_begin_group_packed (include/pob_hip.h)
BAD = 9                     # the witness of the Spend batch that fails its assert (group 0, lane 9)
ORACLE_LANES = ((0, 0), (0, 1), (0, 37), (0, 63), (1, 5))      # (group, lane) compared with the oracle as well


def spend_batch():
    """70 witnesses: a full group, a group of 6, and witness BAD withdrawing more than its balance (spend.circom:41)"""
    from proof_of_burn_amd import inputs as gen
    inputs = [dict(d) for d in gen.synthetic_spend_batch(70).inputs]
    inputs[BAD]["withdrawnBalance"] = str(int(inputs[BAD]["balance"]) + 1)
    return inputs


def single_windows(calc, idx, window_wires, keep):
    return [(w0, wn, v.copy()) for w0, wn, v in calc.packed_windows(idx, window_wires, keep=keep)]


def group_windows(calc, group, window_wires, keep, lanes=None):
    """-> {lane: [(first_wire, n_wires, bytes), ...]} and the mask the library used"""
    out = {}
    for w0, wn, views in calc.group_packed_windows(group, window_wires, keep=keep, lanes=lanes):
        for l, v in views.items():
            out.setdefault(l, []).append((w0, wn, v.copy()))
    return out, calc.group_lanes


def check_group_against_single(calc, group, window_wires, keep, expect_lanes, lanes=None, cache=None):
    """every lane's every window of the group emission == calc.packed_windows(64 * group + lane, same window, keep), byte for byte; -> the windows per lane.
    cache: a dict that keeps the single path's windows per (witness, form, window size in effect) -- the reference is computed once: a payload that fits the default
    window is ONE window whether the caller asks for the default or for the whole payload"""
    got, used = group_windows(calc, group, window_wires, keep, lanes)
    total = calc.nwitness if keep is None else len(keep)
    same = window_wires or GROUP_DEFAULT_WINDOW          # the single path's default is another (8 Mi wires): it is asked for the group path's window size
    in_effect = min(same, total)
    assert used == expect_lanes and sorted(got) == [l for l in range(64) if (expect_lanes >> l) & 1], (hex(used), hex(expect_lanes), sorted(got))
    for l, wins in got.items():
        key = (64 * group + l, keep is None, in_effect)
        want = cache.get(key) if cache is not None else None
        if want is None:
            want = single_windows(calc, 64 * group + l, same, keep)
            if cache is not None:
                cache[key] = want
        assert [(a, b, c.size) for a, b, c in wins] == [(a, b, c.size) for a, b, c in want], (group, l, window_wires)
        for (w0, wn, g), (_, _, s) in zip(wins, want):
            assert np.array_equal(g, s), (group, l, window_wires, w0, int(np.nonzero(g != s)[0][0]))
    return got


def check_lane_against_oracle(main, inp, wins, keep):
    ref = O.run(main, inp).witness_numpy().reshape(-1, 32)
    want = ref if keep is None else ref[keep]
    pos = 0
    for w0, wn, g in wins:
        assert w0 == pos and np.array_equal(g, PF.encode(want[w0:w0 + wn], first_wire=w0)), (main, w0, wn)
        pos += wn
    assert pos == want.shape[0]


def check_states(calc, keep):
    """masks, refusals and the kind rules (Spend batch: witness BAD failed, group 1 has 6 witnesses)"""
    lib, by = calc.lib, ctypes.byref
    used, w0, wn, nb1, p1 = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_void_p()
    p, nb = (ctypes.c_void_p * 64)(), (ctypes.c_uint64 * 64)()
    # an explicit mask that names the failed witness, or one beyond the batch, is refused like the single-witness paths refuse it
    assert lib.pob_emit_begin_group_packed(calc.h, 0, 1 << BAD, None, 0, 0, by(used)) == E_STATE
    assert lib.pob_emit_begin_group_packed(calc.h, 1, 1 << 6, None, 0, 0, by(used)) == E_STATE
    assert lib.pob_emit_begin_group_packed(calc.h, 2, 0, None, 0, 0, by(used)) == E_STATE      # no such group in a batch of 70
    # a mask of two lanes: the others come back as NULL, 0 and cost no PCIe bytes
    two = (1 << 3) | (1 << 40)
    got, m = group_windows(calc, 0, 100_000, keep, lanes=two)
    assert m == two and sorted(got) == [3, 40]
    assert lib.pob_emit_begin_group_packed(calc.h, 0, two, None, 0, 100_000, by(used)) == 0 and used.value == two
    assert lib.pob_emit_next_group_packed(calc.h, p, nb, by(w0), by(wn)) == 0 and wn.value == 100_000
    assert [l for l in range(64) if p[l]] == [3, 40] and all(nb[l] == 0 for l in range(64) if l not in (3, 40))
    # kind rules: the single-witness nexts after a group begin, the group next after a packed begin
    assert lib.pob_emit_next(calc.h, by(p1), by(w0), by(wn)) == E_STATE
    assert lib.pob_emit_next_packed(calc.h, by(p1), by(nb1), by(w0), by(wn)) == E_STATE
    assert lib.pob_emit_next_group_packed(calc.h, p, nb, by(w0), by(wn)) == 0 and w0.value == 100_000        # ... and the group emission goes on
    assert lib.pob_emit_begin_packed(calc.h, 0, None, 0, 100_000) == 0
    assert lib.pob_emit_next_group_packed(calc.h, p, nb, by(w0), by(wn)) == E_STATE
    assert lib.pob_emit_next_packed(calc.h, by(p1), by(nb1), by(w0), by(wn)) == 0 and wn.value == 100_000
    # a window pre-made by pob_emit_queue for the packed kind is not used by a group begin, and the group's windows are right behind it
    calc.emit_queue(3)
    for _ in calc.packed_windows(0, 100_000):
        pass
    got2, _ = group_windows(calc, 0, 100_000, None, lanes=two)
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(got2[3], single_windows(calc, 3, 100_000, None)))
    # the self-check of group emissions is out of scope: refused while it is on
    calc.emit_selfcheck(True)
    assert lib.pob_emit_begin_group_packed(calc.h, 0, 0, None, 0, 0, by(used)) == E_STATE
    calc.emit_selfcheck(False)
    # exactly the two windows' bytes cross: the measurement's count against the format's formula
    for kp in (None, keep):
        want = sum(v.size for l in (3, 40) for _, _, v in single_windows(calc, l, 100_000, kp))
        sizes = 0
        for l in (3, 40):
            vals = calc.witness_payload_packed(l, keep=kp).reshape(-1, 32)
            sizes += sum(PF.packed_size(*PF.counts_of(vals[a:a + 100_000])) for a in range(0, vals.shape[0], 100_000))
        out = np.empty(32 * 100_000, dtype=np.uint8)
        s0, s1, d2h = calc.emit_throughput_group(0, 1, 100_000, keep=kp, lanes=two, out=out)
        assert d2h == sizes == want and s0 > 0 and s1 > 0, (d2h, sizes, want)


def check_wtns(calc, group, lanes, keep, tmp_path):
    paths = {l: str(tmp_path / f"g{group}_{l}.wtns") for l in range(64)}
    mask = calc.write_wtns_group(group, paths, keep=keep, lanes=lanes)
    ref = str(tmp_path / "single.wtns")
    for l in range(64):
        if not (mask >> l) & 1:
            continue
        if keep is None:
            calc.write_wtns(64 * group + l, ref)
        else:
            calc.write_wtns_reduced(64 * group + l, ref, keep)
        with open(paths[l], "rb") as fa, open(ref, "rb") as fb:
            assert fa.read() == fb.read(), (group, l)
    return mask
