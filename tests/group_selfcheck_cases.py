"""Shared by the tests of the group emission's self-check (CPU shim and GPU).  The reference for every expectation is the single-witness checked packed emission of the
same library, which existing tests pin: emit_selfcheck(True), packed_windows(64 * group + lane, same window, same keep), emit_selfcheck_result() -- never the group path."""
import ctypes

import numpy as np

from tests import group_emit_cases as GC

E_STATE = GC.E_STATE
NONE = 0xFFFFFFFF


def single_result(calc, idx, win, keep, cache=None):
    """the single path's verdict for witness idx at this window and map (the group path's default window is asked for explicitly: the single path's default is another)"""
    key = (idx, None if keep is None else len(keep), win)
    if cache is not None and key in cache:
        return cache[key]
    calc.emit_selfcheck(True)
    try:
        for _ in calc.packed_windows(idx, win or GC.GROUP_DEFAULT_WINDOW, keep=keep):
            pass
        r = calc.emit_selfcheck_result()
    finally:
        calc.emit_selfcheck(False)
    if cache is not None:
        cache[key] = r
    return r


def group_result(calc, group, win, keep, lanes=None):
    """one checked group emission -> ({lane: windows}, the mask used, the verdicts)"""
    calc.emit_group_selfcheck(True)
    try:
        got, used = GC.group_windows(calc, group, win, keep, lanes)
        return got, used, calc.emit_group_selfcheck_result()
    finally:
        calc.emit_group_selfcheck(False)


def mask_of(lanes):
    return sum(1 << l for l in lanes)


def assert_same_windows(a, b):
    assert sorted(a) == sorted(b)
    for l in a:
        assert [(w0, wn, v.size) for w0, wn, v in a[l]] == [(w0, wn, v.size) for w0, wn, v in b[l]], l
        for (w0, _, x), (_, _, y) in zip(a[l], b[l]):
            assert np.array_equal(x, y), (l, w0)


def check_clean(calc, group, lanes, expect_mask, win, keep, ref_idx, cache=None):
    """a clean group emission: every selected lane None, checked / skipped those of the single path for witness ref_idx, and the windows byte for byte those
    of the same emission with the switch off; -> (the windows, the verdicts)"""
    plain, used0 = GC.group_windows(calc, group, win, keep, lanes)
    got, used, r = group_result(calc, group, win, keep, lanes)
    assert used == used0 == expect_mask == r["lanes"], (hex(used), hex(expect_mask), r)
    assert r["first_bad_wire"] == {l: None for l in range(64) if (expect_mask >> l) & 1}, r
    want = single_result(calc, ref_idx, win, keep, cache)
    print(f"group {group} window {win} {'O0' if keep is None else 'reduced'}: group {r['checked']} checked / {r['skipped']} skipped, single {want}")
    assert want["first_bad_wire"] is None and (r["checked"], r["skipped"]) == (want["checked"], want["skipped"]) and r["checked"] + r["skipped"] > 0, (r, want)
    assert_same_windows(got, plain)
    return got, r


def check_pokes(calc, group, lanes, expect_mask, poked, win, keep):
    """KeccakBytes.inLen poked in the lanes `poked`: exactly those are flagged, each at the single path's wire for that witness; clean again once the pokes are undone"""
    cls, idx, wire = calc.debug_ref("kb.inLen", 0)
    for l in poked:
        calc.poke(cls, idx, l, 1, group=group)
    try:
        _, used, r = group_result(calc, group, win, keep, lanes)
        want = {l: single_result(calc, 64 * group + l, win, keep)["first_bad_wire"] for l in poked}
    finally:
        for l in poked:
            calc.poke(cls, idx, l, 1, group=group)
    print(f"pokes in lanes {poked} of group {group}, window {win}, {'O0' if keep is None else 'reduced'}: group {r['first_bad_wire']}, single {want}")
    assert used == expect_mask and all(w is not None and w > wire for w in want.values()), (want, wire)
    assert r["first_bad_wire"] == {l: want.get(l) for l in range(64) if (expect_mask >> l) & 1}, (r, want)
    _, _, r = group_result(calc, group, win, keep, lanes)
    assert all(w is None for w in r["first_bad_wire"].values()), r


def z_wires(s):
    """the wires of an IsZero word, lowest first"""
    w = int(s) & 0x7FFFFFFF
    return list(range(w - 3, w + 3)) if int(s) >> 31 else [w, w + 1, w + 2]


def pick_z_sites(z):
    """indices into the IsZero table: first, middle, last, one bare IsZero and one IsEqual child (where the table has both)"""
    picks = [0, len(z) // 2, len(z) - 1]
    child = np.nonzero(z >> 31)[0]
    bare = np.nonzero((z >> 31) == 0)[0]
    for arr in (bare, child):
        extra = [int(i) for i in arr if int(i) not in picks]
        if extra:
            picks.append(extra[len(extra) // 3])
    return picks


def value_lookup(calc, wins):
    """(lane, wire) -> the 32 canonical bytes a group emission's windows hold for that O0 wire (windows are expanded on demand and kept)"""
    cache = {}

    def value(l, wire):
        k = next(i for i, (w0, wn, _) in enumerate(wins[l]) if w0 <= wire < w0 + wn)
        if (l, k) not in cache:
            cache[(l, k)] = calc.unpack_window(wins[l][k][2]).reshape(-1, 32)
        return cache[(l, k)][wire - wins[l][k][0]]
    return value


def nonzero_operand_lane(value, z, i, lanes, taken, win=0):
    """a lane not in `taken` in which site i's operand `in` is not zero.  in * inv === 1 - out and in * out === 0 hold for ANY inv when in = 0 (out = 1): a corrupted
    inv can only be seen by a witness whose operand is not zero.  None also for a site that straddles two windows of `win` wires (it is skipped, not evaluated)"""
    ws, w = z_wires(z[i]), int(z[i]) & 0x7FFFFFFF
    if win and ws[0] // win != ws[-1] // win:
        return None
    for l in lanes:
        if l not in taken and value(l, w + 1).any():
            return l
    return None


def check_xor_sites(calc, group, lanes, value, picks_z, picks_c, z, cs, win=0, keep=None):
    """ONE checked emission with one corrupted value per lane, at exactly the sites named: `inv` of the IsZero sites picks_z, each in a lane whose operand is not zero --
    or, where the operand is zero in every free lane, the site's `out`, which is wrong whatever the operand (in * inv === 1 - out fails for in = 0) --, and the higher wire of
    the copy sites picks_c.  Every such lane reports exactly its site's wire -- w for an IsZero word, the higher wire for a copy pair, as the single kernels name them -- and
    every other lane nothing"""
    expect, taken = {}, set()
    for i in picks_z:
        ws, w = z_wires(z[i]), int(z[i]) & 0x7FFFFFFF
        assert not win or ws[0] // win == ws[-1] // win, (i, w)          # (a site that straddles two windows is skipped: check_window_edge)
        l = nonzero_operand_lane(value, z, i, lanes, taken, win)
        armed = w + 2
        if l is None:
            l, armed = next(x for x in lanes if x not in taken), w
        calc.debug_group_emit_xor(l, armed, byte=0, mask=1)
        print(f"IsZero site {i} at wire {w}: {'inv' if armed == w + 2 else 'out (operand zero in every free lane)'} corrupted in lane {l}")
        expect[l] = w
        taken.add(l)
    for i in picks_c:
        l = next(x for x in lanes if x not in taken)
        calc.debug_group_emit_xor(l, int(cs[i][0]), byte=0, mask=1)
        expect[l] = int(cs[i][0])
        taken.add(l)
    assert len(taken) < len(lanes)                      # (at least one lane stays untouched)
    _, used, r = group_result(calc, group, win, keep, lanes)
    print(f"xor at sites z{picks_z} c{picks_c}: expected {expect}, got {r['first_bad_wire']}")
    assert used == mask_of(lanes) and r["first_bad_wire"] == {l: expect.get(l) for l in lanes}, (r, expect)
    _, _, r = group_result(calc, group, win, keep, lanes)            # an armed xor does not outlive one emission
    assert all(w is None for w in r["first_bad_wire"].values()), r


def straddling_z_site(z, win):
    """index of an IsZero word whose wires lie on both sides of a window boundary, None if the table has none"""
    for i, s in enumerate(z):
        ws = z_wires(s)
        if ws[0] // win != ws[-1] // win:
            return i
    return None


def check_window_edge(calc, group, lanes, value, whole, z, cs, win, cache=None):
    """a site whose wires straddle a boundary of windows of `win` wires: its corruption is NOT reported and it is counted as skipped, both as in the single path (the same
    counts, which check_clean compares for every case; here: against the whole payload in one window, where the corruption IS reported)"""
    i = straddling_z_site(z, win)
    if i is not None:
        l = nonzero_operand_lane(value, z, i, lanes, set())
        wire, named = (int(z[i]) & 0x7FFFFFFF) + 2, int(z[i]) & 0x7FFFFFFF
    else:                                               # no IsZero word straddles: a copy pair whose lower wire lies in an earlier window
        i = next(k for k, (hi, lo) in enumerate(cs) if int(hi) // win != int(lo) // win and not np.any((z & 0x7FFFFFFF) == hi) and not np.any((z & 0x7FFFFFFF) - 3 == hi))
        l, wire, named = lanes[0], int(cs[i][0]), int(cs[i][0])
    assert l is not None
    calc.debug_group_emit_xor(l, wire, byte=0, mask=1)
    _, _, r_win = group_result(calc, group, win, None, lanes)
    calc.debug_group_emit_xor(l, wire, byte=0, mask=1)
    _, _, r_whole = group_result(calc, group, whole, None, lanes)
    want = single_result(calc, 64 * group + lanes[0], win, None, cache)
    print(f"straddling site at wire {named}: windows of {win}: {r_win}; one window: {r_whole['first_bad_wire']}")
    assert all(w is None for w in r_win["first_bad_wire"].values()), r_win
    assert r_whole["first_bad_wire"] == {x: (named if x == l else None) for x in lanes}, r_whole
    assert r_win["skipped"] == want["skipped"] > r_whole["skipped"] and r_win["checked"] == want["checked"], (r_win, r_whole, want)


def kept_out_site(z, keep, alias):
    """an IsZero word that is on the reduced lists under this alias map (pob_emit_selfcheck_alias: alias[w] = the kept wire that stands for w, negative = a constant):
    -> the kept wire that stands for its `out`, which is the site's first listed wire"""
    kept = np.zeros(alias.size, dtype=bool)
    kept[keep] = True
    rep_ok = (alias >= 0) & kept[np.maximum(alias, 0)] | ((alias < 0) & (alias != -(1 << 31)))      # a kept representative, or a constant that fits
    for s in z:
        ws, w = z_wires(s), int(s) & 0x7FFFFFFF
        if alias[w] >= 0 and kept[alias[w]] and all(rep_ok[x] for x in ws):
            return int(alias[w])
    return None


def check_reduced_out(calc, group, lanes, z, keep, alias, win=0):
    """reduced form: one site's kept `out` wire corrupted in one lane (out is wrong whatever the operand: in * out === 0 fails for in != 0, in * inv === 1 - out for in = 0);
    the lane reports the site's first listed wire"""
    w = kept_out_site(z, keep, alias)
    assert w is not None
    calc.debug_group_emit_xor(lanes[1], w, byte=0, mask=1)
    _, _, r = group_result(calc, group, win, keep, lanes)
    print(f"reduced form, out wire {w} corrupted in lane {lanes[1]}: {r['first_bad_wire']}")
    assert r["first_bad_wire"] == {l: (w if l == lanes[1] else None) for l in lanes}, r


def check_states(calc, keep, fresh):
    """fresh: no checked group emission has run on this calculator yet"""
    lib, by = calc.lib, ctypes.byref
    m, c, s, used, w0, wn = (ctypes.c_uint64() for _ in range(6))
    bad = (ctypes.c_uint32 * 64)()
    p, nb = (ctypes.c_void_p * 64)(), (ctypes.c_uint64 * 64)()
    if fresh:                                           # before any checked group emission -- an unchecked one does not count
        assert lib.pob_emit_group_selfcheck_result(calc.h, by(m), by(c), by(s), bad) == E_STATE
        GC.group_windows(calc, 1, 0, None, [0])
        assert lib.pob_emit_group_selfcheck_result(calc.h, by(m), by(c), by(s), bad) == E_STATE
    # mid-emission: windows are made ahead of the caller
    calc.emit_group_selfcheck(True)
    assert lib.pob_emit_begin_group_packed(calc.h, 1, 0b11, None, 0, 100_000, by(used)) == 0
    assert lib.pob_emit_group_selfcheck_result(calc.h, by(m), by(c), by(s), bad) == E_STATE
    while True:
        assert lib.pob_emit_next_group_packed(calc.h, p, nb, by(w0), by(wn)) == 0
        if wn.value == 0:
            break
        assert lib.pob_emit_group_selfcheck_result(calc.h, by(m), by(c), by(s), bad) == E_STATE
    assert lib.pob_emit_group_selfcheck_result(calc.h, by(m), by(c), by(s), bad) == 0 and m.value == 0b11 and list(bad) == [NONE] * 64 and c.value > 0
    # a checked emission abandoned mid-way, then an unchecked one: there is no complete checked emission to report (its partial verdicts are not handed out)
    assert lib.pob_emit_begin_group_packed(calc.h, 1, 0b11, None, 0, 100_000, by(used)) == 0
    assert lib.pob_emit_next_group_packed(calc.h, p, nb, by(w0), by(wn)) == 0 and wn.value == 100_000
    calc.emit_group_selfcheck(False)
    GC.group_windows(calc, 1, 0, None, [0])
    assert lib.pob_emit_group_selfcheck_result(calc.h, by(m), by(c), by(s), bad) == E_STATE
    _, _, r = group_result(calc, 1, 100_000, None, [0, 1])            # ... and a complete one is reported again, also behind a later unchecked emission
    GC.group_windows(calc, 1, 0, None, [0])
    assert calc.emit_group_selfcheck_result() == r and r["lanes"] == 0b11
    # the single-witness switch keeps its refusal, whatever the group switch says
    calc.emit_selfcheck(True)
    for on in (True, False):
        calc.emit_group_selfcheck(on)
        assert lib.pob_emit_begin_group_packed(calc.h, 0, 0, None, 0, 0, by(used)) == E_STATE
    calc.emit_selfcheck(False)
    # an armed xor does not outlive one emission: it is spent by the next group emission, checked or not
    calc.emit_group_selfcheck(False)
    z = calc.debug_selfcheck_sites()[0]
    calc.debug_group_emit_xor(0, int(z[0]) & 0x7FFFFFFF, byte=0, mask=1)
    GC.group_windows(calc, 1, 0, None, [0, 1])
    _, _, r = group_result(calc, 1, 0, None, [0, 1])
    assert r["first_bad_wire"] == {0: None, 1: None}, r
    with np.testing.assert_raises(RuntimeError):        # lane, byte and wire are validated, and an emission takes at most 16 entries
        calc.debug_group_emit_xor(64, 0)
    with np.testing.assert_raises(RuntimeError):
        calc.debug_group_emit_xor(0, 0, byte=32)
    with np.testing.assert_raises(RuntimeError):
        calc.debug_group_emit_xor(0, calc.nwitness)
    for _ in range(16):
        calc.debug_group_emit_xor(1, 0, byte=0, mask=0)
    with np.testing.assert_raises(RuntimeError):
        calc.debug_group_emit_xor(1, 0, byte=0, mask=0)
    GC.group_windows(calc, 1, 0, None, [0])            # (spends the 16 entries: a mask of 0 changes nothing)
