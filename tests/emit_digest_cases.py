"""Shared by the emission digest tests (CPU shim and GPU): every emission path of the library on the Spend(31) batch of group_emit_cases (70 witnesses, witness 9
failing), reduced to sha256 digests and compared with tests/golden/emit_digests.json -- the bytes an earlier commit of this library handed out for the same calls.
The digest of an emission is one sha256 over its windows in order: first_wire (u64 LE), n_wires (u64 LE), then the window's bytes as the caller sees them (canonical
values, or the packed window).  Nothing here is compared with an oracle: the other emission tests do that; this one pins that a change of the emission's host code
changes no byte, no self-check count and no table.

`python -m tests.emit_digest_cases [out.json]` records the file from the CPU shim of the checkout it runs in."""
import hashlib
import json
import os
import struct
import sys

import numpy as np

from tests import group_emit_cases as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emit_digests.json")
MAIN = "Spend(31)"
WITNESSES = (0, 37, 63, 64, 69)      # group 0's first, an inner one and its last; group 1's first and the batch's last
WINDOWS = (100_000, 0)               # 27 windows with partial 64-wire blocks at their edges | the default: one window
QUEUED = (0, 3, 5)                   # emitted back to back, each announced (pob_emit_queue) while the one before it is being emitted
TWO = (1 << 3) | (1 << 40)
GROUPS = (("g0", 0, None), ("g1", 1, None), ("g0_3_40", 0, TWO))
SECTIONS = ("interleaved", "counters", "single", "single_checked", "queued", "group", "group_checked", "sites")


class _Stream:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, w0, wn, data):
        self.h.update(struct.pack("<QQ", int(w0), int(wn)))
        self.h.update(np.ascontiguousarray(data))

    def hex(self):
        return self.h.hexdigest()


def single(calc, idx, packed, keep, win, announce=None):
    """digest of one single-witness emission; announce: the witness named with pob_emit_queue once the first window is with the caller"""
    s = _Stream()
    if packed:
        for w0, wn, v in calc.packed_windows(idx, win, keep=keep):
            if w0 == 0 and announce is not None:
                calc.emit_queue(announce)
            s.add(w0, wn, v)
    else:
        for w0, v in calc.witness_windows(idx, win, keep=keep):
            if w0 == 0 and announce is not None:
                calc.emit_queue(announce)
            s.add(w0, v.size // 32, v)
    return s.hex()


def group(calc, g, keep, win, lanes):
    """{lane: digest} of one group emission"""
    out = {}
    for w0, wn, views in calc.group_packed_windows(g, win, keep=keep, lanes=lanes):
        for l, v in views.items():
            out.setdefault(l, _Stream()).add(w0, wn, v)
    return {str(l): s.hex() for l, s in sorted(out.items())}


def _single_result(calc):
    r = calc.emit_selfcheck_result()
    return [r["checked"], r["skipped"], r["first_bad_wire"]]


def _group_result(calc):
    r = calc.emit_group_selfcheck_result()
    return {"lanes": f"{r['lanes']:016x}", "checked": r["checked"], "skipped": r["skipped"], "first_bad_wire": {str(l): w for l, w in r["first_bad_wire"].items()}}


def _array_digest(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return {"words": int(a.size), "sha256": hashlib.sha256(a).hexdigest()}


def compute(calc, keep):
    """every recorded figure, from a calculator that holds the generated batch and has emitted nothing yet (the interleaved sequence comes first: it needs a handle
    whose probe cache, map, site tables and pre-made window are all still empty)"""
    forms = (("O0", None), ("reduced", keep))
    d = {}
    # one handle, five kinds of emission in a row: each finds the shared state the one before it left
    seq = [single(calc, 0, True, None, 100_000), group(calc, 0, None, 100_000, None), single(calc, 64, False, keep, 100_000)]
    calc.emit_group_selfcheck(True)
    seq.append(group(calc, 1, None, 100_000, None))
    seq.append(_group_result(calc))
    calc.emit_group_selfcheck(False)
    calc.emit_selfcheck(True)
    seq.append(single(calc, 0, False, None, 100_000))
    seq.append(_single_result(calc))
    calc.emit_selfcheck(False)
    d["interleaved"] = seq
    # the emitter's inverse paths over one whole O0 payload
    calc.emit_counters(reset=True)
    calc.witness_payload(0)
    d["counters"] = calc.emit_counters(reset=True)
    # single witness: canonical and packed, O0 and reduced, both window sizes; then the same emissions with the self-check on
    d["single"], d["single_checked"] = {}, {}
    for checked in (False, True):
        calc.emit_selfcheck(checked)
        for idx in WITNESSES:
            for packed in (False, True):
                for form, kp in forms:
                    for win in WINDOWS:
                        key = f"w{idx}/{'packed' if packed else 'canonical'}/{form}/{win}"
                        dig = single(calc, idx, packed, kp, win)
                        if checked:
                            d["single_checked"][key] = [dig] + _single_result(calc)
                        else:
                            d["single"][key] = dig
    calc.emit_selfcheck(False)
    d["queued"] = {}
    for packed in (False, True):
        for i, idx in enumerate(QUEUED):
            d["queued"][f"w{idx}/{'packed' if packed else 'canonical'}"] = single(calc, idx, packed, None, 100_000, announce=QUEUED[i + 1] if i + 1 < len(QUEUED) else None)
    # groups: every good witness of groups 0 and 1, two lanes of group 0; the group self-check off and on
    d["group"], d["group_checked"] = {}, {}
    for checked in (False, True):
        calc.emit_group_selfcheck(checked)
        for name, g, lanes in GROUPS:
            for form, kp in forms:
                for win in WINDOWS:
                    key = f"{name}/{form}/{win}"
                    dig = group(calc, g, kp, win, lanes)
                    if checked:
                        d["group_checked"][key] = {"digests": dig, "result": _group_result(calc)}
                    else:
                        d["group"][key] = dig
    calc.emit_group_selfcheck(False)
    # the site tables behind both checks (pob_debug_selfcheck_sites kinds 0..4; 3 and 4: the lists of the last checked reduced emission)
    z, m, c = calc.debug_selfcheck_sites()
    zr, mr = calc.debug_selfcheck_reduced_lists()
    d["sites"] = {str(k): _array_digest(a) for k, a in enumerate((z, m, c, zr, mr))}
    return json.loads(json.dumps(d))


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def calculator(pkg):
    """-> (calc, keep): the batch generated and evaluated, nothing emitted"""
    from proof_of_burn_amd.circuit_model import keepmap
    calc = pkg.WitnessCalculator(MAIN, max_batch=128)
    res = calc.calculate(GC.spend_batch(), check=True)
    assert [i for i, r in enumerate(res) if not r.ok] == [GC.BAD]
    keep, nw = keepmap.load(MAIN)
    assert nw == calc.nwitness
    return calc, keep


def check_section(got, section):
    want = golden()[section]
    if isinstance(want, dict):
        assert sorted(got[section]) == sorted(want)
        for key in want:
            assert got[section][key] == want[key], (section, key)
    assert got[section] == want, section


if __name__ == "__main__":
    from tests.hostsim import build as hb
    import proof_of_burn_amd
    from proof_of_burn_amd import witness as W
    W.LIB_PATH, W._lib = hb.build(), None
    calc_, keep_ = calculator(proof_of_burn_amd)
    out_ = compute(calc_, keep_)
    calc_.close()
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f_:
        json.dump(out_, f_, indent=1, sort_keys=True)
        f_.write("\n")
