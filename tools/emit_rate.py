#!/usr/bin/env python3
"""Emission rates of ONE production calculator: the O0 payload and the reduced (O1-style) one, steady state (POB_LIB_PATH selects the build).
    python tools/emit_rate.py [label]                    the canonical paths (pob_emit_measure_ex)
    python tools/emit_rate.py --packed [--pairs N] [--parent LIB]
        the packed transfer (pob_emit_measure_packed) beside the canonical one.  --parent: another build of the library (the parent commit's) measured in a second
        process that takes turns with this one, pair by pair, on the same GPU: its canonical figures are the baseline.  Prints medians and ranges.
    python tools/emit_rate.py --group [--pairs N] [--parent LIB]
        the group emission (pob_emit_measure_group: all 64 witnesses of the group in one pass) beside the single-witness packed path -- of the parent's library with
        --parent, else of this one -- taking turns; per form: ms per witness into pinned memory, with the host expansion, and D2H bytes per witness.
    python tools/emit_rate.py --group-selfcheck [--pairs N] --parent LIB
        the group emission's self-check (pob_emit_group_selfcheck): the parent's group emission, this library's with the check off and on, and the parent's 64 checked
        single-witness emissions, taking turns; medians per group, the check's cost per witness
    python tools/emit_rate.py --trace-one [--group]      ONE packed O0 production emission (--group: one group emission) and nothing else after the generation (for
                                                         rocprofv3 --kernel-trace --stats)"""
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAIN = "ProofOfBurn(16, 4, 16, 50, 31, 2, 10 ** 19, 10 ** 20)"
RED_WIN = 1 << 24


def open_calc():
    from proof_of_burn_amd import WitnessCalculator, inputs as gen
    from proof_of_burn_amd.circuit_model import keepmap
    batch = gen.synthetic_batch(64, depth=10, seed=0xB0B, distinct_keys=4)
    calc = WitnessCalculator(MAIN, max_batch=64)
    res = calc.calculate(batch.inputs, check=True)
    assert all(r.ok for r in res)
    keep, _ = keepmap.load(MAIN)
    return calc, keep


def legacy(label):
    calc, keep = open_calc()
    calc.emit_throughput(0, count=1)
    sec, nbytes = calc.emit_throughput(1, count=3)
    calc.emit_throughput(0, count=1, keep=keep, window_wires=RED_WIN)
    out = []
    for rep in range(3):
        rsec, rbytes = calc.emit_throughput(1, count=6, keep=keep, window_wires=RED_WIN)
        out.append(round(rsec / 6 * 1e3, 2))
    print(f"{label}: O0 payload {nbytes / sec / 1e9:.1f} GB/s ({sec / 3 * 1e3:.1f} ms per witness); reduced {out} ms per witness")
    calc.close()


def serve():
    """a measuring process driven over stdin / stdout: 'canon' / 'packed' / 'unpack' -> one JSON line each; every kind is warmed up before its first measurement
    (the first emission of a handle at a window size allocates the window buffers and probes)"""
    import numpy as np
    calc, keep = open_calc()
    warm, buf = set(), None
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "quit":
            break
        if cmd == "canon":
            if cmd not in warm:
                calc.emit_throughput(0, count=1); calc.emit_throughput(0, count=1, keep=keep, window_wires=RED_WIN); warm.add(cmd)
            s0, b0 = calc.emit_throughput(1, count=3)
            s1, b1 = calc.emit_throughput(1, count=6, keep=keep, window_wires=RED_WIN)
            print(json.dumps({"o0_ms": s0 / 3 * 1e3, "o0_bytes": b0 // 3, "red_ms": s1 / 6 * 1e3, "red_bytes": b1 // 6}), flush=True)
        elif cmd == "packed":
            if buf is None:
                buf = np.zeros(32 * RED_WIN, dtype=np.uint8)              # one window of either kind (O0: 8 Mi wires, reduced: 16 Mi): every window is expanded to its start
            if cmd not in warm:
                calc.emit_throughput_packed(0, 1, 0, out=buf); calc.emit_throughput_packed(0, 1, RED_WIN, keep=keep, out=buf); warm.add(cmd)
            p0, e0, d0 = calc.emit_throughput_packed(1, 3, 0, out=buf)
            p1, e1, d1 = calc.emit_throughput_packed(1, 6, RED_WIN, keep=keep, out=buf)
            print(json.dumps({"o0_pinned_ms": p0 / 3 * 1e3, "o0_expanded_ms": e0 / 3 * 1e3, "o0_d2h": d0 // 3,
                              "red_pinned_ms": p1 / 6 * 1e3, "red_expanded_ms": e1 / 6 * 1e3, "red_d2h": d1 // 6}), flush=True)
        elif cmd == "group":
            if buf is None:
                buf = np.zeros(32 * RED_WIN, dtype=np.uint8)
            if cmd not in warm:
                calc.emit_throughput_group(0, 1, 0, out=buf); calc.emit_throughput_group(0, 1, 0, keep=keep, out=buf); warm.add(cmd)
            p0, e0, d0 = calc.emit_throughput_group(0, 1, 0, out=buf)
            p1, e1, d1 = calc.emit_throughput_group(0, 1, 0, keep=keep, out=buf)
            print(json.dumps({"o0_pinned_ms": p0 / 64 * 1e3, "o0_expanded_ms": e0 / 64 * 1e3, "o0_d2h": d0 // 64,
                              "red_pinned_ms": p1 / 64 * 1e3, "red_expanded_ms": e1 / 64 * 1e3, "red_d2h": d1 // 64}), flush=True)
        elif cmd in ("group_pinned", "group_checked"):               # one group of 64 into pinned memory, no host expansion; group_checked: with pob_emit_group_selfcheck on
            if cmd == "group_checked":
                calc.emit_group_selfcheck(True)
            if cmd not in warm:
                calc.emit_throughput_group(0, 1, 0); calc.emit_throughput_group(0, 1, 0, keep=keep); warm.add(cmd)
            p0, _, d0 = calc.emit_throughput_group(0, 1, 0)
            r0 = calc.emit_group_selfcheck_result() if cmd == "group_checked" else None
            p1, _, d1 = calc.emit_throughput_group(0, 1, 0, keep=keep)
            r1 = calc.emit_group_selfcheck_result() if cmd == "group_checked" else None
            if cmd == "group_checked":
                calc.emit_group_selfcheck(False)
                assert all(w is None for r in (r0, r1) for w in r["first_bad_wire"].values()) and r0["lanes"] == r1["lanes"] == (1 << 64) - 1
            print(json.dumps({"o0_ms": p0 * 1e3, "red_ms": p1 * 1e3, "o0_d2h": d0, "red_d2h": d1,
                              "o0_checked": r0 and [r0["checked"], r0["skipped"]], "red_checked": r1 and [r1["checked"], r1["skipped"]]}), flush=True)
        elif cmd == "single_checked":                                 # the only checked alternative without the group check: 64 single-witness packed emissions with pob_emit_selfcheck on
            calc.emit_selfcheck(True)
            if cmd not in warm:
                calc.emit_throughput_packed(0, 1, 4 << 20); calc.emit_throughput_packed(0, 1, 4 << 20, keep=keep); warm.add(cmd)
            p0, _, d0 = calc.emit_throughput_packed(0, 64, 4 << 20)
            r0 = calc.emit_selfcheck_result()
            p1, _, d1 = calc.emit_throughput_packed(0, 64, 4 << 20, keep=keep)
            r1 = calc.emit_selfcheck_result()
            calc.emit_selfcheck(False)
            assert r0["first_bad_wire"] is None and r1["first_bad_wire"] is None
            print(json.dumps({"o0_ms": p0 * 1e3, "red_ms": p1 * 1e3, "o0_d2h": d0, "red_d2h": d1, "o0_checked": [r0["checked"], r0["skipped"]], "red_checked": [r1["checked"], r1["skipped"]]}), flush=True)
        elif cmd == "unpack":
            from proof_of_burn_amd import witness as W
            if buf is None:
                buf = np.zeros(32 * RED_WIN, dtype=np.uint8)
            out = {}
            for name, kp, win in (("o0", None, 0), ("red", keep, RED_WIN)):
                wins = [(wn, v.copy()) for _, wn, v in calc.packed_windows(1, win, keep=kp)][:2]      # the first window holds most values that are not bits, the second is typical
                for k, (wn, pk) in enumerate(wins):
                    W.unpack_window(pk, buf)
                    ts = []
                    for _ in range(5):
                        t0 = time.perf_counter(); W.unpack_window(pk, buf); ts.append(time.perf_counter() - t0)
                    out[f"{name}_window{k}"] = {"wires": wn, "packed_bytes": int(pk.size), "ms": statistics.median(ts) * 1e3, "canonical_GBps": 32 * wn / statistics.median(ts) / 1e9}
            print(json.dumps(out), flush=True)
    calc.close()


class Proc:
    def __init__(self, lib=None):
        env = dict(os.environ)
        if lib:
            env["POB_LIB_PATH"] = os.path.abspath(lib)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        assert json.loads(self.p.stdout.readline())["ready"]

    def ask(self, cmd):
        self.p.stdin.write(cmd + "\n"); self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"the measuring process ended (exit {self.p.wait()})")
        return json.loads(line)

    def close(self):
        self.p.stdin.write("quit\n"); self.p.stdin.flush(); self.p.wait(120)


def _fmt(xs, unit="ms"):
    return f"median {statistics.median(xs):.2f} {unit} (range {min(xs):.2f} .. {max(xs):.2f}, n = {len(xs)})"


def packed(pairs, parent):
    new = Proc()
    old = Proc(parent) if parent else None
    rows = {"new_canon": [], "new_packed": [], "parent_canon": []}
    try:
        for who in (old, new):                                        # warm-up emissions of every kind, each library
            if who is not None:
                who.ask("canon")
        new.ask("packed")
        for _ in range(pairs):                                        # parent and new library take turns
            if old is not None:
                rows["parent_canon"].append(old.ask("canon"))
            rows["new_canon"].append(new.ask("canon"))
            rows["new_packed"].append(new.ask("packed"))
        unpack = new.ask("unpack")
    finally:
        for who in (old, new):
            if who is not None:
                who.close()
    print(f"{MAIN}, one calculator, 64 witnesses resident; per witness, steady state; {pairs} rounds, the libraries taking turns on one GPU")
    for form, key in (("O0 (215 907 954 wires, windows of 8 Mi)", "o0"), ("reduced (21 454 032 kept wires, windows of 16 Mi)", "red")):
        print(f"{form}:")
        if old is not None:
            print(f"  parent library, canonical into pinned memory:   {_fmt([r[key + '_ms'] for r in rows['parent_canon']])}, {rows['parent_canon'][0][key + '_bytes']} B D2H")
        print(f"  this library,   canonical into pinned memory:   {_fmt([r[key + '_ms'] for r in rows['new_canon']])}, {rows['new_canon'][0][key + '_bytes']} B D2H")
        print(f"  this library,   packed into pinned memory:      {_fmt([r[key + '_pinned_ms'] for r in rows['new_packed']])}, {rows['new_packed'][0][key + '_d2h']} B D2H")
        print(f"  this library,   packed + host expansion:        {_fmt([r[key + '_expanded_ms'] for r in rows['new_packed']])} (pob_unpack_window on the pool's default width, every window into one buffer)")
    print("host expansion alone (pob_unpack_window, pool's default width, median of 5):")
    for k, v in unpack.items():
        print(f"  {k}: {v['wires']} wires, {v['packed_bytes']} B packed -> {v['ms']:.2f} ms, {v['canonical_GBps']:.1f} GB/s of canonical bytes written")


def group(pairs, parent):
    new = Proc()
    old = Proc(parent) if parent else new
    rows = {"single": [], "group": []}
    try:
        old.ask("packed"); new.ask("group")                           # warm-up: allocations and probe passes
        for _ in range(pairs):                                        # the two paths take turns on one GPU
            rows["single"].append(old.ask("packed"))
            rows["group"].append(new.ask("group"))
    finally:
        for who in {old, new}:
            who.close()
    print(f"{MAIN}, one calculator, 64 witnesses resident; per witness; {pairs} rounds, the two paths taking turns on one GPU")
    for form, key in (("O0 (215 907 954 wires)", "o0"), ("reduced (21 454 032 kept wires)", "red")):
        print(f"{form}:")
        for name, who in ((("parent library" if parent else "this library") + ", single-witness packed path", "single"), ("this library, group emission of 64            ", "group")):
            r = rows[who]
            print(f"  {name}: into pinned memory {_fmt([x[key + '_pinned_ms'] for x in r])}; with the host expansion {_fmt([x[key + '_expanded_ms'] for x in r])}; {r[0][key + '_d2h']} B D2H")
        a, b = statistics.median(x[key + "_pinned_ms"] for x in rows["single"]), statistics.median(x[key + "_pinned_ms"] for x in rows["group"])
        print(f"  witnesses per second, group / single: {a / b:.1f} x")


def group_selfcheck(pairs, parent):
    """four legs, one production group of 64 at the group path's default window (4 Mi wires), into pinned memory: (a) the parent's library, group emission; (b) this
    library, pob_emit_group_selfcheck off; (c) on; (d) the parent's only checked alternative, 64 single-witness packed emissions with pob_emit_selfcheck on (at the same
    window size, so that the same sites straddle windows)"""
    new = Proc()
    old = Proc(parent)
    legs = (("a", old, "group_pinned"), ("b", new, "group_pinned"), ("c", new, "group_checked"), ("d", old, "single_checked"))
    rows = {k: [] for k, _, _ in legs}
    try:
        for _, who, cmd in legs:                                      # warm-up: allocations, probe and recording passes
            who.ask(cmd)
        for _ in range(pairs):                                        # the four legs take turns on one GPU
            for k, who, cmd in legs:
                rows[k].append(who.ask(cmd))
    finally:
        old.close(); new.close()
    names = {"a": "(a) parent library, group emission of 64             ", "b": "(b) this library, group emission, check off          ",
             "c": "(c) this library, group emission, check on           ", "d": "(d) parent library, 64 single emissions, check on    "}
    print(f"{MAIN}, one calculator, 64 witnesses resident; one group of 64 into pinned memory, window 4 Mi wires; {pairs} rounds, the four legs taking turns on one GPU; ms per GROUP")
    for form, key in (("O0 (215 907 954 wires)", "o0"), ("reduced (21 454 032 kept wires)", "red")):
        print(f"{form}:")
        med = {}
        for k in "abcd":
            xs = [r[key + "_ms"] for r in rows[k]]
            med[k] = statistics.median(xs)
            chk = rows[k][0][key + "_checked"]
            print(f"  {names[k]} {_fmt(xs)}; {rows[k][0][key + '_d2h']} B D2H" + (f"; per witness {chk[0]} relations checked, {chk[1]} skipped" if chk else ""))
        print(f"  cost of the check (c - b): {med['c'] - med['b']:.2f} ms per group = {(med['c'] - med['b']) / 64 * 1e3:.1f} us per witness ({(med['c'] / med['b'] - 1) * 100:+.1f} %)")
        print(f"  checked witnesses per second, (d) / (c): {med['d'] / med['c']:.1f} x")


def trace_one():
    if "--group" in sys.argv:
        calc, _ = open_calc()
        sec, _, d2h = calc.emit_throughput_group(0, 1, 0)
        print(f"one O0 group emission of 64 (first of the handle: allocation and probe pass included): {sec * 1e3:.1f} ms, {d2h} B D2H")
        calc.close()
        return
    calc, _ = open_calc()
    sec, _, d2h = calc.emit_throughput_packed(1, 1, 0)
    print(f"one packed O0 emission (first of the handle: allocation and probe pass included): {sec * 1e3:.1f} ms, {d2h} B D2H")
    calc.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    if "--serve" in a:
        serve()
    elif "--trace-one" in a:
        trace_one()
    elif "--group-selfcheck" in a:
        group_selfcheck(int(a[a.index("--pairs") + 1]) if "--pairs" in a else 7, a[a.index("--parent") + 1])
    elif "--group" in a:
        group(int(a[a.index("--pairs") + 1]) if "--pairs" in a else 7, a[a.index("--parent") + 1] if "--parent" in a else None)
    elif "--packed" in a:
        packed(int(a[a.index("--pairs") + 1]) if "--pairs" in a else 5, a[a.index("--parent") + 1] if "--parent" in a else None)
    else:
        legacy(a[0] if a else "lib")
