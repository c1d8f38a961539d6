#!/usr/bin/env python3
"""What the audit (pob_set_audit) costs inside the service loop, measured on ONE box.

  (i)  --driver --parent LIB: the driver's command (bench.py --gpus 1 --steps 20 --warmup 5) on the parent commit's build (LIB, loaded through POB_LIB_PATH) and on this
       tree's with the audit off: PAIRS interleaved pairs, one process per run, the side that goes first alternating per pair; medians and ranges.
  (ii) --loop: this tree's library, 12 calculators in flight, batch 1 024 of the production instantiation, riding (pob_set_inorder(h, 7)): ms per step for audit off,
       set_audit(1), set_audit(2), set_audit(16, period=16) and set_audit(16) -- ROUNDS interleaved rounds in one process, medians -- and, with --separate, the loop whose
       evaluation does not ride (pob_set_inorder(h, 3): bench.py's separate_evaluation_pass).

    python tools/audit_cost.py --loop --separate --driver --parent /path/to/parent/libpob_hip.so > profiles/audit_cost.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("audit off", 0, 1), ("set_audit(1)", 1, 1), ("set_audit(2)", 2, 1), ("set_audit(16, period=16)", 16, 16), ("set_audit(16)", 16, 1)]


def driver(parent: str, pairs: int, steps: int, warmup: int):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    ms = {"parent": [], "new": []}
    print(f"(i) bench.py --gpus 1 --steps {steps} --warmup {warmup}: the parent commit's library against this one (audit off), {pairs} interleaved pairs, one process per run")
    for r in range(pairs):
        order = ("parent", "new") if r % 2 == 0 else ("new", "parent")
        for side in order:
            env = dict(os.environ)
            env.pop("POB_LIB_PATH", None)
            if side == "parent":
                env["POB_LIB_PATH"] = os.path.abspath(parent)
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            line = next((l for l in out.stdout.splitlines() if l.startswith("{")), None)
            if out.returncode != 0 or line is None:
                print(f"  pair {r + 1} {side}: bench.py failed (exit {out.returncode}): {out.stderr[-400:]}")
                return 1
            d = json.loads(line)
            ms[side].append(float(d["ms_per_step"]))
            print(f"  pair {r + 1} {side:6s} {d['value']:>10.0f} witnesses/s ({d['ms_per_step']:.3f} ms per step)", flush=True)
    p, n = ms["parent"], ms["new"]
    overlap = max(min(p), min(n)) <= min(max(p), max(n))
    print(f"  parent {min(p):.3f}-{max(p):.3f} ms (median {statistics.median(p):.3f}); this library, audit off {min(n):.3f}-{max(n):.3f} ms (median {statistics.median(n):.3f}): "
          f"{(statistics.median(n) / statistics.median(p) - 1) * 100:+.1f} % per step at the medians; the ranges {'overlap' if overlap else 'do NOT overlap'}")
    return 0


def loop(rounds: int, steps: int, depth: int, batch: int, separate: bool):
    import numpy as np
    import bench as BM
    from proof_of_burn_amd import PinnedInputs, inputs as gen
    args = BM.parse_args(["--gpus", "1", "--batch", str(batch)])
    job = BM.Job(args)
    B = job.B
    groups = (B + 63) // 64
    batches = [gen.synthetic_batch(B, depth=10, seed=0xB0B, distinct_keys=16, first=b * B) for b in range(4)]
    expect = [BM._expect(np, bt) for bt in batches]
    loops = [("riding", BM.ServiceLoop(job, BM.MAIN, depth, True, 3))]
    if separate:
        loops.append(("separate", BM.ServiceLoop(job, BM.MAIN, depth, True, 1)))
    pinned = [PinnedInputs(loops[0][1].calcs[0], B) for _ in batches]
    for pin, bt in zip(pinned, batches):
        loops[0][1].calcs[0].pack_json([json.dumps(i).encode() for i in bt.inputs], out=pin)
    for _, lp in loops:
        lp.set_inputs(pinned, expect)
        lp.run(depth + 2)
    job.fence()
    points = [("riding", s) for s in SETTINGS] + ([("separate", ("evaluation as a pass of its own (pob_set_inorder(h, 3))", 0, 1))] if separate else [])
    ms = {p[1][0]: [] for p in points}
    share = {}
    print(f"(ii) service loop, {depth} calculators in flight, batch {B} ({groups} groups) of {BM.MAIN}, {steps} timed steps per point, {rounds} interleaved rounds in one process; ms per step")
    for r in range(rounds):
        row = []
        for which, (label, g, period) in points:
            lp = dict(loops)[which]
            for c in lp.calcs:
                c.set_audit(g, period)
            s, _, _ = lp.timed(steps, depth + 2, k0=0)
            ms[label].append(s / steps * 1e3)
            row.append(f"{s / steps * 1e3:.3f}")
            if which == "riding":                                    # (steady state: one window of min(g, groups) groups every `period` checks of a calculator)
                share[label] = min(g, groups) / groups / period
        print(f"  round {r + 1}: " + "  ".join(row), flush=True)
    base = statistics.median(ms["audit off"])
    for _, (label, g, period) in points:
        v = ms[label]
        sh = f", {share[label] * 100:5.1f} % of the witnesses independently evaluated per step" if label in share else ", every witness independently evaluated"
        print(f"  {label:58s} median {statistics.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f}), {statistics.median(v) - base:+.3f} ms against audit off{sh}")
    for _, lp in loops:
        lp.close()
    for pin in pinned:
        pin.free()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--driver", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--separate", action="store_true", help="--loop: also the loop whose evaluation is a pass of its own")
    ap.add_argument("--parent", default=None, help="--driver: the parent commit's libpob_hip.so")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=192, help="--loop: timed steps per point; a multiple of depth x the longest period (12 x 16), so that the timed region holds whole periods of every calculator")
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--batch", type=int, default=1024)
    a = ap.parse_args()
    rc = 0
    if a.loop:
        rc |= loop(a.rounds, a.steps, a.depth, a.batch, a.separate)
    if a.driver:
        if not a.parent or not os.path.exists(a.parent):
            ap.error("--driver needs --parent LIB")
        rc |= driver(a.parent, a.pairs, 20, 5)
    return rc


if __name__ == "__main__":
    sys.exit(main())
