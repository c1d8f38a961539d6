#!/usr/bin/env python3
"""Loops of one kernel in a gfx950 code object and the v_mad_u64_u32 (or any opcode) count of each, from the disassembly (no GPU needed): a loop is a
backward branch, its body the instructions from the branch target to the branch.  Prints the nest of loops with their own and their inner counts and the
kernel's total, for "disassembly x trip counts" estimates (profiles/pos4lane_ab.txt).

    python tools/isa_loop_mads.py proof_of_burn_amd/csrc/g_gen_poswide.o _Z11k_pos_chainILb1ELb0EEv5GArgs5KArgsjj [v_mad_u64_u32]
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def disasm(obj):
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "fb"), os.path.join(td, "co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        return subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout


def main(obj, kernel, op="v_mad_u64_u32"):
    ins, on = [], False
    for line in disasm(obj).splitlines():
        if line.endswith(">:"):
            on = line.split("<", 1)[1][:-2] == kernel
            continue
        m = re.match(r"\s+(\S+)(.*)//\s*([0-9A-Fa-f]+):", line)
        if on and m:
            tgt = re.search(r"<" + re.escape(kernel) + r"\+0x([0-9a-f]+)>", line)
            ins.append((int(m.group(3), 16), m.group(1), int(tgt.group(1), 16) if tgt else None))
    base = ins[0][0]
    addr = [a - base for a, _, _ in ins]
    loops = sorted({(t, addr[i]) for i, (_, o, t) in enumerate(ins) if o.startswith("s_cbranch") or o == "s_branch" if t is not None and t <= addr[i]})
    count = lambda lo, hi: sum(1 for a, (_, o, _) in zip(addr, ins) if lo <= a <= hi and o == op)
    print(f"{kernel}: {count(0, addr[-1])} x {op} in all, {len(loops)} loops")
    for lo, hi in loops:
        inner = [(l2, h2) for l2, h2 in loops if (l2, h2) != (lo, hi) and lo <= l2 and h2 <= hi]
        depth = sum(1 for l2, h2 in loops if (l2, h2) != (lo, hi) and l2 <= lo and hi <= h2)
        own = count(lo, hi) - sum(count(l2, h2) for l2, h2 in inner if not any((l3, h3) != (l2, h2) and l3 <= l2 and h2 <= h3 for l3, h3 in inner))
        print(f"{'  ' * depth}loop +0x{lo:x}..+0x{hi:x}: {count(lo, hi)} ({own} outside its inner loops)")


if __name__ == "__main__":
    main(*sys.argv[1:])
