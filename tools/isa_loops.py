#!/usr/bin/env python3
"""Loop map of one structured-kernel instance in the built library: disassembles the gfx950 code
object (llvm-objdump --offloading into a temp dir, then -d), finds the instance's function, and
lists every backward branch (a loop: target .. branch) with its instruction count and the scratch,
global and LDS memory instructions inside it -- where the register spills land relative to the
ADMM iteration loop.  Usage: python tools/isa_loops.py [--sweep-steps] '<256, 3, 3, 1, 39' [lib.so] [min_len]
--sweep-steps: for every step of the matrix-instruction stage sweeps (the v_mfma_f64_4x4x4 of the
raised-priority regions) also print what stands between the instruction and the DPP moves that read its
result, with the s_nop wait states among it, and what stands between the step's add and the next
matrix instruction -- the instructions that are issued on the serial chain without belonging to it."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
argv = [a for a in sys.argv[1:] if a != "--sweep-steps"]
sweep_steps = "--sweep-steps" in sys.argv[1:]
want = argv[0] if len(argv) > 0 else "<256, 3, 3, 1, 39"
lib = os.path.abspath(argv[1] if len(argv) > 1 else os.path.join(os.path.dirname(__file__), "..",
                                                                 "intent-mpc_amd", "lib", "libimpc_qp.so"))
min_len = int(argv[2]) if len(argv) > 2 else 200
tmp = tempfile.mkdtemp()
try:
    src = os.path.join(tmp, os.path.basename(lib))
    shutil.copy(lib, src)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", src], check=True, capture_output=True, cwd=tmp)
    co = sorted(f for f in os.listdir(tmp) if "gfx950" in f)
    dis = "".join(subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--demangle", "--no-show-raw-insn",
                                  os.path.join(tmp, c)], check=True, capture_output=True, text=True).stdout
                  for c in co)
finally:
    shutil.rmtree(tmp)

# functions: "<addr> <name>:" headers; instructions: "  <ws><mnemonic> ... // <addr>:" or "addr: insn"
funcs, cur = {}, None
for ln in dis.splitlines():
    m = re.match(r"^([0-9a-f]+) <(.*)>:$", ln)
    if m:
        cur = m.group(2)
        funcs[cur] = []
        continue
    if cur is None:
        continue
    m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", ln)
    if m:
        funcs[cur].append((int(m.group(2), 16), m.group(1)))
names = [n for n in funcs if "k_mpc_wave_group" in n and want in n]
if not names:
    sys.exit(f"no k_mpc_wave_group instance matching {want!r}")
name = names[0]
ins = funcs[name]
print(name[:160], len(ins), "instructions")
pos = {a: i for i, (a, _) in enumerate(ins)}
loops = []
for i, (a, t) in enumerate(ins):
    m = re.match(r"s_(cbranch_\w+|branch)\s+(-?\d+)", t)
    if not m:
        continue
    imm = int(m.group(2))
    if imm > 32767:
        imm -= 65536
    ta = a + 4 + 4 * imm  # SOPP simm16: dwords after the next instruction
    if ta < a and ta in pos:
        loops.append((pos[ta], i))


def kinds(lo, hi):
    c = {"scratch_ld": 0, "scratch_st": 0, "global_ld": 0, "global_st": 0, "ds": 0, "valu": 0, "salu": 0,
         "s_waitcnt": 0, "s_barrier": 0}
    for _, t in ins[lo:hi + 1]:
        op = t.split()[0]
        if op.startswith("scratch_load") or op.startswith("buffer_load"):
            c["scratch_ld"] += 1
        elif op.startswith("scratch_store") or op.startswith("buffer_store"):
            c["scratch_st"] += 1
        elif op.startswith("global_load") or op.startswith("flat_load"):
            c["global_ld"] += 1
        elif op.startswith(("global_store", "global_atomic", "flat_store", "flat_atomic")):
            c["global_st"] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
        elif op.startswith("s_waitcnt"):
            c["s_waitcnt"] += 1
        elif op.startswith("s_barrier"):
            c["s_barrier"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    return c


def sweep_step_lines(text):
    """Per step of a sweep (text: the region's instructions): the instructions between the matrix
    instruction and the first DPP move, and between the add behind the moves and the next one."""
    ops = [t.split()[0] for t in text]
    mf = [i for i, o in enumerate(ops) if o.startswith("v_mfma_f64_4x4x4")]

    def short(i):  # waits with their operand, everything else by mnemonic
        return text[i] if ops[i].startswith(("s_nop", "s_waitcnt")) else ops[i]

    out = []
    for n, i in enumerate(mf):
        end = mf[n + 1] if n + 1 < len(mf) else len(ops)
        dpp = next((k for k in range(i + 1, end) if ops[k].startswith("v_mov_b32_dpp")), None)
        add = None if dpp is None else next((k for k in range(dpp + 1, end) if ops[k].startswith("v_add_f64")), None)
        if add is None:
            out.append(f"  step {n:2d}: no DPP move and add behind the instruction")
            continue
        behind = [short(k) for k in range(i + 1, dpp)]
        ws = sum(int(text[k].split()[1]) + 1 for k in range(i + 1, dpp) if ops[k] == "s_nop")
        tail = [short(k) for k in range(add + 1, end)] if n + 1 < len(mf) else ["(last step)"]
        out.append(f"  step {n:2d}: behind the instruction [{', '.join(behind)}] ({ws} s_nop wait states, "
                   f"{len(behind) - sum(o.startswith('s_nop') for o in behind)} other); "
                   f"add .. next instruction [{', '.join(tail)}]")
    return out


tot = kinds(0, len(ins) - 1)
print("whole function:", tot)
# the raised-priority regions (s_setprio N > 0 .. s_setprio 0: the serial stage sweeps): a register
# reload there sits on the team's critical path
up, prio = None, []
for i, (a, t) in enumerate(ins):
    m = re.match(r"s_setprio\s+(\d+)", t)
    if not m:
        continue
    if int(m.group(1)) > 0:
        up = i
    elif up is not None:
        c = kinds(up, i)
        print(f"setprio {ins[up][0]:#x}..{a:#x} ({i - up + 1} instructions): scratch_ld {c['scratch_ld']} "
              f"scratch_st {c['scratch_st']} ds {c['ds']} valu {c['valu']}")
        if sweep_steps:
            print("\n".join(sweep_step_lines([t for _, t in ins[up:i + 1]])))
        prio.append((up, i))
        up = None
# the ADMM iteration loop: the innermost loop around each raised-priority region
shown = set()
for plo, phi in prio:
    around = [(lo, hi) for lo, hi in loops if lo <= plo and phi <= hi]
    if around:
        lo, hi = min(around, key=lambda x: x[1] - x[0])
        if (lo, hi) in shown:
            continue
        shown.add((lo, hi))
        print(f"iteration loop {ins[lo][0]:#x}..{ins[hi][0]:#x} ({hi - lo + 1} instructions):", kinds(lo, hi))
for lo, hi in sorted(loops, key=lambda x: x[1] - x[0], reverse=True):
    if hi - lo < min_len:
        continue
    print(f"loop {ins[lo][0]:#x}..{ins[hi][0]:#x} ({hi - lo + 1} instructions):", kinds(lo, hi))
