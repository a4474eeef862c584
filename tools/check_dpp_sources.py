"""The back substitution (csrc/uvs_solve_kernel.h: trsv_fmac_row_lane) issues v_fmac_f64_dpp from inline assembly, which the compiler's hazard recognizer
does not see: a DPP operand must not be read within two wait states of the VALU instruction that wrote it.  The source provides them once per x_k
(trsv_dpp_source); this script checks the emitted ISA: for every such instruction, no VALU write of its DPP source in the two wait states before it.

usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -mllvm -disable-machine-licm -S --cuda-device-only uv-slam_amd/csrc/uvs_solve512.hip -o /tmp/s512.s
       python tools/check_dpp_sources.py /tmp/s512.s        (likewise uvs_solver.hip and uvs_solve_dstep256.hip: the three units that instantiate the kernel)"""
import re
import sys


def regs(tok):
    tok = tok.strip().rstrip(",")
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m: return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def check(path):
    ins = [l.strip() for l in open(path)]
    ins = [l for l in ins if l and not l.startswith((";", ".", "//")) and not l.endswith(":")]
    n = bad = 0
    for i, l in enumerate(ins):
        if not l.startswith("v_fmac_f64_dpp"): continue
        n += 1
        src = regs(l.split(None, 1)[1].split(",")[1])
        ws, j = 0, i - 1
        while ws < 2 and j >= 0:
            p = ins[j]; op = p.split()[0]; j -= 1
            if op == "s_nop": ws += int(p.split()[1]) + 1; continue
            ops = p.split(None, 1)[1].split(",") if len(p.split(None, 1)) > 1 else []
            w = regs(ops[0]) if ops else set()
            if "permlane" in op and "swap" in op and len(ops) > 1: w |= regs(ops[1])      # a swap writes both of its operands
            if op.startswith("v_") and (w & src):
                bad += 1; print(f"{path}: {p}  ->  {l}")
            ws += 1
    print(f"{path}: {n} v_fmac_f64_dpp, {bad} with a write of the DPP source less than two wait states before")
    return n, bad


if __name__ == "__main__":
    res = [check(p) for p in sys.argv[1:]]
    sys.exit(0 if res and all(n > 0 and bad == 0 for n, bad in res) else 1)
