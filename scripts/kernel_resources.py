"""Static resources of the one-stream decode step's instantiations (no GPU needed).

    python scripts/kernel_resources.py [--source FILE] [--asm FILE --remarks FILE] [--list-loop NAME]

Compiles genvc_amd/csrc/gpt.hip for gfx950 (device code only, to assembly) with the project's flags and
-Rpass-analysis=kernel-resource-usage and prints one row per k_decode_persist instantiation: SGPR spills, VGPRs,
scratch, occupancy (the compiler's remarks), and counts inside the LAYER LOOP of the emitted assembly: lane
reads (v_readlane_b32: reloads of scalars that were spilled to VGPR lanes), hazard no-ops (s_nop), scalar memory loads
(s_load_* / s_buffer_load_*: the loop is meant to hold none -- they share a counter with the LDS reads, and reading the layer
table with them cost 4-15 us per step, profiles/decode_scalar_spills.md) and all instructions, over all paths.  The layer loop is the largest loop of the function: the widest span between a label
and a branch back to it (the loader wave's segment loop and every poll loop are smaller).  Also printed: lane
writes (v_writelane_b32) in the loop and timestamp reads (s_memrealtime / s_memtime) in the whole function.

--source compiles another translation unit (one that instantiates the kernel); --asm / --remarks read the output of
an earlier compilation instead of compiling; --list-loop NAME prints, for the instantiation whose
template arguments are NAME (e.g. 4,0,0,1,0), the loop's reloads and spills of scalars with the label of the basic block each sits in.

Lane reads are of two kinds: reloads of spilled scalars (from the VGPRs that the assembly's "SGPR spill to VGPR lane" comments name)
and the cross-row steps of the wave sums, which are arithmetic; the table gives the total and the reloads.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genvc_amd import build as gbuild       # HIPCC, FLAGS: the flags the library is built with

KERNEL = "k_decode_persist"
BRANCH = re.compile(r"^\s+(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
SPILL_VGPR = re.compile(r"implicit-def: \$vgpr(\d+) : SGPR spill to VGPR lane")
LANE_OP = re.compile(r"^\s+v_(read|write)lane_b32 (\S+), (\S+),")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)(\s|$)")
TEMPLATE_ARGS = re.compile(r"L([ib])(\d+)E")


def compile_to_asm(source, workdir):
    asm = os.path.join(workdir, "kernel.s")
    cmd = [gbuild.HIPCC] + gbuild.FLAGS + ["-x", "hip", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                           "-I", gbuild.CSRC, source, "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("hipcc failed:\n" + r.stderr[-4000:])
    return open(asm).read(), r.stderr


def parse_remarks(text):
    """{mangled name: {remark key: int}} for the kernel's instantiations."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {}) if KERNEL in m.group(1) else None
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def function_bodies(asm):
    """{mangled name: [lines]} for the kernel's instantiations."""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and KERNEL in m.group(1) and m.group(1) not in out:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                cur.append(line)
    return out


def layer_loop(lines):
    """(first, last) line indices of the largest loop: the widest label .. backward branch span."""
    label_at = {}
    for i, line in enumerate(lines):
        m = LABEL.match(line)
        if m:
            label_at[m.group(1)] = i
    best = (0, -1)
    for i, line in enumerate(lines):
        m = BRANCH.match(line)
        if m and label_at.get(m.group(2), i + 1) <= i:
            j = label_at[m.group(2)]
            if i - j > best[1] - best[0]:
                best = (j, i)
    return best


def mnemonics(lines):
    for line in lines:
        m = INSTR.match(line)
        if m and not line.lstrip().startswith((".", ";")):
            yield m.group(1)


def spill_lane_ops(lines, loop_lines):
    """(reloads, spills) in loop_lines: lane reads from / lane writes to the VGPRs that the compiler names as homes of spilled SGPRs
    (the other lane reads of the loop belong to the arithmetic: the cross-row steps of the wave sums)."""
    homes = {"v" + m.group(1) for line in lines for m in [SPILL_VGPR.search(line)] if m}
    reads = writes = 0
    for line in loop_lines:
        m = LANE_OP.match(line)
        if m and m.group(1) == "read" and m.group(3) in homes:
            reads += 1
        elif m and m.group(1) == "write" and m.group(2) in homes:
            writes += 1
    return reads, writes, homes


def short_name(mangled):
    args = [v for _, v in TEMPLATE_ARGS.findall(mangled.split(KERNEL, 1)[1].split("EEv", 1)[0] + "E")]
    return ",".join(args)


def analyse(asm, remarks_text):
    remarks, rows = parse_remarks(remarks_text), []
    for name, lines in function_bodies(asm).items():
        a, b = layer_loop(lines)
        loop = list(mnemonics(lines[a:b + 1]))
        whole = list(mnemonics(lines))
        r = remarks.get(name, {})
        reloads, respills, homes = spill_lane_ops(lines, lines[a:b + 1])
        rows.append({"name": short_name(name), "mangled": name, "lines": lines, "loop": (a, b),
                     "sgpr_spill": r.get("SGPRs Spill", -1), "vgprs": r.get("VGPRs", -1), "scratch": r.get("ScratchSize [bytes/lane]", -1),
                     "occupancy": r.get("Occupancy [waves/SIMD]", -1),
                     "readlane": loop.count("v_readlane_b32"), "writelane": loop.count("v_writelane_b32"), "nop": loop.count("s_nop"),
                     "instr": len(loop), "sloads": sum(m.startswith(("s_load_", "s_buffer_load_")) for m in loop), "reloads": reloads, "respills": respills, "homes": homes, "stamps": sum(m in ("s_memrealtime", "s_memtime") for m in whole)})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default=os.path.join(gbuild.CSRC, "gpt.hip"))
    ap.add_argument("--asm")
    ap.add_argument("--remarks")
    ap.add_argument("--list-loop", metavar="NAME")
    args = ap.parse_args()
    if args.asm and args.remarks:
        asm, rem = open(args.asm).read(), open(args.remarks).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            asm, rem = compile_to_asm(args.source, d)
    rows = analyse(asm, rem)
    if not rows:
        raise SystemExit(f"no {KERNEL} instantiation in the assembly")
    print(f"{KERNEL}<...>: remarks of the compiler, and counts inside the layer loop of the emitted assembly (all paths)")
    print("| instantiation | SGPR spills | VGPRs | scratch | occupancy | lane reads | of them reloads of spilled scalars | lane writes | hazard no-ops | scalar loads | loop instructions | timestamp reads |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in sorted(rows, key=lambda r: r["name"]):
        print(f"| <{r['name']}> | {r['sgpr_spill']} | {r['vgprs']} | {r['scratch']} | {r['occupancy']} | {r['readlane']} | {r['reloads']} | {r['writelane']} | "
              f"{r['nop']} | {r['sloads']} | {r['instr']} | {r['stamps']} |")
    if args.list_loop:
        for r in rows:
            if r["name"] != args.list_loop:
                continue
            a, b = r["loop"]
            block = "?"
            for line in r["lines"][a:b + 1]:
                m = LABEL.match(line)
                if m:
                    block = m.group(1)
                m = LANE_OP.match(line)
                if m and (m.group(3) if m.group(1) == "read" else m.group(2)) in r["homes"]:
                    print(f"{block:14s} {line.strip()}")


if __name__ == "__main__":
    main()
