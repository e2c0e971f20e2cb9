"""Vector-memory operations and the waits on them in the main loops of the 8-state E-step sweeps.

Compiles bhmm_amd/csrc/bhmm_amd.hip for the device only (no GPU needed), or reads a .s file made that
way, and prints for every main loop of the chosen kernels

  * the vector-memory operations and every `s_waitcnt` with a vmcnt field, in program order, with the
    number of vector-memory operations issued since the top of the loop (a wavefront's vector-memory
    operations retire in issue order: `vmcnt(n)` waits until at most n are outstanding, so the wait in
    front of the first use of a register set should have n = operations issued after that set's last
    load; `vmcnt(0)` waits for everything, the loads just issued included);
  * the counts of VALU, DPP, LDS, vector-memory and scratch instructions of the loop;

and the kernel's VGPRs, spills and scratch bytes from the code object's metadata.

A main loop is an innermost loop (by the compiler's own loop annotations in the listing) with at least
--min-valu VALU instructions and at least one vector-memory load; the four-step warm-up loops stay below
the default.  Blocks are printed header first, then in the order of the listing.

    python tools/isa_waits.py                      # compile the working tree
    python tools/isa_waits.py --asm some.s         # read an existing listing
    python tools/isa_waits.py --kernels 'k_estep_lightILi8ELi1ELb1ELb0ELb0ELi2E'   # other kernels (substring of the mangled name)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, "bhmm_amd", "csrc", "bhmm_amd.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "--cuda-device-only", "-S"]
# the instantiations the two 8-state shapes of BASELINE.md run: <8, kind, SPEC, no gamma, not careful, phase>
DEFAULT = [("P1 discrete", "13k_estep_lightILi8ELi1ELb1ELb0ELb0ELi2E"), ("P2 discrete", "7k_estepILi8ELi1ELb1ELb0ELb0ELi3E"),
           ("P1 gaussian", "13k_estep_lightILi8ELi0ELb1ELb0ELb0ELi2E"), ("P2 gaussian", "7k_estepILi8ELi0ELb1ELb0ELb0ELi3E")]
VMEM = re.compile(r"^(global|flat|buffer|scratch)_(load|store|atomic)")
BRANCH = re.compile(r"^s_c?branch\S*\s+(\.LBB\d+_\d+)")
DPP = re.compile(r"quad_perm|row_shl|row_shr|row_ror|row_bcast|row_mirror|row_half_mirror|row_newbcast|row_share|row_xmask|wave_")


def compile_unit(path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-o", path, UNIT])


def kernel_blocks(lines, sub):
    """(mangled name, basic blocks) of the kernel whose mangled name contains sub; a block is
    [label, the compiler's loop annotation of the label, instruction lines]"""
    for i, l in enumerate(lines):
        if l.startswith("_ZN") and sub in l.split(":")[0] and l.rstrip().split(":")[1].lstrip().startswith(";"):
            name = l.split(":")[0]
            blocks = [["entry", "", []]]
            fresh = False  # directly behind a label: comment lines continue its annotation
            for m in lines[i + 1:]:
                if m.startswith(".Lfunc_end"):
                    break
                s = m.strip()
                lab = re.match(r"^(\.LBB\d+_\d+):(.*)$", s)
                if lab:
                    blocks.append([lab.group(1), lab.group(2), []])
                    fresh = True
                elif s.startswith(";"):
                    if fresh:
                        blocks[-1][1] += " " + s
                elif s and not s.startswith("."):
                    blocks[-1][2].append(s)
                    fresh = False
            return name, blocks
    return None, []


def loops_of(blocks):
    """innermost loops from the compiler's annotations: the header block first (execution order of a
    rotated loop), then the other blocks of the loop in the order of the listing"""
    loops = []
    for lab, note, _ in blocks:
        if "Inner Loop Header" in note:
            hdr = lab[2:]  # BBn_m
            rest = [b for b in blocks if re.search(r"in Loop: Header=%s\b" % re.escape(hdr), b[1])]
            loops.append([b for b in blocks if b[0] == lab] + rest)
    return loops


def classify(insts):
    c = dict(total=0, valu=0, dpp=0, lds=0, vmem=0, scratch=0)
    for s in insts:
        op = s.split()[0]
        c["total"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
            if DPP.search(s):
                c["dpp"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif VMEM.match(op):
            c["vmem"] += 1
            if op.startswith("scratch_"):
                c["scratch"] += 1
    return c


def metadata(lines, name):
    """.vgpr_count etc. of the kernel from the amdhsa metadata at the end of the listing"""
    out = {}
    block = []
    blocks = []
    for l in lines:
        if l.startswith("  - .") and block:
            blocks.append(block)
            block = []
        if l.startswith("  - .") or (block and l.startswith("    .")):
            block.append(l)
    if block:
        blocks.append(block)
    for blk in blocks:
        if any(re.match(r"^\s+(- )?\.name:\s+%s\s*$" % re.escape(name), l) for l in blk):
            for l in blk:
                m = re.match(r"^\s+(?:- )?\.(vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", l)
                if m:
                    out[m.group(1)] = int(m.group(2))
    return out


def report(lines, title, sub, min_valu):
    name, blocks = kernel_blocks(lines, sub)
    if not name:
        print("## %s: no kernel matching %s\n" % (title, sub))
        return
    md = metadata(lines, name)
    print("## %s" % title)
    print("`%s`  " % name[:name.find("EEv") + 2 if "EEv" in name else 60])
    print("VGPRs %s, VGPR spills %s, scratch bytes / lane %s, %d instructions\n"
          % (md.get("vgpr_count"), md.get("vgpr_spill_count"), md.get("private_segment_fixed_size"),
             sum(len(b[2]) for b in blocks)))
    found = False
    for loop in loops_of(blocks):
        insts = [s for b in loop for s in b[2]]
        c = classify(insts)
        if c["valu"] < min_valu or not any(re.match(r"^(global|flat|buffer)_load", s) for s in insts):
            continue
        found = True
        print("### loop %s, %d block%s  (%d instructions: VALU %d, of them DPP %d; LDS %d; vector memory %d, of them scratch %d)"
              % (loop[0][0], len(loop), "s" if len(loop) > 1 else "", c["total"], c["valu"], c["dpp"], c["lds"],
                 c["vmem"], c["scratch"]))
        issued = valu = 0
        print("```")
        for k, (lab, _, bi) in enumerate(loop):
            if k:
                print("%5d  %s:" % (valu, lab))
            for s in bi:
                op = s.split()[0]
                if op.startswith("v_"):
                    valu += 1
                if VMEM.match(op):
                    issued += 1
                    print("%5d  %-28s ; vector-memory operation %d of the iteration" % (valu, op, issued))
                elif op == "s_waitcnt" and "vmcnt" in s:
                    flag = "   <-- waits for everything" if "vmcnt(0)" in s else ""
                    print("%5d  %-28s ; %d issued so far%s" % (valu, s, issued, flag))
                elif BRANCH.match(s):
                    print("%5d  %s" % (valu, s))
        print("```")
        print("(first column: VALU instructions since the top of the loop)\n")
    if not found:
        print("no main loop found (min VALU %d)\n" % min_valu)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="read this listing instead of compiling the unit")
    ap.add_argument("--kernels", nargs="*", help="substrings of mangled kernel names (default: the four 8-state E-step sweeps)")
    ap.add_argument("--min-valu", type=int, default=250)
    args = ap.parse_args()
    if args.asm:
        path = args.asm
    else:
        path = os.path.join(tempfile.mkdtemp(prefix="isa_waits_"), "bhmm_amd.s")
        compile_unit(path)
    with open(path) as f:
        lines = f.read().split("\n")
    kernels = [(k, k) for k in args.kernels] if args.kernels else DEFAULT
    for title, sub in kernels:
        report(lines, title, sub, args.min_valu)
    return 0


if __name__ == "__main__":
    sys.exit(main())
