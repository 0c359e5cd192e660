#!/usr/bin/env python3
"""census_valu.py -- vector instructions of a kernel's basic blocks, from the assembly hipcc leaves with -save-temps (no GPU).

    python3 tools/census_valu.py at_k16_g8c-hip-amdgcn-amd-amdhsa-gfx950.s 'at_sweep16ILi1ELi8ELi19E.*Lb1ELb0ELb1E' [--top 6]

For every kernel whose mangled name matches the pattern: registers, scratch, and the basic blocks with the most v_ lines, each with
its opcode histogram.  The unrolled step bodies are the largest blocks; an opcode whose count is a multiple of rows x steps is row
work, one whose count is a multiple of the steps is per-step work, the rest belongs to the block.
"""
import argparse
import collections
import re
import sys


def kernels(path):
    """{name: [lines]} of the function bodies, and {name: {key: value}} of the metadata that follows"""
    body, cur, meta = {}, None, {}
    for ln in open(path):
        m = re.match(r"^(_Z\w+):\s", ln)
        if m and cur is None:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is not None:
            if ln.startswith("\t.end_amdhsa_kernel") or ln.startswith(".Lfunc_end"):
                cur = None
                continue
            body[cur].append(ln.rstrip("\n"))
    name = None
    for ln in open(path):
        m = re.match(r"^\t\.amdhsa_kernel (\S+)", ln)
        if m:
            name = m.group(1)
            meta[name] = {}
        m = re.match(r"^; (codeLenInByte|NumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|SGPRSpill|VGPRSpill)\s*[:=]\s*(\d+)", ln)
        if m and name:
            meta[name][m.group(1)] = int(m.group(2))
    return body, meta


def blocks(lines):
    out, cur, label = [], [], "entry"
    for ln in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            out.append((label, cur))
            label, cur = m.group(1), []
            continue
        s = ln.strip()
        if s and not s.startswith((";", ".")):
            cur.append(s)
    out.append((label, cur))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("pattern")
    ap.add_argument("--top", type=int, default=6)
    args = ap.parse_args()
    body, meta = kernels(args.asm)
    for name, lines in body.items():
        if not re.search(args.pattern, name):
            continue
        print("kernel", name)
        print("  resources", meta.get(name))
        bl = blocks(lines)
        tot = sum(1 for _, b in bl for i in b if i.startswith("v_"))
        print("  v_ lines in all blocks:", tot, " blocks:", len(bl))
        bl.sort(key=lambda x: -sum(1 for i in x[1] if i.startswith("v_")))
        for label, b in bl[:args.top]:
            hist = collections.Counter()
            for i in b:
                op = i.split()[0]
                if op.startswith("v_"):
                    if "row_shl" in i:
                        op += " row_shl"
                    elif "row_shr" in i:
                        op += " row_shr"
                    hist[op] += 1
            nv = sum(hist.values())
            ns = sum(1 for i in b if i.startswith("s_"))
            print("  block %s: %d v_, %d s_, %d ds_, %d global_/scratch_" % (label, nv, ns, sum(1 for i in b if i.startswith("ds_")),
                  sum(1 for i in b if i.startswith(("global_", "scratch_", "buffer_")))))
            for op, n in sorted(hist.items(), key=lambda x: (-x[1], x[0])):
                print("      %5d  %s" % (n, op))


if __name__ == "__main__":
    sys.exit(main())
