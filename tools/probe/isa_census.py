#!/usr/bin/env python3
"""Static instruction census of the streaming kernel (no GPU needed).

Two inputs, either or both:

  --lib  polee_amd/csrc/libpolee_hip.so   the gfx950 code objects inside the library: register counts, scratch and the
                                          waves per SIMD they allow, from the kernels' metadata, and the instruction mix
                                          of the whole kernel from the disassembly
  --asm  loglik.s                         compiler output with loop annotations (hipcc ... --offload-device-only -S, or the
                                          .s that -save-temps leaves): the same mix PER SLICE LOOP, i.e. per loop of depth 2
                                          under the kernel's tile loop, named after the matrix instruction it contains

Counts are STATIC: a slice loop holds all straight-line versions of its body (groups of four transcripts x wrapped or not),
so a column is "instructions in the loop", not "instructions a slice executes"; the difference between two builds is what
was removed from (or added to) the loop's text.  Classes: SALU (s_* but waits / nops / branches), BRANCH (s_cbranch, s_branch),
WAIT (s_waitcnt, s_nop, s_barrier), VALU (v_* but MFMA), MFMA, DS (ds_*), VMEM (global_*, buffer_*, scratch_*, flat_*).

It also checks a hazard the compiler cannot see into inline assembly for: an LDS-DMA instruction (global_load_lds_*) whose
SGPR base was written by v_readlane / v_readfirstlane fewer than five wait states before it.

    python tools/probe/isa_census.py --lib polee_amd/csrc/libpolee_hip.so [--kernel REGEX] [--json]
"""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("POLEE_LLVM_BIN", "/opt/rocm/llvm/bin")
PRODUCTION = r"loglik_stream_kernelILi6ELb0ELb0ELb0EEE"  # K = 6, no lp, no multiplicities, float atomics: the VI step's
CLASSES = ("SALU", "BRANCH", "WAIT", "VALU", "MFMA", "DS", "VMEM")
VGPRS_PER_SIMD = 512  # gfx90a and later: one file of 512 registers per lane for vector and accumulation registers
VGPR_GRANULE = 8


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "MFMA"
    if op.startswith("s_cbranch") or op in ("s_branch", "s_setpc_b64", "s_swappc_b64", "s_endpgm"):
        return "BRANCH"
    if op in ("s_waitcnt", "s_nop", "s_barrier", "s_sleep") or op.startswith("s_waitcnt"):
        return "WAIT"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "DS"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "VMEM"
    if op.startswith("v_"):
        return "VALU"
    return None


def code_objects(lib):
    """The gfx950 code objects bundled in a host library (uncompressed clang offload bundles)."""
    data = open(lib, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, at = [], 0
    while True:
        at = data.find(magic, at)
        if at < 0:
            break
        p = at + len(magic)
        (n,) = struct.unpack_from("<Q", data, p)
        p += 8
        if n > 64:  # (the magic as a string constant somewhere else)
            at += 1
            continue
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tl].decode("ascii", "replace")
            p += tl
            if "gfx950" in triple and size > 0:
                out.append(data[at + off:at + off + size])
        at = p
    return out


def kernel_metadata(obj_path):
    """{kernel name: {vgpr, agpr, sgpr, scratch, lds, max_threads}} from the code object's AMDGPU metadata note."""
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj_path], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in re.split(r"\n\s*- \.", txt):
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or ".vgpr_count" not in blk:
            continue
        num = lambda key, default=0: int(m.group(1)) if (m := re.search(r"\." + key + r":\s+(\d+)", blk)) else default  # noqa: E731
        res[name.group(1)] = {"vgpr": num("vgpr_count"), "agpr": num("agpr_count"), "sgpr": num("sgpr_count"),
                              "scratch": num("private_segment_fixed_size"), "spilled_vgprs": num("vgpr_spill_count"),
                              "spilled_sgprs": num("sgpr_spill_count"), "lds_static": num("group_segment_fixed_size"),
                              "max_threads": num("max_flat_workgroup_size")}
    return res


def waves_per_simd(vgpr_total):
    alloc = max(VGPR_GRANULE, -(-vgpr_total // VGPR_GRANULE) * VGPR_GRANULE)
    return min(8, VGPRS_PER_SIMD // alloc)


INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")


def parse_instructions(lines):
    """[(opcode, operand text)] of assembly or disassembly lines; labels come back as ('label', name)."""
    out = []
    for ln in lines:
        ln = ln.split("//")[0].split(";")[0].rstrip() if not ln.lstrip().startswith(";") else ""
        if not ln:
            continue
        m = re.match(r"^(\.?[A-Za-z_][\w.$]*):", ln) or re.match(r"^[0-9a-f]+ <([^>]+)>:", ln)
        if m:
            out.append(("label", m.group(1)))
            continue
        m = INSN.match(ln)
        if m and classify(m.group(1)):
            out.append((m.group(1), m.group(2).strip()))
    return out


def mix(insns):
    c = dict.fromkeys(CLASSES, 0)
    extra = {"s_nop_wait_states": 0, "v_readlane": 0, "v_readfirstlane": 0, "v_writelane": 0, "lds_dma": 0}
    for op, args in insns:
        if op == "label":
            continue
        c[classify(op)] += 1
        if op == "s_nop":
            extra["s_nop_wait_states"] += int(args.strip() or 0, 0) + 1
        for key in ("v_readlane", "v_readfirstlane", "v_writelane"):
            if op.startswith(key):
                extra[key] += 1
        if op.startswith("global_load_lds"):
            extra["lds_dma"] += 1
    c["total"] = sum(c[k] for k in CLASSES)
    c.update(extra)
    return c


def sgprs_of(text):
    """SGPR numbers named in an operand string."""
    regs = set()
    for a, b in re.findall(r"\bs\[(\d+):(\d+)\]", text):
        regs.update(range(int(a), int(b) + 1))
    regs.update(int(a) for a in re.findall(r"\bs(\d+)\b", text))
    return regs


def dma_hazards(insns):
    """LDS-DMA instructions whose SGPR base was written by a VALU lane read fewer than five wait states earlier (walking
    back in program order; a label does not stop the walk, which errs on the side of reporting)."""
    bad = []
    for i, (op, args) in enumerate(insns):
        if not op.startswith("global_load_lds"):
            continue
        base = sgprs_of(args)
        waited, j = 0, i - 1
        while j >= 0 and waited < 5:
            pop, pargs = insns[j]
            if pop == "label":
                j -= 1
                continue
            if pop.startswith(("v_readlane", "v_readfirstlane")) and sgprs_of(pargs.split(",")[0]) & base:
                bad.append((i, op + " " + args, pop + " " + pargs, waited))
                break
            waited += (int(pargs.strip() or 0, 0) + 1) if pop == "s_nop" else 1
            j -= 1
    return bad


def functions_of_asm(path, pattern):
    """{symbol: lines} of the functions of a .s file whose name matches."""
    res, cur, name = {}, None, None
    with open(path, errors="replace") as fh:
        for ln in fh:
            m = re.match(r"^(_Z\w+):", ln)
            if m and re.search(pattern, m.group(1)):
                name, cur = m.group(1), []
                res[name] = cur
            elif cur is not None:
                if ln.startswith(".Lfunc_end"):
                    cur = None
                else:
                    cur.append(ln)
    return res


def slice_loops(lines):
    """The loops of depth 2 (slice loops under the tile loop) of an annotated function: [(header label, lines)].  A depth-2 loop
    runs from its header to the line before the next block that is not `in Loop: Header=<it>` / a child of it."""
    headers = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):\s*;.*Parent Loop BB\d+_\d+ Depth=1\s*$", ln)
        if m and i + 1 < len(lines) and re.search(r"This Loop Header: Depth=2|This Inner Loop Header: Depth=2", lines[i + 1]):
            headers[m.group(1)] = i
    member = {h: [] for h in headers}
    cur = None  # header the current block belongs to
    block_re = re.compile(r"^(\.LBB\d+_\d+):\s*;(.*)$|^; %bb\.\d+:\s*;(.*)$")
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = block_re.match(ln)
        if m:
            note = (m.group(2) or m.group(3) or "")
            label = m.group(1)
            if label in headers:
                cur = label
            else:
                h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
                p = re.search(r"Parent Loop (BB\d+_\d+) Depth=2", note)
                k = i + 1
                while p is None and k < len(lines) and lines[k].lstrip().startswith(";") and not block_re.match(lines[k]):
                    p = re.search(r"Parent Loop (BB\d+_\d+) Depth=2", lines[k])
                    k += 1
                if h and int(h.group(2)) == 2 and ".L" + h.group(1) in headers:
                    cur = ".L" + h.group(1)
                elif p and ".L" + p.group(1) in headers:
                    cur = ".L" + p.group(1)
                elif h and int(h.group(2)) >= 3:
                    pass  # (a block of a child loop: stays with the loop it is nested in)
                else:
                    cur = None
        if cur is not None:
            member[cur].append(ln)
        i += 1
    return [(h, member[h]) for h in sorted(headers, key=headers.get)]


def loop_name(c, text):
    if c["MFMA"] == 0:
        return "mixed_stream (BN)" if c["DS"] > 8 else "ring start / prefetch"
    narrow = "v_mfma_f32_4x4x1" in text
    masked = "v_cndmask_b32_dpp" in text
    if narrow:
        return "wide_masked_stream (A2M)" if text.count("v_cndmask_b32_dpp") > 64 else ("narrow_stream masked (A1M)" if masked else "narrow_stream dense (A1)")
    return "wide_stream (A2)"


def table(rows):
    cols = ("name",) + CLASSES + ("total", "s_nop_wait_states", "v_readlane", "v_readfirstlane", "v_writelane", "lds_dma")
    width = max(len(r["name"]) for r in rows) + 2
    lines = ["%-*s" % (width, "loop") + " ".join("%8s" % c[:8] for c in cols[1:])]
    for r in rows:
        lines.append("%-*s" % (width, r["name"]) + " ".join("%8d" % r[c] for c in cols[1:]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib")
    ap.add_argument("--asm")
    ap.add_argument("--kernel", default=PRODUCTION, help="regular expression on the mangled kernel name")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the tables")
    args = ap.parse_args()
    if not args.lib and not args.asm:
        ap.error("--lib and / or --asm")
    res = {"kernel_pattern": args.kernel}
    if args.lib:
        kernels = {}
        with tempfile.TemporaryDirectory() as tmp:
            for n, blob in enumerate(code_objects(args.lib)):
                path = os.path.join(tmp, "co%d.o" % n)
                with open(path, "wb") as fh:
                    fh.write(blob)
                for name, md in kernel_metadata(path).items():
                    if not re.search(args.kernel, name):
                        continue
                    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + name, path],
                                         capture_output=True, text=True, check=True).stdout.splitlines()
                    insns = parse_instructions(dis)
                    md["waves_per_simd"] = waves_per_simd(md["vgpr"])
                    md["mix"] = mix(insns)
                    md["dma_hazards"] = [{"dma": d, "writer": w, "wait_states_between": ws} for _, d, w, ws in dma_hazards(insns)]
                    kernels[name] = md
        res["lib"] = {"path": args.lib, "kernels": kernels}
    if args.asm:
        fns = {}
        for name, lines in functions_of_asm(args.asm, args.kernel).items():
            insns = parse_instructions(lines)
            rows = [dict(mix(insns), name="whole kernel")]
            for header, body in slice_loops(lines):
                c = mix(parse_instructions(body))
                rows.append(dict(c, name="%s %s" % (loop_name(c, "".join(body)), header)))
            fns[name] = {"rows": rows, "dma_hazards": [{"dma": d, "writer": w, "wait_states_between": ws} for _, d, w, ws in dma_hazards(insns)]}
        res["asm"] = {"path": args.asm, "functions": fns}
    if args.json:
        print(json.dumps(res))
        return 0
    if args.lib:
        for name, md in res["lib"]["kernels"].items():
            print("%s\n  VGPRs %d (of them AGPRs %d)  SGPRs %d  scratch %d B/lane  spilled VGPRs %d  spilled SGPRs %d  -> %d waves per SIMD"
                  % (name, md["vgpr"], md["agpr"], md["sgpr"], md["scratch"], md["spilled_vgprs"], md["spilled_sgprs"], md["waves_per_simd"]))
            print(table([dict(md["mix"], name="whole kernel (code object)")]))
            print("  LDS-DMA hazards: %s" % (md["dma_hazards"] or "none"))
    if args.asm:
        for name, f in res["asm"]["functions"].items():
            print("%s  (static counts per slice loop: all straight-line versions of the body together)" % name)
            print(table(f["rows"]))
            print("  LDS-DMA hazards: %s" % (f["dma_hazards"] or "none"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
