#!/usr/bin/env python3
"""Per-kernel instruction streams and resource metadata of a source tree's .hip files, to show that moving code between files
changed no kernel.  No GPU needed.

  python tools/isa_digest.py dump cuda-pathtracer_amd a.json      # compiles every csrc/*.hip for the device only, disassembles
  python tools/isa_digest.py diff parent.json a.json [--skip SUBSTRING]   # --skip: kernels expected to change; their metadata is listed
  python tools/isa_digest.py siblings parent.json a.json SUBSTRING        # a kernel template that gained trailing bool parameters
  python tools/isa_digest.py loop cuda-pathtracer_amd csrc/bounce_sync.hip SUBSTRING   # register copies in a kernel's segment loop

dump: every .hip is compiled with the Makefile's flags + --cuda-device-only, unbundled, and for each kernel the disassembly
(comments stripped, trailing padding ignored) and the AMDGPU metadata note (registers, scratch, LDS, kernarg size) are recorded.
diff: kernel names missing / new / duplicated, and every kernel whose text or metadata differs.  Kernels whose name holds the
--skip substring are left out of all three counts when their names changed (a new template parameter renames every instantiation).
siblings: for the kernels whose name holds SUBSTRING, pairs each new instantiation whose added trailing template arguments are all
false with the parent's instantiation of the same leading arguments and compares registers, spills, scratch and LDS; lists the
resources of every new instantiation; three result lines.  Where the template kept its arity and its last parameter turned from
a bool into an int (SPEC -> SURF), an instantiation whose arguments the parent has is paired with that one, and every other
(SURF = 2) is listed next to the new instantiation of the value below (SURF = 1) with the registers it adds.
"""
import concurrent.futures
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import yaml

ROCM = os.environ.get("ROCM", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
ARCH = os.environ.get("ARCH", "gfx950")
META = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size"]
PAD = re.compile(r"^(s_nop 0|s_code_end|\.\.\.)$")


def makefile_flags(pkg):
    with open(os.path.join(pkg, "Makefile")) as f:
        return re.search(r"^COMMON\s*=\s*(.*)$", f.read(), re.M).group(1).split()


def one_file(pkg, src, tmp, flags):
    base = os.path.join(tmp, os.path.basename(src))
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "--offload-arch=" + ARCH, *flags, "--cuda-device-only", "-c", src, "-o", base + ".o"],
                   check=True, cwd=pkg)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + ARCH,
                    "--input=" + base + ".o", "--output=" + base + ".co", "--unbundle"], check=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", base + ".co"], capture_output=True, text=True, check=True).stdout
    doc = yaml.safe_load(notes[notes.index("---"):notes.rindex("...")])
    kernels = {k[".name"]: {m: k.get(m) for m in META} for k in doc.get("amdhsa.kernels", [])}
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", base + ".co"],
                         capture_output=True, text=True, check=True).stdout
    out, name, lines = [], None, []

    def close():
        if name in kernels:
            while lines and PAD.match(lines[-1]):
                lines.pop()
            out.append({"name": name, "file": os.path.basename(src), "meta": kernels[name], "n": len(lines),
                        "sha": hashlib.sha256("\n".join(lines).encode()).hexdigest()})
    for ln in dis.split("\n"):
        m = re.match(r"^<(.*)>:$", ln.strip())
        if m:
            close()
            name, lines = m.group(1), []
        elif name:
            ln = ln.split("//")[0].strip()
            if ln:
                lines.append(ln)
    close()
    assert len(out) == len(kernels), (src, len(out), len(kernels))
    return out


def dump(pkg, dest, extra):
    pkg = os.path.abspath(pkg)
    flags = makefile_flags(pkg) + extra
    srcs = sorted(os.path.join(pkg, "csrc", f) for f in os.listdir(os.path.join(pkg, "csrc")) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(int(os.environ.get("JOBS", "4"))) as ex:
        res = [k for r in ex.map(lambda s: one_file(pkg, s, tmp, flags), srcs) for k in r]
    with open(dest, "w") as f:
        json.dump(res, f, indent=0)
    print("%d kernels in %d files -> %s" % (len(res), len(srcs), dest))


def diff(a, b, skip):
    A, B = json.load(open(a)), json.load(open(b))
    bad = 0
    for tag, L in (("parent", A), ("new", B)):
        names = [k["name"] for k in L]
        for n in sorted(set(n for n in names if names.count(n) > 1)):
            print("DUPLICATE in %s: %s" % (tag, n)); bad += 1
    da, db = {k["name"]: k for k in A}, {k["name"]: k for k in B}
    renamed = 0
    for n in sorted(set(da) - set(db)):
        if skip and skip in n:
            renamed += 1
            continue
        print("MISSING: %s" % n); bad += 1
    for n in sorted(set(db) - set(da)):
        if skip and skip in n:
            renamed += 1
            continue
        print("NEW: %s" % n); bad += 1
    if renamed:
        print("%d names with '%s' exist on one side only (see `siblings`)" % (renamed, skip))
    same = skipped = 0
    for n in sorted(set(da) & set(db)):
        if skip and skip in n:
            skipped += 1
            ma, mb = da[n]["meta"], db[n]["meta"]
            print("CHANGED %s\n    %s" % (n, "  ".join("%s %s->%s" % (m[1:], ma[m], mb[m]) for m in META if ma[m] != mb[m]) or "(metadata equal)"))
            continue
        if da[n]["sha"] != db[n]["sha"] or da[n]["meta"] != db[n]["meta"]:
            print("DIFFERS: %s (%s -> %s)  text %s  meta %s" % (n, da[n]["file"], db[n]["file"], da[n]["sha"] == db[n]["sha"], da[n]["meta"] == db[n]["meta"])); bad += 1
        else:
            same += 1
    print("parent %d kernels, new %d; identical %d, skipped %d, defects %d" % (len(A), len(B), same, skipped, bad))
    return 1 if bad else 0


RESOURCES = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
             ".group_segment_fixed_size"]


def template_args(name):
    """the literal template arguments (Li<n>E, Lb<n>E) of a mangled kernel name, in order"""
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", name.split("Ev")[0]))


def siblings(a, b, sub):
    A = {template_args(k["name"]): k for k in json.load(open(a)) if sub in k["name"]}
    B = {template_args(k["name"]): k for k in json.load(open(b)) if sub in k["name"]}
    n_lead = len(next(iter(A)))
    paired = differ = heavy = 0
    for args in sorted(B):
        m = B[args]["meta"]
        line = "%s<%s>: %s, %d instructions" % (sub, ", ".join(map(str, args)), "  ".join("%s %s" % (r[1:], m[r]) for r in RESOURCES), B[args]["n"])
        widened = len(args) == n_lead and args not in A         # same arity, a value the parent's bool does not have
        if widened:
            sib = B.get(args[:-1] + (args[-1] - 1,))
            if sib is None:
                line += "  | NO SIBLING"; differ += 1
            else:
                line += "  | sibling <%s>: %s" % (", ".join(map(str, args[:-1] + (args[-1] - 1,))),
                                                 "  ".join("%s %+d" % (r[1:], m[r] - sib["meta"][r]) for r in RESOURCES[:5]))
        elif not any(args[n_lead:]):
            p = A.get(args[:n_lead])
            if p is None:
                line += "  | NO PARENT"; differ += 1
            else:
                paired += 1
                same = all(p["meta"][r] == m[r] for r in RESOURCES)
                differ += 0 if same else 1
                line += "  | parent: %s, %d instructions" % ("same resources" if same else "  ".join("%s %s" % (r[1:], p["meta"][r]) for r in RESOURCES if p["meta"][r] != m[r]), p["n"])
        if m[".private_segment_fixed_size"] or m[".vgpr_spill_count"]:
            heavy += 1
        print(line)
    spills = [k["meta"][".sgpr_spill_count"] for k in B.values()]
    pspills = [k["meta"][".sgpr_spill_count"] for k in A.values()]
    print("%s: parent %d instantiations, new %d; %d with the added parameters false, %d of them differ from the parent's resources" % (sub, len(A), len(B), paired, differ))
    print("%s: %d of %d new instantiations use scratch or spill VGPRs" % (sub, heavy, len(B)))
    print("%s: SGPRs parked in VGPR lanes (sgpr_spill_count): parent %d - %d, new %d - %d" % (sub, min(pspills), max(pspills), min(spills), max(spills)))
    return 1 if differ or heavy or len(A) != paired else 0


COPIES = ("v_mov_b32", "v_readlane_b32", "v_writelane_b32")


def loop_blocks(body):
    """the basic blocks of one function of hipcc's -S output as (label, innermost loop header or None, is a header, instructions),
    and each loop header's enclosing headers, from the loop annotations the compiler writes behind every block label"""
    blocks, parents = [["", None, False, []]], {}
    lines = body.split("\n")
    for n, ln in enumerate(lines):
        lab = re.match(r"^(\.LBB\d+_\d+):(.*)$", ln)
        if lab:
            notes = lab.group(2)
            for more in lines[n + 1:]:                       # a nested header's annotation goes on over comment-only lines
                if not re.match(r"^\s*;", more):
                    break
                notes += more
            name = lab.group(1)[2:]
            header = "Loop Header" in notes
            if header:
                parents[name] = re.findall(r"Parent Loop (BB\d+_\d+)", notes)
            inner = name if header else (re.search(r"in Loop: Header=(BB\d+_\d+)", notes) or [None, None])[1]
            blocks.append([name, inner, header, []])
            continue
        ln = ln.split(";")[0].strip()
        if ln and not ln.startswith(".") and not ln.endswith(":"):
            blocks[-1][3].append(ln.split()[0])
    return blocks, parents


def loop(pkg, src, sub):
    """For each kernel whose mangled name holds SUB: its largest outermost loop (a bounce kernel's segment loop), split into the
    blocks of the loop itself and the blocks of the loops nested in it (the walk), with the instructions that compute nothing.
    Static counts over all blocks, the rarely taken ones included.  src: a .hip of the package, or a .s that hipcc -S wrote."""
    if src.endswith(".s"):
        text = open(src).read()
    else:
        pkg = os.path.abspath(pkg)
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "k.s")
            subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "--offload-arch=" + ARCH, *makefile_flags(pkg), "--cuda-device-only", "-S", src,
                            "-o", out], check=True, cwd=pkg)
            text = open(out).read()
    found = 0
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        if sub not in m.group(1):
            continue
        found += 1
        blocks, parents = loop_blocks(m.group(2))
        outer = [h for h, ps in parents.items() if not ps]
        size = {h: sum(len(b[3]) for b in blocks if b[1] and (b[1] == h or h in parents[b[1]])) for h in outer}
        if not size:
            print("%s: no loop" % m.group(1))
            continue
        h = max(size, key=size.get)
        own = [op for b in blocks if b[1] == h for op in b[3]]
        nested = [op for b in blocks if b[1] and b[1] != h and h in parents[b[1]] for op in b[3]]
        print("%s\n  loop at %s" % (m.group(1), h))
        for tag, ops in (("outside its inner loops", own), ("in its inner loops", nested)):
            print("  %-24s %4d instructions, %4d VALU:  %s  v_cndmask %d;  s_load %d  s_mov %d  s_waitcnt %d  ds_read %d" % (
                tag, len(ops), sum(1 for op in ops if op.startswith("v_")), "  ".join("%s %d" % (c, sum(1 for op in ops if op.startswith(c))) for c in COPIES),
                sum(1 for op in ops if op.startswith("v_cndmask")), sum(1 for op in ops if op.startswith("s_load")),
                sum(1 for op in ops if op.startswith("s_mov")), ops.count("s_waitcnt"), sum(1 for op in ops if op.startswith("ds_read"))))
    return 0 if found else 1


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "loop":
        sys.exit(loop(sys.argv[2], sys.argv[3], sys.argv[4]))
    elif len(sys.argv) >= 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3], sys.argv[4:])
    elif len(sys.argv) >= 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) > 5 and sys.argv[4] == "--skip" else None))
    elif len(sys.argv) == 5 and sys.argv[1] == "siblings":
        sys.exit(siblings(sys.argv[2], sys.argv[3], sys.argv[4]))
    else:
        sys.exit(__doc__)
