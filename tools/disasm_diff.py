#!/usr/bin/env python3
"""Compares the gfx950 instruction streams of every kernel of two source trees (no GPU needed).

    python tools/disasm_diff.py PARENT_TREE THIS_TREE [--out profiles/NAME.txt] [--files a.hip b.hip ...]

Each translation unit of n-body_amd/csrc is compiled device-only to assembly (hipcc -S --cuda-device-only) in both
trees.  A kernel's instruction stream is its instruction lines with comments dropped and the function number taken out
of the basic-block labels (.LBB<fn>_<bb>), so that a kernel appended to a file does not show up in its neighbours.  The
summary lists, per file, the kernels whose streams are identical, those that changed and those that are new or gone,
and the compiler's resource report (VGPRs, SGPRs, scratch, occupancy) of the changed and new ones.  Exit code 1 when
an existing kernel changed or went away.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

FILES = ["api.hip", "direct.hip", "direct_sym.hip", "hermite.hip", "hermite_block.hip", "hermite_batch.hip", "system_diag.hip", "integrator.hip", "energy.hip", "spatial_hash.hip", "slab.hip",
         "barnes_hut.hip", "sharded.hip", "sharded_hash.hip"]


def assembly(tree, name, out_dir, tag):
    src = os.path.join(tree, "n-body_amd", "csrc", name)
    out = os.path.join(out_dir, f"{tag}_{name}.s")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
           "-fvisibility=hidden", "-I" + os.path.join(tree, "include"), "-I" + os.path.dirname(src),
           "--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd)
    return out


def kernels(path):
    """{symbol: (instruction lines, resource dict)} of the amdgpu_kernel functions of one assembly file"""
    out, cur, name = {}, None, None
    res = {}
    kernel_syms = set()
    lines = open(path).read().splitlines()
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kernel_syms.add(m.group(1))
    for ln in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        if m and m.group(1) in kernel_syms and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is None:
            m = re.match(r"^; (NumVgprs|TotalNumSgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", ln)
            if m and name:
                res.setdefault(name, {})[m.group(1)] = int(m.group(2))
            continue
        if ln.startswith(".Lfunc_end"):
            out[name] = cur
            cur = None
            continue
        body = ln.split(";")[0].rstrip()
        if not body.strip() or body.strip().startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", body):
                cur.append(re.sub(r"\.LBB\d+_", ".LBB_", body))
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", body.strip()))
    return {k: (v, res.get(k, {})) for k, v in out.items()}


def demangle(sym):
    try:
        return subprocess.check_output(["c++filt", sym], text=True).strip()
    except Exception:
        return sym


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--files", nargs="*", default=FILES)
    a = ap.parse_args()
    rows, total_same, total_changed = [], 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for f in a.files:
            # (a translation unit the parent does not have yet: every kernel of it is new)
            has = os.path.exists(os.path.join(a.parent, "n-body_amd", "csrc", f))
            old = kernels(assembly(a.parent, f, tmp, "parent")) if has else {}
            new = kernels(assembly(a.this, f, tmp, "this"))
            same = [k for k in old if k in new and old[k][0] == new[k][0]]
            changed = [k for k in old if k in new and old[k][0] != new[k][0]]
            gone = [k for k in old if k not in new]
            added = [k for k in new if k not in old]
            total_same += len(same)
            total_changed += len(changed) + len(gone)
            rows.append(f"{f}: {len(old)} kernels in the parent, {len(new)} here; identical instruction streams "
                        f"{len(same)}, changed {len(changed)}, gone {len(gone)}, new {len(added)}")
            library = 0  # (rocPRIM's kernels are counted, the project's own are listed)
            for k in same:
                name = demangle(k)
                if "nbh::" not in name.split("(")[0]:
                    library += 1
                    continue
                h = hashlib.sha1("\n".join(new[k][0]).encode()).hexdigest()[:12]
                rows.append(f"  same    {len(new[k][0]):6d} lines  sha1 {h}  {name[:150]}")
            if library:
                rows.append(f"  same    {library} kernels instantiated from libraries (rocPRIM)")
            def resources(tag, k, lines, r):
                rows.append(f"  {tag} {len(lines):6d} lines  VGPR {r.get('NumVgprs')} AGPR {r.get('NumAgprs')} "
                            f"SGPR {r.get('TotalNumSgprs')} scratch {r.get('ScratchSize')} B LDS {r.get('LDSByteSize')} B "
                            f"occupancy {r.get('Occupancy')} waves/SIMD  {demangle(k)[:150]}")

            # the parent's side of what changed or went away (the kernel a new instantiation replaces is read off here),
            # then this tree's side of what changed or is new
            for tag, ks in (("CHANGED", changed), ("GONE   ", gone)):
                for k in ks:
                    resources(tag, k, *old[k])
            for k in added + changed:
                resources("new    ", k, *new[k])
    head = (f"instruction streams of the existing kernels, parent tree against this tree (hipcc -O3 --offload-arch=gfx950 "
            f"--cuda-device-only -S): {total_same} identical, {total_changed} changed or gone")
    text = "\n".join([head] + rows) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)
    return 1 if total_changed else 0


if __name__ == "__main__":
    sys.exit(main())
