#!/usr/bin/env python3
"""Compare the device code of two source trees, kernel by kernel (no GPU needed).

  python tools/isa_compare.py TREE_A TREE_B [--keep DIR]

Every unit of TREE_B's build.py DEVICE_SRC is compiled to device-only assembly in both trees with the
build's own flags (DEVICE_CXXFLAGS + the unit's DEVICE_FLAGS). Per kernel symbol the instruction text
(from the symbol's label to its .Lfunc_end) and the kernel's amdhsa.kernels metadata entry are compared,
after replacing __hip_cuid_<hash>, which is a hash of the source file. The order of the kernels within a
unit is not compared. One line per unit: unit, kernel count, "identical" or the kernels that differ.
Exit status 1 when anything differs. --keep DIR keeps the .s files (DIR/a, DIR/b)."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_isa_build", os.path.join(tree, "raytracingrenderer_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_tree(tree, out_dir, units):
    b = load_build(tree)
    os.makedirs(out_dir, exist_ok=True)
    procs = []
    for rel in units:
        out = os.path.join(out_dir, os.path.basename(rel) + ".s")
        cmd = ([b.HIPCC, "--offload-arch=" + b.ARCH] + b.DEVICE_CXXFLAGS + b.DEVICE_FLAGS.get(rel, []) +
               ["--cuda-device-only", "-S", "-o", out, os.path.join(tree, "raytracingrenderer_amd", "csrc", rel)])
        procs.append((rel, out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    res = {}
    for rel, out, pr in procs:
        log = pr.communicate()[0]
        if pr.returncode != 0:
            sys.stderr.write(log)
            raise SystemExit("compile failed: %s in %s" % (rel, tree))
        res[rel] = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", open(out).read())
    return res


def kernels_of(asm):
    """{symbol: (instruction text, metadata entry)} of one unit's assembly."""
    md = asm[asm.index("amdhsa.kernels:"):]
    md = md[:md.index("amdhsa.target")]
    entries = {}
    for blk in re.split(r"\n  - ", md)[1:]:
        entries[re.search(r"\.symbol:\s+(\S+)\.kd", blk).group(1)] = blk.rstrip("\n")  # (the unit's last entry ends the list)
    out = {}
    for sym, blk in entries.items():
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(sym), asm, re.S | re.M)
        out[sym] = (m.group(0) if m else None, blk)
    return out


def main(argv):
    keep = None
    if "--keep" in argv:
        i = argv.index("--keep")
        keep = argv[i + 1]
        del argv[i:i + 2]
    if len(argv) != 2:
        raise SystemExit(__doc__)
    tree_a, tree_b = (os.path.abspath(t) for t in argv)
    units = load_build(tree_b).DEVICE_SRC
    with tempfile.TemporaryDirectory() as tmp:
        d = keep or tmp
        a = compile_tree(tree_a, os.path.join(d, "a"), units)
        b = compile_tree(tree_b, os.path.join(d, "b"), units)
    bad = 0
    for rel in units:
        ka, kb = kernels_of(a[rel]), kernels_of(b[rel])
        diff = sorted(s for s in set(ka) | set(kb) if ka.get(s) != kb.get(s) or ka[s][0] is None)
        bad += len(diff)
        print("%-28s %3d kernels  %s" % (os.path.basename(rel), len(kb), "identical" if not diff else
                                        "DIFFERENT: " + " ".join(diff)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
