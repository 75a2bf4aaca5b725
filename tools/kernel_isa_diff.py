"""Which kernels of a .hip file compile to other instructions than at a git revision?

    python tools/kernel_isa_diff.py imagestitch_amd/csrc/surf_kernels.hip [REV]      (REV defaults to HEAD~1)

Compiles the file as it stands and as it was at REV (with the headers of REV: the revision's csrc and include trees are unpacked next to
it) for gfx950 (device only, the Makefile's flags), strips directives, comments and labels' metadata, and prints `same` or `DIFFERENT` per kernel.  A kernel trace of two builds can then tell a change of code from the
run-to-run movement of kernels whose instruction stream is identical (profiles/r11_ab_candidate_path.txt)."""
import os
import re
import subprocess
import sys
import tarfile
import tempfile

FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-value --cuda-device-only -S".split()


def kernels(asm):
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)", asm):
        m = re.search(r"\n" + re.escape(name) + r":[^\n]*\n", asm)
        body = asm[m.end():asm.index(".end_amdhsa_kernel", m.end())]
        out[name] = "\n".join(l for l in body.splitlines() if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";")))
    return out


def compile_to_asm(src, out):
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + [src, "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


def main(path, rev="HEAD~1"):
    root = subprocess.check_output(["git", "rev-parse", "--show-toplevel"], text=True).strip()
    rel = os.path.relpath(os.path.abspath(path), root)
    with tempfile.TemporaryDirectory() as tmp:
        tar = os.path.join(tmp, "rev.tar")                              # the revision's sources and headers, at their relative places
        subprocess.check_call(["git", "archive", "-o", tar, rev, os.path.dirname(rel), "include"], cwd=root)
        tarfile.open(tar).extractall(os.path.join(tmp, "rev"))
        old = kernels(compile_to_asm(os.path.join(tmp, "rev", rel), os.path.join(tmp, "old.s")))
        new = kernels(compile_to_asm(os.path.abspath(path), os.path.join(tmp, "new.s")))
    for name in sorted(set(old) | set(new)):
        state = "same" if old.get(name) == new.get(name) else ("DIFFERENT" if name in old and name in new else "only in one")
        print("%-10s %s" % (state, name))


if __name__ == "__main__":
    main(*sys.argv[1:3])
