#!/usr/bin/env python
"""tools/isa_stream_diff.py <git revision> file.hip [file.hip ...] [-DWAA_MEASURE] — per kernel of the named sources of csrc/: the
instruction count in that revision and in this tree, and whether the two instruction streams are identical once labels, symbol
names, directives and comments are stripped from the compiler's -S output.  Identical streams settle bit identity and speed of a
kernel outright.  (cross-compiles, no GPU; the companion of tools/kernel_resource_diff.py)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
T = os.path.join(tempfile.gettempdir(), "waa_isa_stream_diff")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero", "--cuda-device-only", "-S"]


def streams(path):
    out, cur = {}, None
    for ln in open(path):
        s = ln.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+):\s*$", s)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        t = s.strip()
        if cur is None or not t:
            continue
        if t.startswith((".amdhsa_kernel", ".section", ".rodata")):
            cur = None
            continue
        if t.startswith(".") or re.match(r"^[.\w$]+:$", t):
            continue
        cur.append(re.sub(r"_Z\w+", "SYM", re.sub(r"\.LBB\d+_\d+", "L", t)))
    return {k: v for k, v in out.items() if v}


def compile_s(src, inc, extra, out):
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + extra + ["-I" + inc, "-I" + ROOT + "/include", src, "-o", out],
                          stderr=subprocess.DEVNULL)
    return streams(out)


def main(argv):
    rev, files, extra = argv[0], [a for a in argv[1:] if not a.startswith("-")], [a for a in argv[1:] if a.startswith("-")]
    old = os.path.join(T, "old")
    os.makedirs(old, exist_ok=True)
    for f in subprocess.check_output(["git", "-C", ROOT, "ls-tree", "--name-only", rev, "web-audio-api-rs_amd/csrc/"]).decode().split():
        if f.endswith((".hpp", ".hip")):
            open(os.path.join(old, os.path.basename(f)), "wb").write(subprocess.check_output(["git", "-C", ROOT, "show", rev + ":" + f]))
    for f in files:
        a = compile_s(os.path.join(old, f), old, extra, os.path.join(T, "old_" + f + ".s"))
        b = compile_s(os.path.join(CSRC, f), CSRC, extra, os.path.join(T, "new_" + f + ".s"))
        for k in sorted(set(a) | set(b)):
            print("%-14s %-60s %s %6d  this tree %6d  %s" % (f, k[:60], rev, len(a.get(k, [])), len(b.get(k, [])),
                                                              "IDENTICAL" if a.get(k) == b.get(k) else "differs"))


if __name__ == "__main__":
    main(sys.argv[1:])
