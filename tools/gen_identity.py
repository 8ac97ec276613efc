#!/usr/bin/env python3
"""Fingerprints of the assembly generators' output, for refactors of fidget_amd/csrc/gen_*.py: the generated code object has to come out
byte for byte the same.  Builds interp_gfx950.s / .co from the generators of a csrc directory (this tree's by default, `--csrc` for a
checkout of another commit) in every configuration the generators know - the product build, the build without the compiled routines
(no _t kernels), each experiment switch, FH_BLKL=3 - and prints one line per configuration: name, sha1 of the .s, sha1 of the .co.
Run it on both commits and diff the two outputs.  `--normalise`: the .s sha1 is taken with the numbers of the `.L<stem>_<n>` local labels
replaced (they do not reach the object).  Needs trans_funcs.s as the build leaves it in csrc/_gen (the routines' source is no generator).

usage: gen_identity.py [--csrc DIR] [--trans FILE] [--out DIR] [--normalise]"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
EXPS = ["nosqrt", "twicesqrt", "nosin", "noexp", "twiceexp", "nodiv", "nofastdiv", "twicediv", "nodelta", "file64", "vgpr160", "nointerp",
        "compiledsincos", "prune_nolive", "nodiv,nosqrt"]
CONFIGS = [("product", {}, True), ("no routines", {}, False)] + [(f"FH_EXP={e}", {"FH_EXP": e}, True) for e in EXPS] + [("FH_BLKL=3", {"FH_BLKL": "3"}, True)]


def sha1(data):
    return hashlib.sha1(data).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(HERE, "..", "fidget_amd", "csrc"))
    ap.add_argument("--trans", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--normalise", action="store_true")
    args = ap.parse_args()
    csrc = os.path.abspath(args.csrc)
    trans = os.path.abspath(args.trans or os.path.join(HERE, "..", "fidget_amd", "csrc", "_gen", "trans_funcs.s"))
    out = os.path.abspath(args.out or tempfile.mkdtemp(prefix="gen_identity_"))
    os.makedirs(out, exist_ok=True)
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    subprocess.check_call(["g++", "-std=c++17", "-I", csrc, os.path.join(csrc, "offsets.cpp"), "-o", os.path.join(out, "offsets")])
    with open(os.path.join(out, "offsets.json"), "w") as f:
        subprocess.check_call([os.path.join(out, "offsets")], stdout=f)
    for i, (name, env, routines) in enumerate(CONFIGS):
        s, o, co = (os.path.join(out, f"c{i:02d}.{ext}") for ext in ("s", "o", "co"))
        e = {k: v for k, v in os.environ.items() if k not in ("FH_EXP", "FH_BLKL")}
        e.update(env)
        subprocess.check_call([sys.executable, os.path.join(csrc, "gen_interp.py"), os.path.join(out, "offsets.json"), s] + ([trans] if routines else []), env=e)
        subprocess.check_call([os.path.join(llvm, "clang"), "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", s, "-o", o])
        subprocess.check_call([os.path.join(llvm, "ld.lld"), "-shared", o, "-o", co])
        text = open(s, "rb").read()
        if args.normalise:
            text = re.sub(rb"(\.L[A-Za-z0-9_]*?_)\d+\b", rb"\1N", text)
        print(f"{name:24s} {sha1(text)} {sha1(open(co, 'rb').read())}", flush=True)


if __name__ == "__main__":
    main()
