#!/usr/bin/env python3
"""Device-side assembly of the engine's HIP sources, for proving a refactor behaviour-neutral.

    python tools/device_asm.py OUTDIR [-DNAME=VALUE ...] [--only c4_engine.hip,c4_net.hip] [--per-kernel]

Compiles every source of __graft_entry__.ENGINE_HIP (or the ones named by --only) for the device only, to
OUTDIR/<name>.s, with the real build's flags (HIP_FLAGS without -shared/-fPIC) plus any -D given here, and
prints one sha256 per source.  Apart from the compile-unit id (removed, see CUID) the assembly holds no paths
or line numbers, so two trees that print the same hash run the same kernels.  CPU only; one c4_engine.hip compile takes minutes, so this is a
developer aid and no test calls it.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import ENGINE_HIP, HIP_FLAGS, HIPCC, ROOT  # noqa: E402

# the compile-unit id symbol is a hash of the command line (source and output paths included): the one name in the
# assembly that depends on where the tree and OUTDIR are, so its digits are dropped before hashing
CUID = re.compile(rb"__hip_cuid_[0-9a-f]+")   # (up to 16 digits: leading zeros are not printed)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("outdir")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME[=VALUE]")
    ap.add_argument("--only", default="", help="comma-separated source file names (default: all)")
    ap.add_argument("--per-kernel", action="store_true", help="also print one sha256 per kernel symbol")
    args = ap.parse_args()
    only = [n for n in args.only.split(",") if n]
    unknown = set(only) - {os.path.basename(s) for s in ENGINE_HIP}
    if unknown:
        ap.error("not in ENGINE_HIP: %s" % ", ".join(sorted(unknown)))
    os.makedirs(args.outdir, exist_ok=True)
    flags = [f for f in HIP_FLAGS if f not in ("-shared", "-fPIC")] + ["--cuda-device-only", "-S"]
    flags += ["-D" + d for d in args.defines]
    for src in ENGINE_HIP:
        name = os.path.basename(src)
        if only and name not in only:
            continue
        out = os.path.join(args.outdir, os.path.splitext(name)[0] + ".s")
        subprocess.check_call([HIPCC] + flags + ["-o", out, src], cwd=ROOT)
        with open(out, "rb") as f:
            text = CUID.sub(b"__hip_cuid_", f.read())
        with open(out, "wb") as f:
            f.write(text)
        print("%s  %s" % (hashlib.sha256(text).hexdigest(), name), flush=True)
        if args.per_kernel:
            per_kernel(text)


# labels and the loop comments carry the function's ordinal in the file (.LBB12_3, BB12_3, .Lfunc_end12), which moves with
# the order of instantiation
ORDINAL = re.compile(rb"(BB|func_begin|func_end)\d+")


def per_kernel(text):
    """One sha256 per kernel: from its function label to the end of its .amdhsa_kernel block, ordinals dropped."""
    for m in sorted(re.finditer(rb"^\s*\.amdhsa_kernel (\S+)$", text, re.M), key=lambda m: m.group(1)):
        sym = m.group(1)
        start = text.index(b"\n" + sym + b":")
        end = text.index(b".end_amdhsa_kernel", m.end())
        body = ORDINAL.sub(rb"\1", text[start:end])
        print("  %s  %s" % (hashlib.sha256(body).hexdigest(), sym.decode()), flush=True)


if __name__ == "__main__":
    main()
