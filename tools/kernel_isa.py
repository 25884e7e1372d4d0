#!/usr/bin/env python3
"""One line per GPU kernel of the given .hip sources: what a refactor of a kernel file must leave unchanged.

    python tools/kernel_isa.py xworld_amd/csrc/kernels_xworld_ego.hip [more.hip ...] > after.txt
    python tools/kernel_isa.py --root /path/to/other/tree xworld_amd/csrc/kernels_xworld_ego.hip > before.txt
    diff before.txt after.txt

Each source is compiled for the device only (hipcc <xworld_amd.build.FLAGS> --cuda-device-only -S; no GPU needed) and the
assembly is cut at the .amdhsa_kernel symbols.  Per kernel: mangled name, sha256[:16] of its instruction text, VGPRs,
SGPRs, LDS bytes, scratch bytes; sorted by name.  Local labels carry a per-file function index (.LBB<n>_<m>,
.Lfunc_end<n>, ...): it is replaced, so a kernel hashes the same whichever file it is compiled in.  Extra compiler flags
(a lab build: -DXWB_EGO_PROF) go after `--`.  --root: the tree the relative source paths (and include paths) belong to;
the flags always come from this tree's xworld_amd.build.
"""
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xworld_amd.build import FLAGS, hipcc  # noqa: E402

LOCAL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")
META = {"vgpr": ".amdhsa_next_free_vgpr", "sgpr": ".amdhsa_next_free_sgpr", "lds": ".amdhsa_group_segment_fixed_size",
        "scratch": ".amdhsa_private_segment_fixed_size"}


def kernels_of(asm):
    """{name: (instruction text, {vgpr, sgpr, lds, scratch})} of one device assembly listing"""
    lines = asm.splitlines()
    names, meta = [], {}
    for i, ln in enumerate(lines):
        if ln.strip().startswith(".amdhsa_kernel "):
            name = ln.split()[1]
            names.append(name)
            m = {}
            for nxt in lines[i + 1:]:
                t = nxt.split()
                if t and t[0] == ".end_amdhsa_kernel":
                    break
                for key, directive in META.items():
                    if t and t[0] == directive:
                        m[key] = t[1]
            meta[name] = m
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        body = []
        for ln in lines[start + 1:]:
            s = ln.split(";")[0].strip()                    # (comments hold file paths and line numbers)
            if s.startswith(".Lfunc_end"):
                break
            if not s or (s.startswith(".") and not s.startswith(".L")):
                continue                                    # directives: .p2align, .loc, .cfi_...
            body.append(LOCAL.sub(lambda m: ".L" + m.group(1) + "N" + (m.group(3) or ""), s))
        out[name] = ("\n".join(body), meta[name])
    return out


def main(argv):
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    root = os.getcwd()
    if argv and argv[0] == "--root":
        root, argv = argv[1], argv[2:]
    if not argv:
        sys.exit(__doc__)
    rows = {}
    for src in argv:
        cmd = [hipcc()] + FLAGS + extra + ["--cuda-device-only", "-S", os.path.join(root, src), "-o", "-"]
        asm = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
        for name, (text, m) in kernels_of(asm).items():
            if name in rows:
                sys.exit("kernel %s is defined in two of the sources" % name)
            rows[name] = "%s %s vgpr=%s sgpr=%s lds=%s scratch=%s" % (
                name, hashlib.sha256(text.encode()).hexdigest()[:16], m.get("vgpr"), m.get("sgpr"), m.get("lds"), m.get("scratch"))
    for name in sorted(rows):
        print(rows[name])


if __name__ == "__main__":
    main(sys.argv[1:])
