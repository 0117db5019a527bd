#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of the same libraries, kernel by kernel: the resources from the
code-object metadata (rtlws.codeobj) and the llvm-objdump -d text with addresses, raw encodings and the padding behind
a kernel's last instruction left out.  No GPU is used.

    tools/codeobj_compare.py PARENT_LIB_DIR NEW_LIB_DIR NAME [NAME ...]      NAME: fmbank for librtlws_fmbank.so
    tools/codeobj_compare.py --host PARENT_BUILD_DIR NEW_BUILD_DIR UNIT [UNIT ...]      UNIT: fmbank_shim for fmbank_shim.o

Prints one table per library (the form of profiles/ddc_family_codeobj.txt) and exits 1 when a kernel both builds have
differs.  --host compares the host side of object files instead: the objdump -d text of every function, with addresses
and raw encodings left out, and the sizes of .text and .rodata*."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rtl-ws_amd"))
from rtlws import codeobj                                                                      # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def listing(lib):
    """kernel symbol -> its instructions, one string each"""
    out = {}
    for img in codeobj.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as tf:
            tf.write(img)
            tf.flush()
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", tf.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            if cur is None or not line.strip():
                continue
            ins = re.sub(r"\s*//.*$", "", line).strip()                    # the address comment behind an instruction
            ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
            cur.append(ins)
    for ins in out.values():                                               # the padding behind the last instruction
        while ins and (ins[-1] == "..." or ins[-1].startswith(("s_code_end", "s_nop"))):
            ins.pop()
    return out


def host_listing(obj):
    """function symbol -> its host instructions, one string each; and the sizes of the sections that hold code and words"""
    txt = subprocess.run(["objdump", "-d", "-r", "--no-show-raw-insn", obj], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"^\s*[0-9a-f]+:\s*", "", line).strip())
    sizes = {}
    for line in subprocess.run(["size", "-A", obj], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if len(f) == 3 and (f[0].startswith(".text") or f[0].startswith(".rodata")):
            sizes[f[0]] = sizes.get(f[0], 0) + int(f[1])
    return out, sizes


def host_main(parent_dir, new_dir, units):
    same = True
    for u in units:
        (a, sa), (b, sb) = [host_listing(os.path.join(d, u + ".o")) for d in (parent_dir, new_dir)]
        differing = sum(a.get(f) != b.get(f) for f in set(a) | set(b))
        ok = differing == 0 and sa == sb
        same = same and ok
        print("%-16s host side: %3d functions, %5d instruction lines, .text + .rodata %6d bytes | %s"
              % (u + ".o", len(b), sum(len(v) for v in b.values()), sum(sb.values()),
                 "identical to the parent's" if ok else "DIFFERS: %d functions, sections %s against %s" % (differing, sa, sb)))
    return 0 if same else 1


def resources(k):
    return (k["vgpr_count"], k.get("agpr_count", 0), k["sgpr_count"], k.get("group_segment_fixed_size", 0),
            k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0) + k.get("sgpr_spill_count", 0))


def short(name):
    return name.replace("rtlws::", "")


def main(parent_dir, new_dir, names):
    same = True
    for n in names:
        libs = [os.path.join(d, "librtlws_%s.so" % n) for d in (parent_dir, new_dir)]
        meta = [{k["name"]: k for k in codeobj.kernels(lib)} for lib in libs]
        text = [listing(lib) for lib in libs]
        print("librtlws_%s.so: %d kernels in the parent's build, %d in the new one" % (n, len(meta[0]), len(meta[1])))
        print("%-62s | parent vgpr agpr sgpr lds scr spill  | new    vgpr agpr sgpr lds scr spill  | disassembly" % "kernel")
        for sym in sorted(set(meta[0]) | set(meta[1]), key=lambda s: meta[0].get(s, meta[1].get(s)).get("demangled", s)):
            k = meta[0].get(sym) or meta[1].get(sym)
            cols = ["  %4d %4d %4d %6d %3d %3d       " % resources(m[sym]) if sym in m else "  %-35s" % "absent" for m in meta]
            if sym in meta[0] and sym in meta[1]:
                a, b = text[0][sym], text[1][sym]
                differing = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
                ok = differing == 0 and resources(meta[0][sym]) == resources(meta[1][sym])
                same = same and ok
                verdict = "identical (%d instructions)" % len(a) if ok else "DIFFERS: %d of %d | %d lines" % (differing, len(a), len(b))
            else:
                verdict = "only in one build"
                same = False
            print("%-62s |%s|%s| %s" % (short(k.get("demangled", sym))[:62], cols[0], cols[1], verdict))
        print()
    return 0 if same else 1


if __name__ == "__main__":
    if sys.argv[1] == "--host":
        sys.exit(host_main(sys.argv[2], sys.argv[3], sys.argv[4:]))
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
