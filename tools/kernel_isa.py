#!/usr/bin/env python3
"""Per-kernel ISA digests of csrc/*.hip (gfx950), for refactors that must not change a kernel.

    python tools/kernel_isa.py dump  out.json     # {demangled kernel name: sha1 of its normalised instruction stream}
    python tools/kernel_isa.py diff  a.json b.json  # kernel for kernel; flavour kernels under their folded name (FOLDED)

Every .hip file is compiled device-only to assembly (`hipcc -S --cuda-device-only`, the Makefile's flags); a kernel's
text is what lies between its label and its `.Lfunc_end`; local labels (`.LBB<function>_<block>`) are renumbered
by function so that moving a kernel to another translation unit changes nothing.  Registers, metadata
(`.vgpr_count`, LDS size) and the instruction text are all part of the digest."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "easygaussiansplatting_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fno-slp-vectorize",
         "-Wno-unused-function"]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                         text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels_of(asm):
    """{mangled name: normalised text} for every function with an .amdhsa_kernel descriptor"""
    kern = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res = {}
    for name in kern:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.section\s+\.rodata" % re.escape(name), asm, re.M | re.S)
        if not m:
            continue
        body = m.group(1)
        body = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", body)
        body = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", body)
        body = re.sub(r"\.Ltmp\d+", ".Ltmp", body)
        body = "\n".join(ln.split(";")[0].rstrip() for ln in body.split("\n") if ln.strip() and not ln.strip().startswith(";"))
        d = re.search(r"^\s*\.amdhsa_kernel\s+%s\s*\n(.*?)\.end_amdhsa_kernel" % re.escape(name), asm, re.M | re.S)
        desc = "\n".join(ln.strip() for ln in d.group(1).split("\n")
                         if any(k in ln for k in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size",
                                                  "private_segment_fixed_size", "accum_offset"))) if d else ""
        res[name] = body + "\n" + desc
    return res


def dump(out_path, sources=None):
    srcs = sources or sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    table = {}
    with tempfile.TemporaryDirectory() as td:
        for f in srcs:
            s = os.path.join(td, f + ".s")
            subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-S", "--cuda-device-only", os.path.join(CSRC, f), "-o", s],
                           check=True)
            ks = kernels_of(open(s).read())
            dm = demangle(list(ks))
            for k, body in ks.items():
                nm = dm[k]
                assert nm not in table, "kernel defined twice: " + nm
                table[nm] = {"sha1": hashlib.sha1(body.encode()).hexdigest(), "lines": body.count("\n"), "file": f}
    json.dump(table, open(out_path, "w"), indent=1, sort_keys=True)
    print("%d kernels -> %s" % (len(table), out_path))


# A kernel flavour used to be a kernel NAME (k_draw_extra<..>), now it is a template argument (k_draw<.., true>):
# old flavour name -> (folded name, template arguments it had, template arguments the fold appends).  A kernel that
# gained a trailing template argument later has one more rule in FOLDED_AGAIN, applied to the name the first gave.
FOLDED = {
    "k_preprocess_fwd": ("k_preprocess_fwd", 3, ["false"]),                         # <NC, RAW, JW> + AA
    "k_preprocess_fwd_aa": ("k_preprocess_fwd", 3, ["true"]),
    "k_preprocess_bwd": ("k_preprocess_bwd", 3, ["false", "false", "false"]),       # <NC, RAW, JW> + EXTRA, POSE, AA
    "k_preprocess_bwd_extra": ("k_preprocess_bwd", 3, ["true", "false", "false"]),
    "k_preprocess_bwd_pose": ("k_preprocess_bwd", 4, ["true", "false"]),            # <NC, RAW, JW, EXTRA>
    "k_preprocess_bwd_aa": ("k_preprocess_bwd", 5, ["true"]),                       # <NC, RAW, JW, EXTRA, POSE>
    "k_viewer_prep": ("k_viewer_prep", 1, ["false"]),                               # <NC> + AA
    "k_viewer_prep_aa": ("k_viewer_prep", 1, ["true"]),
    "k_draw": ("k_draw", 4, ["false"]),                                             # <BOX, FLOOR, CLAMP, SKIP> + EXTRA
    "k_draw_extra": ("k_draw", 4, ["true"]),
    "k_draw_bwd": ("k_draw_bwd", 5, ["false"]),                                     # <BOX, FLOOR, CLAMP, RED, SEG> + EXTRA
    "k_draw_bwd_extra": ("k_draw_bwd", 4, ["false", "true"]),                       # <BOX, FLOOR, CLAMP, RED>
}
FOLDED_AGAIN = {
    "k_draw_bwd": (6, ["false"]),                                    # <BOX, FLOOR, CLAMP, RED, SEG, EXTRA> + ABS
    "k_preprocess_bwd": (6, ["false"]),                              # <NC, RAW, JW, EXTRA, POSE, AA> + POSE_ONLY
}
# A template argument that was retired at its only surviving value: kernel -> (index, that value).  A name whose argument
# there is still a number is an older dump's: it takes the folds above and, at that value, loses the argument; the
# instances of the other values keep their names and are reported "only in a".  Today's names take no fold.
DROPPED = {
    "k_draw_bwd": (3, "7"),                                          # <BOX, FLOOR, CLAMP, RED, SEG, EXTRA, ABS> - RED
}


def canonical(name):
    """The name a kernel is compared under: a flavour kernel of an older dump gets the name of the template instance
    it was folded into, so that a dump from before the fold and one from after it compare kernel for kernel.  The
    parameter list is dropped for these kernels (the fold gave every instance the flavours' trailing arguments); any
    other name is returned as it is."""
    m = re.match(r"void egs::(\w+)<(.*?)>\(", name)
    if not m or m.group(1) not in FOLDED:
        return name
    base, args = m.group(1), [x.strip() for x in m.group(2).split(",")]
    dropped = DROPPED.get(FOLDED[base][0])
    if dropped and not args[dropped[0]].isdigit():
        return "%s<%s>" % (base, ", ".join(args))
    new_base, arity, appended = FOLDED[base]
    if len(args) == arity:
        base, args = new_base, args + appended
    if base in FOLDED_AGAIN and len(args) == FOLDED_AGAIN[base][0]:
        args = args + FOLDED_AGAIN[base][1]
    if dropped and args[dropped[0]] == dropped[1]:
        del args[dropped[0]]
    return "%s<%s>" % (base, ", ".join(args))


def load(path):
    table = {}
    for k, v in json.load(open(path)).items():
        assert canonical(k) not in table, "two kernels map to " + canonical(k)
        table[canonical(k)] = v
    return table


def diff(a, b):
    A, B = load(a), load(b)
    bad = added = 0
    for k in sorted(set(A) | set(B)):
        if k not in A: print("only in b:", k); added += 1     # (a feature adds kernels: reported, not an error)
        elif k not in B: print("only in a:", k); bad += 1
        elif A[k]["sha1"] != B[k]["sha1"]:
            print("DIFFERENT (%d vs %d lines): %s" % (A[k]["lines"], B[k]["lines"], k)); bad += 1
    print("%d kernels compared, %d differ, %d only in b" % (len(set(A) & set(B)), bad, added))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3:] or None)
    else:
        sys.exit(diff(sys.argv[2], sys.argv[3]))
