#!/usr/bin/env python3
"""CPU: compare the gfx950 ISA of two csrc/ trees, kernel by kernel (no GPU needed; hipcc cross-compiles).

    python tools/isa_diff.py PARENT_CSRC NEW_CSRC [--files a.hip b.hip ...] > profiles/<name>.txt

Every conv translation unit (or --files) of both trees is compiled with lib.HIPCC_FLAGS (minus -shared) plus `-S --cuda-device-only`,
the recipe of tests/test_isa_counted_waits.py, and for every kernel symbol the script reports
  * `identical`            the instruction text is the same once labels, symbol names and comments are stripped;
  * `identical (kernarg)`  the same up to the immediate offsets of `s_load_*` from the kernarg pointer and .kernarg_segment_size
                           (what removing a field of a by-value argument struct moves, and nothing else);
  * otherwise the resource metadata and the instruction histogram of both sides, with `!=` on every line that differs, and whether
    the two bodies at least consist of the same instructions (equal multiset of mnemonics).
Kernels that exist on one side only are listed (--rename maps a parent symbol whose template parameter list changed onto the new one).
The options of the run are printed in the first lines, so that a committed output names the command that made it.
Exit status 1 if a kernel of both trees has a higher VGPR / AGPR / SGPR count, other scratch or LDS, another register-implied occupancy,
other MFMA / VMEM / LDS / barrier / hand-written wait counts or more VALU / SALU instructions, or if a kernel exists only in NEW."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hover_net_amd.lib import HIPCC_FLAGS  # noqa: E402

# the ten matrix-pipe translation units + the two other files that use csrc/hvn_conv_common.h
CONV_FILES = ("hvn_conv.hip", "hvn_conv_x3.hip", "hvn_conv_x3g.hip", "hvn_conv_bf16.hip", "hvn_conv_bf16g.hip", "hvn_conv_chain.hip",
              "hvn_conv_chain_bf16.hip", "hvn_conv_chain_x3.hip", "hvn_conv_chain_x3r.hip", "hvn_wgrad_x3.hip", "hvn_train.hip", "hvn_net_ops.hip")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size",
        ".max_flat_workgroup_size")
HIGHER_FAILS = (".vgpr_count", ".agpr_count", ".sgpr_count")                                   # a lower count is no regression
MUST_EQUAL = (".private_segment_fixed_size", ".group_segment_fixed_size", "waves_per_simd")
# histogram classes: (name, regex on the mnemonic [+ operands]); the first that matches takes the instruction
CLASSES = (("v_mfma", r"^v_mfma_"), ("buffer_load_lds", r"^buffer_load_\S+ .*\blds$"), ("buffer_load", r"^buffer_load_"),
           ("buffer_store", r"^buffer_store_"), ("global", r"^global_"), ("scratch", r"^scratch_"), ("flat", r"^flat_"),
           ("ds_read", r"^ds_read"), ("ds_write", r"^ds_write"), ("s_barrier", r"^s_barrier"))
GATED = ("v_mfma", "buffer_load_lds", "buffer_load", "buffer_store", "global", "scratch", "flat", "ds_read", "ds_write", "s_barrier", "asm_waits")


def compile_s(csrc, name, out):
    flags = [f for f in HIPCC_FLAGS if f != "-shared"]
    subprocess.run(["hipcc", *flags, "-I" + csrc, "-S", "--cuda-device-only", "-o", out, os.path.join(csrc, name)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read().split("\n")


def parse(lines):
    """-> {kernel symbol: {"meta": {...}, "text": [normalised instructions], "hist": {...}}}"""
    kernels = {}
    names = [m.group(1) for l in lines for m in [re.match(r"\s+\.amdhsa_kernel (\S+)", l)] if m]
    start = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\w+):", l)] if m and m.group(1) in names}
    for name in names:
        body, labels, waits, in_app = [], {}, [], False
        for l in lines[start[name] + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            s = l.split(";")[0].strip() if not l.lstrip().startswith(";") else ""
            if l.strip() in (";;#ASMSTART", ";;#ASMEND"):     # inline assembly: the hand-written waits
                in_app = l.strip() == ";;#ASMSTART"
                continue
            if not s or s.startswith(".") and not s.endswith(":"):
                continue                                  # directives (.p2align, .loc, ...)
            s = re.sub(r"\s+", " ", s)
            s = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), s)
            s = s.replace(name, "KERNEL")
            if in_app and s.startswith("s_waitcnt"):
                waits.append(s[len("s_waitcnt "):])
            body.append(s)
        hist = {c: 0 for c, _ in CLASSES}
        hist.update({"v_total": 0, "s_total": 0})
        for s in body:
            if s.endswith(":"):
                continue
            for c, rx in CLASSES:
                if re.match(rx, s):
                    hist[c] += 1
                    break
            if s.startswith("v_"):
                hist["v_total"] += 1
            elif s.startswith("s_"):
                hist["s_total"] += 1
        hist["asm_waits"] = " ".join("%s x%d" % (w, waits.count(w)) for w in sorted(set(waits))) or "-"
        kernels[name] = {"text": body, "hist": hist, "meta": {}}
    # the metadata note: one YAML list entry per kernel
    try:
        i = next(k for k, l in enumerate(lines) if l.startswith("amdhsa.kernels:"))
    except StopIteration:
        return kernels
    entry = {}
    for l in lines[i + 1:]:
        if l.startswith("  - ") or not l.startswith("  "):
            if entry.get(".name") in kernels:
                kernels[entry[".name"]]["meta"] = entry
            entry = {}
            if not l.startswith("  "):
                break
        m = re.match(r"^(?:  - |    )(\.\w+):\s+(\S+)\s*$", l)
        if m:
            entry[m.group(1)] = m.group(2)
    for k in kernels.values():
        k["meta"] = {m: int(k["meta"].get(m, "0")) for m in META}
        k["meta"]["waves_per_simd"] = waves(k["meta"])
    return kernels


def waves(meta):
    """Waves per SIMD the register file allows (gfx950: 512 unified VGPR + AGPR per lane, granule 8, at most 8 waves).  LDS and the
    launch bounds can only lower it further, by the same amount on both sides when .group_segment_fixed_size and the bounds are equal."""
    regs = meta[".vgpr_count"] + meta[".agpr_count"]
    regs = max(8, (regs + 7) // 8 * 8)
    return min(8, 512 // regs)


def strip_kernarg(text):
    return [re.sub(r"^(s_load_dword\w* \S+ s\[\d+:\d+\],) 0x[0-9a-f]+$", r"\1 KARG", s) for s in text]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--files", nargs="*", default=list(CONV_FILES))
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="rewrite PARENT kernel symbols before matching (a kernel whose template parameter list changed keeps its partner)")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="isa_diff_")
    jobs = [(side, csrc, f) for f in a.files for side, csrc in (("parent", a.parent), ("new", a.new))]
    with ThreadPoolExecutor(max_workers=a.jobs) as ex:
        res = list(ex.map(lambda j: parse(compile_s(j[1], j[2], os.path.join(tmp, "%s_%s.s" % (j[0], j[2])))), jobs))
    bad = 0
    counts = {"identical": 0, "identical (kernarg)": 0, "differs": 0}
    print("# tools/isa_diff.py: gfx950, flags: %s -S --cuda-device-only" % " ".join(f for f in HIPCC_FLAGS if f != "-shared"))
    print("# python tools/isa_diff.py PARENT_CSRC NEW_CSRC --files %s%s" % (" ".join(a.files), "".join(" --rename '%s'" % r for r in a.rename)))
    for n, f in enumerate(a.files):
        old, new = res[2 * n], res[2 * n + 1]
        for r in a.rename:
            rx, repl = r.split("=", 1)
            old = {re.sub(rx, repl, k): v for k, v in old.items()}
        print("\n== %s: %d kernels in parent, %d in new" % (f, len(old), len(new)))
        for k in sorted(set(old) - set(new)):
            print("only in parent: %s" % k)
        for k in sorted(set(new) - set(old)):
            print("only in new:    %s   <-- FAIL" % k)
            bad += 1
        for k in sorted(set(old) & set(new)):
            o, w = old[k], new[k]
            if o["text"] == w["text"] and o["meta"] == w["meta"]:
                print("identical: %s" % k)
                counts["identical"] += 1
                continue
            mo = {m: v for m, v in o["meta"].items() if m != ".kernarg_segment_size"}
            mw = {m: v for m, v in w["meta"].items() if m != ".kernarg_segment_size"}
            if strip_kernarg(o["text"]) == strip_kernarg(w["text"]) and mo == mw:
                print("identical (kernarg): %s   [.kernarg_segment_size %d -> %d]" % (k, o["meta"][".kernarg_segment_size"], w["meta"][".kernarg_segment_size"]))
                counts["identical (kernarg)"] += 1
                continue
            counts["differs"] += 1
            fail = []
            print("DIFFERS: %s" % k)
            for m in list(META) + ["waves_per_simd"]:
                ne = o["meta"][m] != w["meta"][m]
                print("    %-30s %8d %8d %s" % (m, o["meta"][m], w["meta"][m], "!=" if ne else ""))
                if ne and m in MUST_EQUAL:
                    fail.append(m)
                if m in HIGHER_FAILS and w["meta"][m] > o["meta"][m]:
                    fail.append(m + " higher")
            for c in list(o["hist"]):
                ne = o["hist"][c] != w["hist"][c]
                print("    %-30s %8s %8s %s" % (c, o["hist"][c], w["hist"][c], "!=" if ne else ""))
                if ne and c in GATED:
                    fail.append(c)
                if c in ("v_total", "s_total") and w["hist"][c] > o["hist"][c]:
                    fail.append(c + " higher")
            print("    instructions                   %8d %8d" % (sum(1 for s in o["text"] if not s.endswith(":")), sum(1 for s in w["text"] if not s.endswith(":"))))
            mn = lambda t: sorted(s.split(" ")[0] for s in t if not s.endswith(":"))
            print("    same instructions (mnemonic multiset; order, registers and operand order aside): %s" % ("yes" if mn(o["text"]) == mn(w["text"]) else "no"))
            if fail:
                print("    FAIL: %s" % ", ".join(fail))
                bad += 1
    print("\n# summary: %d identical, %d identical up to kernarg offsets, %d differ, %d fail" % (counts["identical"], counts["identical (kernarg)"], counts["differs"], bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
