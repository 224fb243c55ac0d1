#!/usr/bin/env python3
"""Compare two ISA listings of one kernel file, kernel by kernel.

    hipcc ... --cuda-device-only -S -Rpass-analysis=kernel-resource-usage lstm_scan.hip -o before.s 2> before.remarks
    (the same on the changed source: after.s)
    tools/compare_kernel_isa.py before.s after.s --match lstm_scan_fwd_split \\
        --equal mfma buffer_load store atomic barrier --out profiles/some_refactor_isa.json

Kernels whose demangled name contains --match are the ones under change: for each, the resources the assembler
recorded (registers, scratch, LDS, occupancy), the instruction count and the histogram of whatever opcodes the
listing holds are written for both builds, with the opcodes whose counts differ.  The script fails if one of them
has scratch, if LDS or occupancy differ, or if the summed count of the opcodes containing one of the --equal
substrings differs.  Every OTHER kernel must come out as identical text, local label names aside.
"""
import argparse
import collections
import json
import re
import subprocess
import sys

RESOURCES = {"vgpr": "NumVgprs", "agpr": "NumAgprs", "sgpr": "TotalNumSgprs", "scratch": "ScratchSize",
             "lds": "LDSByteSize", "occupancy": "Occupancy"}


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.split("\n")))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def kernels(path):
    """name -> (instruction lines, resource dict) for every kernel of the listing"""
    out, name, body = {}, None, []
    kernel_names = set()
    lines = open(path).read().split("\n")
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kernel_names.add(m.group(1))
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"(\w+):", ln)
        if m and m.group(1) in kernel_names and name is None:
            name, body = m.group(1), []
        elif name is not None:
            if re.match(r"\.Lfunc_end\d+:", ln):
                res = {}
                for j in range(i, min(i + 80, len(lines))):
                    for key, tag in RESOURCES.items():
                        mm = re.match(r";\s*%s:\s*(\d+)" % tag, lines[j])
                        if mm and key not in res:
                            res[key] = int(mm.group(1))
                out[name] = (body, res)
                name = None
            else:
                code = ln.split(";")[0].rstrip()
                if code.strip() and not code.lstrip().startswith("."):      # (directives and local labels start with a dot)
                    body.append(code.strip())
                elif re.match(r"\.L\w+:", code.strip()):
                    body.append(code.strip())
        i += 1
    return out


def normalised(body):
    """the text with local labels renumbered in order of appearance"""
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), ".L%d" % len(seen))
    return [re.sub(r"\.L\w+", sub, ln) for ln in body]


def histogram(body):
    return collections.Counter(ln.split()[0] for ln in body if not ln.startswith(".L"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--match", required=True, help="substring of the demangled names of the kernels under change")
    ap.add_argument("--equal", nargs="*", default=[], help="opcode substrings whose summed counts must not change")
    ap.add_argument("--out", help="JSON file for the per-kernel table")
    args = ap.parse_args()
    kb, ka = kernels(args.before), kernels(args.after)
    names = demangle(sorted(set(kb) | set(ka)))
    failures, table, untouched = [], {}, 0
    for mangled in sorted(names, key=names.get):
        nice = re.sub(r"^void \(anonymous namespace\)::|\(KlScan\w+\)$", "", names[mangled])
        if args.match not in nice:
            if mangled not in kb or mangled not in ka:
                failures.append("%s: only in one build" % nice)
            elif normalised(kb[mangled][0]) != normalised(ka[mangled][0]):
                failures.append("%s: outside --match, but its ISA differs" % nice)
            else:
                untouched += 1
            continue
        row = {}
        for tag, k in (("before", kb), ("after", ka)):
            if mangled in k:
                body, res = k[mangled]
                h = histogram(body)
                row[tag] = dict(res, instructions=sum(h.values()), opcodes=dict(sorted(h.items())))
        if "before" in row and "after" in row:
            b, a = row["before"], row["after"]
            row["opcode_differences"] = {op: [b["opcodes"].get(op, 0), a["opcodes"].get(op, 0)]
                                         for op in sorted(set(b["opcodes"]) | set(a["opcodes"]))
                                         if b["opcodes"].get(op, 0) != a["opcodes"].get(op, 0)}
            row["register_differences"] = {r: [b.get(r), a.get(r)] for r in ("vgpr", "agpr", "sgpr") if b.get(r) != a.get(r)}
            for r in ("lds", "occupancy"):
                if b.get(r) != a.get(r):
                    failures.append("%s: %s %s -> %s" % (nice, r, b.get(r), a.get(r)))
            for sub in args.equal:
                cb = sum(n for op, n in b["opcodes"].items() if sub in op)
                ca = sum(n for op, n in a["opcodes"].items() if sub in op)
                if cb != ca:
                    failures.append("%s: '%s' opcodes %d -> %d" % (nice, sub, cb, ca))
        else:
            row["only_in"] = "before" if "before" in row else "after"
        for tag in ("before", "after"):
            if tag in row and row[tag].get("scratch", 0) != 0:
                failures.append("%s: scratch %d bytes (%s)" % (nice, row[tag]["scratch"], tag))
        table[nice] = row
    for nice, row in table.items():
        if "only_in" in row:
            print("%-52s only in '%s'" % (nice, row["only_in"]))
            continue
        b, a = row["before"], row["after"]
        print("%-52s vgpr %3d/%3d agpr %3d/%3d scratch %d/%d lds %5d/%5d occ %d/%d instr %4d -> %4d  %s" % (
            nice, b["vgpr"], a["vgpr"], b["agpr"], a["agpr"], b["scratch"], a["scratch"], b["lds"], a["lds"],
            b["occupancy"], a["occupancy"], b["instructions"], a["instructions"],
            " ".join("%s:%d>%d" % (op, x, y) for op, (x, y) in row["opcode_differences"].items())))
    print("%d kernels outside '%s' identical" % (untouched, args.match))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"match": args.match, "equal_substrings": args.equal, "untouched_identical": untouched,
                       "failures": failures, "kernels": table}, f, indent=1, sort_keys=True)
            f.write("\n")
    for msg in failures:
        print("FAIL", msg)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
