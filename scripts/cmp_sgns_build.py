"""Compare the kernels of two trees (a parent and a change that must not alter them).

  python scripts/cmp_sgns_build.py asm PARENT_DIR NEW_DIR [--files STEMS] [--kernels REGEX]
      DIR/STEM.s = device assembly of csrc/STEM.hip (the Makefile's FLAGS plus
      --offload-device-only -S), for each of the comma-separated STEMS a tree has (default: the
      SGNS instantiation files come_sgns_vec{1,2,4,8}; a refactor may move kernels between files,
      so a tree's kernels are pooled over its files).  Kernels are matched by demangled name
      without the parameter list -- and without template arguments where the exact name is not in
      the other tree -- and a kernel's text is its label to .Lfunc_end, comments stripped, the
      function's index taken out of its block labels (.LBB<function>_<block>: the compiler numbers
      them by the function's position in the code object).  Prints, per kernel, whether the text
      is equal; exit status 1 unless both trees have the same kernels and every kernel whose name
      matches REGEX (default k_sgns_o2_stream) is identical and calls nothing.
  python scripts/cmp_sgns_build.py ru PARENT_DIR NEW_DIR [--files STEMS]
      DIR/ru_STEM.txt = output of `make resource-usage RU_SRCS=STEM.hip`.  Prints the parent / new
      table of VGPRs, SGPRs, scratch, occupancy and LDS bytes and marks new or grown scratch and
      any change of occupancy or LDS; exit status 1 on grown scratch, lower occupancy or other LDS.
  A kernel the parent has and REGEX does not match may be missing from the new tree (retired).
"""
import argparse
import os
import re
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("asm", "ru"))
ap.add_argument("parent")
ap.add_argument("new")
ap.add_argument("--files", default=",".join("come_sgns_vec%d" % n for n in (1, 2, 4, 8)))
ap.add_argument("--kernels", default="k_sgns_o2_stream")
args = ap.parse_args()
STEMS = args.files.split(",")


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True)
    short = [re.sub(r"^void come::|^come::|\([^()]*\)$", "", s) for s in p.stdout.split("\n")]
    return dict(zip(names, short))


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = re.sub(r"\s*;.*$", "", line.rstrip("\n")).rstrip()
        m = re.match(r"^(_Z\w+):$", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None and line.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif name is not None and line:
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def kernels(d):
    """demangled name -> text, over the tree's files"""
    out = {}
    for stem in STEMS:
        path = os.path.join(d, stem + ".s")
        if not os.path.exists(path):
            continue
        names = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M)))
        fn, dm = functions(path), demangle(names)
        out.update((dm[k], fn[k]) for k in names)
    return out


def resources(d):
    out = {}
    for stem in STEMS:
        path, cur, names = os.path.join(d, "ru_%s.txt" % stem), None, {}
        if not os.path.exists(path):
            continue
        for line in open(path):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = names.setdefault(m.group(1), {})
            m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|Occupancy|ScratchSize|LDS Size)"
                          r"( \[[^]]*\])?: (\d+)", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(3))
        dm = demangle(sorted(names))
        out.update((dm[k], v) for k, v in names.items())
    return out


def fmt(r):
    return "%4d %4d %4d %2d %6d" % (r["VGPRs"], r["TotalSGPRs"], r["ScratchSize"], r["Occupancy"],
                                    r.get("LDS Size", 0))


load = kernels if args.mode == "asm" else resources
ta, tb = load(args.parent), load(args.new)
# the other tree's name for a kernel: the same, or the same without template arguments (a template
# that became a plain kernel) -- kernels matching REGEX choose first, no name is given twice
partner = {}
for k in sorted(ta, key=lambda k: (re.search(args.kernels, k) is None, k)):
    base = re.sub(r"<.*>$", "", k)
    free = [n for n in (k, base) if n in tb and n not in partner.values()]
    partner[k] = free[0] if free else None
pairs = [(k, partner[k]) for k in sorted(ta)]
extra = sorted(set(tb) - set(partner.values()))
ok = bool(ta) and not extra  # no kernel found: wrong directories or --files
for k, p in pairs:
    must = re.search(args.kernels, k) is not None
    if p is None:
        print("  %-46s only in the parent%s" % (k, "  FAIL" if must else " (retired)"))
        ok &= not must
    elif args.mode == "asm":
        same = ta[k] == tb[p]
        calls = sum(1 for line in tb[p] if re.match(r"\s*s_(swappc|call)_b64", line))
        print("  %-46s %6d -> %6d lines%s%s" % (k, len(ta[k]), len(tb[p]),
                                                "  identical" if same else "",
                                                "  %d calls" % calls if calls else ""))
        ok &= (same and not calls) or not must
    else:
        x, y = ta[k], tb[p]
        note = " scratch up" if y["ScratchSize"] > x["ScratchSize"] else ""
        note += " occupancy %+d" % (y["Occupancy"] - x["Occupancy"]) \
            if y["Occupancy"] != x["Occupancy"] else ""
        note += " LDS changed" if y.get("LDS Size", 0) != x.get("LDS Size", 0) else ""
        print("  %-46s %s   %s %s" % (k, fmt(x), fmt(y), note))
        ok &= not ("scratch up" in note or "LDS" in note or y["Occupancy"] < x["Occupancy"])
for k in extra:
    print("  %-46s only in the new tree" % k)
print("FAIL" if not ok else "no scratch gained, no occupancy lost, LDS equal" if args.mode == "ru"
      else "kernels matching %r identical, same kernels in both trees" % args.kernels)
sys.exit(0 if ok else 1)
