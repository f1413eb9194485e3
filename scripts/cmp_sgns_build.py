"""Compare the SGNS kernels of two trees (a parent and a change that must not alter them).

  python scripts/cmp_sgns_build.py asm PARENT_DIR NEW_DIR
      DIR/vec{1,2,4,8}.s = device assembly of csrc/come_sgns_vecN.hip (the Makefile's FLAGS plus
      --offload-device-only -S).  Prints whether the .amdhsa_kernel symbol sets are equal and, per
      kernel, whether the text from its label to .Lfunc_end (comments stripped) is; exit status 1
      unless the sets are equal and every k_sgns_o2_stream instantiation is identical.
  python scripts/cmp_sgns_build.py ru PARENT_DIR NEW_DIR
      DIR/ru_vecN.txt = output of `make resource-usage RU_SRCS=come_sgns_vecN.hip`.  Prints the
      parent / new table of VGPRs, SGPRs, scratch and occupancy and marks new or grown scratch and
      any change of occupancy.
"""
import re
import subprocess
import sys

MODE, A, B = sys.argv[1:4]
VECS = (1, 2, 4, 8)


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
            body.append(line)
    return out


def kernels(path):
    return sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M)))


def resources(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|Occupancy|ScratchSize)( \[[^]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(3))
    return out


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True)
    short = [re.sub(r"^void come::|\(come::O[12]Args\)$", "", s) for s in p.stdout.split("\n")]
    return dict(zip(names, short))


ok = True
for n in VECS:
    if MODE == "asm":
        pa, pb = "%s/vec%d.s" % (A, n), "%s/vec%d.s" % (B, n)
        ka, fa, fb = kernels(pa), functions(pa), functions(pb)
        same = [k for k in ka if fa[k] == fb.get(k)]
        stream = [k for k in ka if "k_sgns_o2_stream" in k]
        print("vec%d: %d kernels, symbol sets equal: %s; identical: %d of %d stream kernels, %d of "
              "%d others" % (n, len(ka), ka == kernels(pb), len(set(stream) & set(same)),
                             len(stream), len(set(same) - set(stream)), len(ka) - len(stream)))
        dm = demangle(ka)
        for k in ka:
            print("  %-46s %6d -> %6d lines%s" % (dm[k], len(fa[k]), len(fb.get(k, [])),
                                                  "  identical" if k in same else ""))
        ok &= ka == kernels(pb) and set(stream) <= set(same)
    else:
        ra, rb = resources("%s/ru_vec%d.txt" % (A, n)), resources("%s/ru_vec%d.txt" % (B, n))
        dm = demangle(sorted(ra))
        fmt = lambda r: "%4d %4d %4d %2d" % (r["VGPRs"], r["TotalSGPRs"], r["ScratchSize"],
                                            r["Occupancy"])
        for k in sorted(ra, key=dm.get):
            x, y = ra[k], rb[k]
            note = " scratch up" if y["ScratchSize"] > x["ScratchSize"] else ""
            note += " occupancy %+d" % (y["Occupancy"] - x["Occupancy"]) \
                if y["Occupancy"] != x["Occupancy"] else ""
            print("  %-46s %s   %s %s" % (dm[k], fmt(x), fmt(y), note))
print("stream kernels identical, symbol sets equal" if ok and MODE == "asm" else
      "" if ok else "FAIL")
sys.exit(0 if ok else 1)
