"""Kernel resource table of two builds of one .hip file, from the compiler's remarks.

    hipcc <the Makefile's flags> -Rpass-analysis=kernel-resource-usage -c -o /dev/null FILE.hip 2> parent.txt     (at the parent commit)
    hipcc ...                                                                          2> branch.txt     (at this one)
    python scripts/kernel_resources.py parent.txt branch.txt [only-kernels-matching]

Per kernel: TotalSGPRs, VGPRs, AGPRs, ScratchSize, Occupancy, SGPRs Spill, VGPRs Spill, LDS Size; the parent's line, then this commit's,
"=" where all eight agree.  No GPU is needed.  Device functions that are not inlined are listed like kernels (the remark has them)."""
import re
import subprocess
import sys

KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size"]


def parse(path):
    out, cur = {}, None
    names = []
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            names.append(cur)
            out[cur] = {}
            continue
        if cur is None:
            continue
        for k in KEYS:
            m = re.search(r":\s+" + re.escape(k) + r"(?: \[[^\]]*\])?: (\d+)", line)
            if m:
                out[cur][k] = int(m.group(1))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, dem):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*$", "", d).replace("bslv::", "")
        short[d] = out[n]
    return short


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    pat = sys.argv[3] if len(sys.argv) > 3 else ""
    print("%-44s" % "kernel (parent / branch)" + "".join("%13s" % k for k in KEYS) + " | same")
    differ = 0
    for name in sorted(set(a) | set(b)):
        if pat and not re.search(pat, name):
            continue
        ra, rb = a.get(name), b.get(name)
        fmt = lambda r: "".join("%13d" % r.get(k, -1) for k in KEYS)
        print("%-44s" % name + (fmt(ra) + " | parent" if ra else "  (not in this build) | parent"))
        if rb is None:
            print("%-44s" % "" + "  (not in this build) | branch GONE")
            differ += 1
        elif ra is None:
            print("%-44s" % "" + fmt(rb) + " | branch NEW")
        else:
            same = ra == rb
            differ += not same
            print("%-44s" % "" + fmt(rb) + " | branch " + ("=" if same else "DIFFERS"))
    print("existing kernels that differ: %d" % differ)


if __name__ == "__main__":
    main()
