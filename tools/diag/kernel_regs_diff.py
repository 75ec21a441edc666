"""Compare two tools/diag/kernel_regs.py summaries (parent, change) kernel by kernel and check the resource
condition: no kernel loses occupancy, gains scratch or gains a VGPR spill.  A kernel of the change that the parent
does not have is matched with the parent instance named by its template arguments without the last one (a
template that gained a trailing argument, e.g. conv_kernel's FAST1).  Prints every kernel whose occupancy, AGPRs,
VGPR spills or scratch differ or whose VGPRs rise by more than 3, then the counts; exits 1 if the condition fails.
Usage: python tools/diag/kernel_regs_diff.py parent_regs.txt change_regs.txt"""
import re
import sys

LINE = re.compile(r"(.*?)\s+V\s+(\S+) A\s+(\S+) occ (\S+) sgprspill (\S+) vgprspill (\S+) scratch (\S+) lds (\S+)")
FMT = "V %3d A %3d occ %d sgprspill %2d vgprspill %d scratch %2d"


def load(path):
    rows = {}
    for line in open(path):
        m = LINE.match(line)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    return rows


parent, change = load(sys.argv[1]), load(sys.argv[2])
differ = worse = unmatched = 0
for k in sorted(change):
    pk = k if k in parent else re.sub(r", [^,<>]+>$", ">", k)
    if pk not in parent:
        unmatched += 1
        print("no parent instance:", k, FMT % change[k][:6])
        continue
    p, c = parent[pk], change[k]
    if p == c:
        continue
    differ += 1
    bad = c[2] < p[2] or c[5] > p[5] or c[4] > p[4]
    worse += bad
    if bad or c[1] != p[1] or c[2] != p[2] or c[4] != p[4] or c[5] != p[5] or c[0] > p[0] + 3:
        print("%s%s\n  < %s\n  > %s" % ("WORSE " if bad else "", k, FMT % p[:6], FMT % c[:6]))
print("# %d kernels in the parent, %d in the change; %d differ in some field, %d unmatched; %d lose occupancy or gain "
      "scratch / VGPR spills" % (len(parent), len(change), differ, unmatched, worse))
sys.exit(1 if worse else 0)
