"""Compare two directories of device assembly (parent, change; one .s per .hip, from hipcc --cuda-device-only -S with
the Makefile's HIPFLAGS) kernel symbol by kernel symbol.  A kernel's text is what stands between its label and its
.Lfunc_end label, without comments, blank lines, .file / .loc / .ident lines and the numbers in local labels; nothing
else about the instructions is looked at.  Prints the demangled name of every kernel whose text differs (or that only
one side has) with the line counts of both sides; exits 1 if one of them matches none of the allowed regexes.
Usage: python tools/diag/kernel_isa_diff.py parent_asm_dir change_asm_dir [allowed-name-regex ...]"""
import os
import re
import subprocess
import sys

LOCAL = re.compile(r"(\.L[A-Za-z_]*)[0-9][0-9_]*")
SKIP = re.compile(r"\s*\.(file|loc|ident)\b")


def kernels(path):
    """{kernel symbol: [normalised lines]} of one assembly file"""
    lines = open(path).read().split("\n")
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    out, cur = {}, None
    for l in lines:
        m = re.match(r"([A-Za-z_$][\w$.]*):", l)
        if m and m.group(1) in names:
            cur = out[m.group(1)] = []
            continue
        if cur is None:
            continue
        if l.lstrip().startswith(".Lfunc_end"):
            cur = None
            continue
        l = l.split(";")[0].rstrip()
        if l.strip() and not SKIP.match(l):
            cur.append(LOCAL.sub(r"\1", l))
    return out


def load(d):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".s"):
            for k, v in kernels(os.path.join(d, f)).items():
                out[(f, k)] = v
    return out


parent, change = load(sys.argv[1]), load(sys.argv[2])
allowed = [re.compile(a) for a in sys.argv[3:]]
keys = sorted(set(parent) | set(change))
differ = [k for k in keys if parent.get(k) != change.get(k)]
dem = subprocess.run(["c++filt"], input="\n".join(k[1] for k in differ), capture_output=True, text=True).stdout.split("\n")
bad = 0
for (f, _), d in zip(differ, dem):
    d = d.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
    ok = any(a.search(d) for a in allowed)
    bad += not ok
    n = [len(s[(f, _)]) if (f, _) in s else "absent" for s in (parent, change)]
    print("%s%s: %s  parent %s lines, change %s lines" % ("" if ok else "NOT ALLOWED ", f, d, n[0], n[1]))
print("# %d kernels in the parent, %d in the change; %d differ, %d of them outside the allow-list" % (
    len(parent), len(change), len(differ), bad))
sys.exit(1 if bad else 0)
