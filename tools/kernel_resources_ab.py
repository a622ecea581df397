"""Kernel resources and instruction text of rts_kernels.hip, parent commit against this one (profiles/r14/kernel_resources.txt).

    python tools/kernel_resources_ab.py PARENT_LOG PARENT_S NEW_LOG NEW_S [PARENT_NAME=NEW_NAME ...]

PARENT_NAME=NEW_NAME: a kernel that only changed its mangled name (it gained a template parameter, say) is compared under the parent's.
LOG = the output of `make -C raytracedshadows_amd/csrc asm` in that tree, S = the build/rts_kernels.s it writes.  A kernel counts as
the same when every figure of its resource remark and the hash of its instructions and labels agree."""
import hashlib
import os
import re
import sys
def remarks(path):
    out = {}; cur = None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m: cur = m.group(1); out[cur] = {}; continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur: out[cur][m.group(1).strip()] = m.group(2)
    return out
def bodies(path):
    out = {}; cur = None; buf = []
    for line in open(path):
        m = re.match(r"^(_ZN\d+rts\w+):\s", line)
        if m and not line.startswith("."):
            cur = m.group(1); buf = []; continue
        if cur is not None:
            if line.startswith("\t.section") or line.startswith(".Lfunc_end"):
                out.setdefault(cur, "".join(buf)); cur = None; continue
            s = line.split(";")[0].rstrip()
            if s.strip() and not s.strip().startswith("."): buf.append(re.sub(r"\.LBB\d+_", ".LBB_", s) + "\n")
            elif s.strip().startswith(".LBB"): buf.append(re.sub(r"\.LBB\d+_", ".LBB_", s) + "\n")
    return out
pr, nr = remarks(sys.argv[1]), remarks(sys.argv[3])
pb = bodies(sys.argv[2])
nb = bodies(sys.argv[4])
for old, new in (a.split("=") for a in sys.argv[5:]):
    nr[old] = nr.pop(new); nb[old] = nb.pop(new)
    print("# renamed:", old, "is this commit's", new)
keys = ["VGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size"]
def row(r): return " ".join(f"{k.split()[0]}={r.get(k, r.get(k+' [bytes/lane]', '?'))}" for k in keys)
unit = os.path.splitext(os.path.basename(sys.argv[4]))[0] + ".hip"
print(f"# hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (`make asm` and its flags) of {unit}, parent commit and this commit.")
print("# text = first 12 hex digits of the sha1 over the kernel's instructions and labels in the generated assembly.")
print("## kernels this commit adds")
for k in sorted(nr):
    if k not in pr: print(k, nr[k])
print("## kernels of the parent commit: parent | this commit")
same = diff = 0
for k in sorted(pr):
    hp = hashlib.sha1(pb.get(k, "").encode()).hexdigest()[:12]; hn = hashlib.sha1(nb.get(k, "?").encode()).hexdigest()[:12]
    ok = pr[k] == nr.get(k) and hp == hn and len(pb.get(k, "")) > 0
    same += ok; diff += not ok
    print(("same " if ok else "DIFF "), k, pr[k], "|", nr.get(k), "| text", hp, hn, "| instructions", pb.get(k, "").count("\n"))
print(f"## {same} kernels identical in resources and instruction text, {diff} different")
