"""Compare the gfx950 assembly of two trees of this repository, kernel by kernel.

    python tools/isa_diff.py OLD_TREE NEW_TREE [--probe tools/FILE.hip] [-j N]

Every unit of physicsvae_amd/build.py's UNITS (of each tree's own build.py) is compiled with that tree's
FLAGS + ["-S", "--cuda-device-only"]; with --probe, the one stand-alone program instead (the path is taken relative to each
tree).  For every kernel symbol the instruction lines between its label and .Lfunc_end are compared -- comment lines,
assembler directives and the __hip_cuid_* symbol are left out (all that differs between two compiles of one source) -- and
the kernel is reported as

    identical   the same instruction lines in the same order
    reordered   the same multiset of mnemonics; the number of positions whose line differs is printed
    different   anything else (also: a kernel only one tree has)

with .vgpr_count / .sgpr_count / LDS bytes / private-segment bytes of both sides from the code object metadata.
Exit status 1 if any kernel is `different`.  A parent tree: `git archive HEAD~ | tar -x -C <tmpdir>` or `git worktree`."""
import argparse
import collections
import concurrent.futures
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

META = (("vgpr_count", "vgpr"), ("sgpr_count", "sgpr"), ("group_segment_fixed_size", "lds"),
        ("private_segment_fixed_size", "private"))


def load_build(tree):
    path = os.path.join(tree, "physicsvae_amd", "build.py")
    spec = importlib.util.spec_from_file_location("pvae_build_%x" % (hash(path) & 0xffffffff), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_asm(cc, flags, src, out):
    res = subprocess.run([cc] + flags + ["-S", "--cuda-device-only", src, "-o", out], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s%s" % (src, res.stdout, res.stderr))
    with open(out) as f:
        return f.read().split("\n")


def metadata(asm):
    """{kernel symbol: {key: value}} of the amdhsa.kernels list (the keys of a kernel's own mapping, not of its .args)."""
    out, cur = {}, None
    for l in asm:
        m = re.match(r"^  - \.(\w+):\s*(.*)$", l)
        if m:
            cur = {m.group(1): m.group(2)}
            continue
        m = re.match(r"^    \.(\w+):\s*(.*)$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                out[m.group(2).strip("'\"")] = cur
        elif not l.startswith("    "):
            cur = None
    return out


def kernels(asm):
    """{kernel symbol: [instruction line, ...]} -- whitespace-normalised, trailing comments dropped."""
    meta = metadata(asm)
    label = {}
    for i, l in enumerate(asm):
        m = re.match(r"^([^\s:]+):", l)
        if m and m.group(1) in meta:
            label[m.group(1)] = i
    out = {}
    for name, start in label.items():
        ins = []
        for l in asm[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            s = l.split(";", 1)[0].strip()
            if not l.startswith("\t") or not s or s.startswith(".") or "__hip_cuid_" in s:
                continue
            ins.append(" ".join(s.split()))
        out[name] = (ins, meta[name])
    return out


def classify(old, new):
    if old == new:
        return "identical", 0
    ops = lambda ins: collections.Counter(i.split()[0] for i in ins)
    if len(old) == len(new) and ops(old) == ops(new):
        return "reordered", sum(a != b for a, b in zip(old, new))
    return "different", 0


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool and os.path.exists("/opt/rocm/llvm/bin/llvm-cxxfilt"):
        tool = "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool] + list(names), capture_output=True, text=True)
    lines = res.stdout.strip().split("\n")
    return dict(zip(names, lines)) if res.returncode == 0 and len(lines) == len(names) else {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--probe", help="compare this stand-alone program (path relative to each tree) instead of build.UNITS")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    trees = [os.path.abspath(a.old), os.path.abspath(a.new)]
    builds = [load_build(t) for t in trees]
    cc = builds[1]._hipcc()
    tmp = tempfile.mkdtemp(prefix="isa_diff_")
    try:
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(max(1, min(16, a.j))) as pool:
            for side, (tree, b) in enumerate(zip(trees, builds)):
                units = [a.probe] if a.probe else b.UNITS
                for u in units:
                    src = os.path.join(tree, u) if a.probe else os.path.join(b.CSRC, u)
                    out = os.path.join(tmp, "%d_%s.s" % (side, os.path.basename(u)))
                    jobs[(side, u)] = pool.submit(compile_asm, cc, b.FLAGS, src, out)
        asm = {k: kernels(f.result()) for k, f in jobs.items()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    units = [a.probe] if a.probe else list(dict.fromkeys(builds[0].UNITS + builds[1].UNITS))
    total = collections.Counter()
    for u in units:
        old, new = asm.get((0, u), {}), asm.get((1, u), {})
        names = sorted(set(old) | set(new))
        pretty = demangle(names)
        print("== %s: %d kernels" % (u, len(names)))
        for n in names:
            if n not in old or n not in new:
                kind, note = "different", "only in the %s tree" % ("new" if n in new else "old")
                regs = ""
            else:
                (oi, om), (ni, nm) = old[n], new[n]
                kind, moved = classify(oi, ni)
                note = "%d instructions" % len(ni)
                if kind == "reordered":
                    note += ", %d positions differ" % moved
                elif kind == "different":
                    note = "%d -> %d instructions" % (len(oi), len(ni))
                regs = "  ".join("%s %s/%s" % (short, om.get(key, "?"), nm.get(key, "?")) for key, short in META)
            total[kind] += 1
            print("%-10s %s\n           %s  [old/new: %s]" % (kind, pretty[n], note, regs))
    print("== total: " + ", ".join("%d %s" % (total[k], k) for k in ("identical", "reordered", "different")))
    return 1 if total["different"] else 0


if __name__ == "__main__":
    sys.exit(main())
