#!/usr/bin/env python3
"""Show that an edit of the kernel sources is a no-op: compare the gfx950 instruction streams of two trees.

    tools/isa_diff.py A B          A, B: a source tree (directory) or a git revision (checked out with `git worktree`
                                   under a temporary directory)

For every file in SRCS of perceiverio_pytorch_amd/csrc/Makefile, on both sides: take that object's compile line from
`make -n -B`, run it with -S --cuda-device-only instead of -c, and split the assembly into functions.  File-scope
objects are masked by their size (so renaming one is no difference, resizing one is), compiler-made label numbers by
their order of appearance, comments dropped.  Prints per kernel "identical" or a unified diff, then its resource line
(registers, scratch, LDS, occupancy; both sides' where they differ), and a table per translation unit at the end.
Exit status 1 on any difference.  CPU only: hipcc cross-compiles.
"""
import concurrent.futures
import difflib
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join("perceiverio_pytorch_amd", "csrc")
RESOURCES = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def checkout(arg, tmp, side):
    if os.path.isdir(arg):
        return os.path.abspath(arg)
    tree = os.path.join(tmp, "tree_" + side)
    subprocess.check_call(["git", "worktree", "add", "--detach", tree, arg], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    return tree


def sources(tree):
    mk = open(os.path.join(tree, CSRC, "Makefile")).read()
    return re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()


def assemble(tree, src, out):
    """The object's own compile line (flags included), redirected to device assembly in `out`."""
    csrc = os.path.join(tree, CSRC)
    obj = src[:-len(".hip")] + ".o"
    plan = subprocess.check_output(["make", "-n", "-B", obj], cwd=csrc, text=True)
    line = next(l for l in plan.splitlines() if " -c " in l and src in l)
    words = shlex.split(line.split(" 2>")[0])
    drop = {"-c", "-o", obj, "-MMD", "-MP"}
    cmd = [w for w in words if w not in drop] + ["-S", "--cuda-device-only", "-o", out]
    subprocess.run(cmd, cwd=csrc, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def functions(asm):
    """{name: (masked instruction lines, resource lines)} of one assembly file."""
    sizes = dict(re.findall(r"^\s*\.(?:size|comm)\s+([^\s,]+),\s*(\d+)\b", asm, re.M))
    objects = {o: "<object of %s bytes>" % sizes.get(o, "?") for o in re.findall(r"^\s*\.type\s+([^\s,]+),@object", asm, re.M)}
    symbol = re.compile("|".join(sorted(map(re.escape, objects), key=len, reverse=True)) or r"(?!)")
    out, name, body, labels = {}, None, [], {}
    for raw in asm.splitlines():
        start = re.match(r"^([^\s;:]+):\s*; @\1\s*$", raw)
        if start:
            name, body, labels = start.group(1), [], {}
        elif name is None:
            pass
        elif raw.startswith(".Lfunc_end"):
            out[name] = (body, [])
        elif name in out:  # behind the code: the "; Kernel info:" comments
            info = re.match(r"^; (%s): (\S+)" % "|".join(RESOURCES), raw)
            if info:
                out[name][1].append("%s %s" % info.groups())
        else:
            text = symbol.sub(lambda m: objects[m.group(0)], raw.split(";")[0].rstrip())
            text = re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), text)
            if text.strip():
                body.append(text)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        trees = [checkout(a, tmp, s) for a, s in zip(sys.argv[1:], "ab")]
        try:
            srcs, table = sources(trees[0]), []
            if sources(trees[1]) != srcs:
                print("SRCS differ: %s / %s" % (srcs, sources(trees[1])))
                status = 1
            with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
                jobs = {(s, i): pool.submit(assemble, t, s, os.path.join(tmp, "%s.%d.s" % (s, i)))
                        for s in srcs for i, t in enumerate(trees)}
                for s in srcs:
                    a, b = (functions(jobs[s, i].result()) for i in (0, 1))
                    same = 0
                    for k in sorted(set(a) | set(b)):
                        if k not in a or k not in b:
                            print("only in %s: %s" % (sys.argv[1 if k in a else 2], k))
                            continue
                        if a[k][0] == b[k][0]:
                            print("identical  %s" % k)
                        else:
                            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(
                                a[k][0], b[k][0], "%s %s" % (sys.argv[1], k), "%s %s" % (sys.argv[2], k), lineterm="", n=2))
                        for side in {0: (a,), 1: (a, b)}[a[k][1] != b[k][1]]:
                            print("    " + ", ".join(side[k][1]))
                        same += a[k] == b[k]
                    table.append("%-22s %3d kernels, %3d identical" % (s, len(set(a) | set(b)), same))
                    status |= same != len(set(a) | set(b))
        finally:
            for t, arg in zip(trees, sys.argv[1:]):
                if not os.path.isdir(arg):
                    subprocess.call(["git", "worktree", "remove", "--force", t], stdout=subprocess.DEVNULL)
    print("\n".join(table))
    print("DIFFERENT" if status else "identical: every kernel of every translation unit, instructions and resources")
    sys.exit(status)


if __name__ == "__main__":
    main()
