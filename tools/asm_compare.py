#!/usr/bin/env python3
"""Compare two device assembly files function by function.

    asm_compare.py A.s B.s [--map RENAMES]

A.s and B.s are what `hipcc -S --cuda-device-only` writes for one translation
unit before and after a change (the library's flags: HIPFLAGS of
dwarf-p-cloudsc_amd/Makefile).  Each file is cut into functions; of a function
only its instruction lines and the labels between them are kept: comments and
assembler directives are dropped, and so is the per-function number of the
local labels (.LBB<function>_<block>), which changes whenever a function is
added in front.  The two streams of a function are then compared line by line.

Output, one line per function of A in A's order,

      N instr     M differing  <demangled name>

where N counts the kept lines and M those a line diff does not match (0: the
same instruction stream, register for register), then the functions that only one side has, and
first of all the kernel counts of both sides.  The exit status is 1 if any
function differs or is missing on either side.

--map RENAMES: a text file of `OLD => NEW` lines that maps names of A to names
of B, for a change that renames functions.  OLD and NEW are names as printed
here; with `re:` in front, OLD is a regular expression that has to match a whole
name, and NEW may refer to its groups (\\1 ...).  The first rule that matches a
name applies.  Blank lines and lines that start with # are skipped.

The tool reads text only; it needs no GPU.
"""
import argparse
import difflib
import re
import shutil
import subprocess
import sys

FUNC_TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+_(\d+)")


def parse(text):
    """-> ({mangled name: [stream lines]} in file order, set of kernel names)"""
    funcs, kernels = {}, set()
    pending, cur = None, None
    for raw in text.splitlines():
        m = KERNEL.match(raw)
        if m:
            kernels.add(m.group(1))
        m = FUNC_TYPE.match(raw)
        if m:
            pending = m.group(1)
            continue
        if cur is None:
            if pending is not None and raw.startswith(pending + ":"):
                cur = funcs.setdefault(pending, [])
                pending = None
            continue
        if FUNC_END.match(raw):
            cur = None
            continue
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        line = LOCAL_LABEL.sub(r".L\1_\2", line)
        if line.startswith(".") and not line.endswith(":"):
            continue                                   # a directive (a local label ends in ':')
        cur.append(" ".join(line.split()))
    return funcs, kernels


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True).stdout.splitlines()
    if len(out) != len(names):
        return {n: n for n in names}
    return {n: short_name(d) for n, d in zip(names, out)}


def short_name(demangled):
    """A template instance without its parameter list (the template arguments tell instances apart)."""
    if "<" not in demangled:
        return demangled
    depth = 0
    for i, ch in enumerate(demangled.replace("(anonymous namespace)", "[anonymous namespace]")):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return demangled[:i]
    return demangled


def load_map(path):
    rules = []
    if not path:
        return rules
    for raw in open(path):
        line = raw.strip()
        if not line or line.startswith("#"):
            continue
        if "=>" not in line:
            raise SystemExit("%s: not an `OLD => NEW` line: %s" % (path, line))
        old, new = (x.strip() for x in line.split("=>", 1))
        rules.append((re.compile(old[3:].strip()), new) if old.startswith("re:") else (old, new))
    return rules


def rename(name, rules):
    for old, new in rules:
        if isinstance(old, str):
            if old == name:
                return new
        elif old.fullmatch(name):
            return old.sub(new, name)
    return name


def differing(a, b):
    if a == b:
        return 0
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")


def compare(text_a, text_b, rules=()):
    """-> (report lines, number of functions that differ or are missing on a side)"""
    fa, ka = parse(text_a)
    fb, kb = parse(text_b)
    na, nb = demangle(list(fa)), demangle(list(fb))
    by_name_b = {nb[m]: m for m in fb}
    lines = ["kernels: A %d, B %d" % (len(ka), len(kb))]
    bad, seen = 0, set()
    only_a = []
    for m, stream in fa.items():
        name = rename(na[m], rules)
        if name == na[m] and m in fb:
            mb = m
        else:
            mb = by_name_b.get(name)
        if mb is None or mb in seen:
            only_a.append(na[m] if name == na[m] else "%s (=> %s)" % (na[m], name))
            continue
        seen.add(mb)
        d = differing(stream, fb[mb])
        bad += d != 0
        label = name if name == na[m] else "%s  (was %s)" % (name, na[m])
        lines.append("%6d instr %5d differing  %s" % (len(stream), d, label))
    only_b = [nb[m] for m in fb if m not in seen]
    lines += ["only in A: " + n for n in only_a] + ["only in B: " + n for n in only_b]
    return lines, bad + len(only_a) + len(only_b)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--map", help="file of `OLD => NEW` name rules (see the module text)")
    args = ap.parse_args(argv)
    lines, bad = compare(open(args.a).read(), open(args.b).read(), load_map(args.map))
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
