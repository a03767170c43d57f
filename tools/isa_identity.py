#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two gfx950 assembly files of the same source (`hipcc -O3 -std=c++17
--offload-arch=gfx950 --cuda-device-only -S`): instruction lines with comments and directives stripped, and the resource
figures the compiler prints behind each kernel.  Prints one markdown table row per kernel; exit status 1 when a kernel
exists on one side only, 2 when a kernel that had no scratch has some.

    python tools/isa_identity.py [--rename 'parent kernel=head kernel' ...] parent/grad.s head/grad.s [more pairs ...]

A kernel that was merged into or renamed to another is paired by hand, with the names the table prints:
`--rename 'bn_pack_ste_kernel<4>=pack_ste_kernel<4, true>'` compares the parent's first with the head's second.
"""
import difflib
import re
import sys

FIGURES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize")


def kernels(text):
    """{symbol: (instruction lines, {figure: int})} of every function of an assembly file, in file order."""
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = [body, {}]
            name = None
            continue
        code = line.split(";")[0].strip()
        if code and not code.startswith("."):
            body.append(code)
    # the figures follow each function as comments, in the same order as the functions
    blocks = re.findall(r"; (?:Kernel|Function) info:\n((?:; .*\n)+)", text)
    for (name, entry), block in zip(out.items(), blocks):
        for key in FIGURES:
            m = re.search(rf"; {key}: (\d+)", block)
            entry[1][key] = int(m.group(1)) if m else -1
    return out


def short_name(sym):
    """`kernel<template arguments>` of a mangled kernel symbol (the arguments these sources use: int, bool, float types
    and named structs)."""
    pos, name = 3, ""   # behind _ZN: length-prefixed identifiers, the last one is the kernel
    while (n := re.match(r"\d+", sym[pos:])):
        pos += len(n.group())
        name = sym[pos:pos + int(n.group())]
        pos += int(n.group())
    if sym[pos:pos + 1] != "I":
        return name
    pos += 1
    words = {"DF16b": "bf16", "DF16_": "f16", "f": "float", "Lb0E": "false", "Lb1E": "true"}
    args = []
    while pos < len(sym) and sym[pos] != "E":
        if (t := re.match(r"L[ib]\d+E|DF16b|DF16_|f", sym[pos:])):
            args.append(words.get(t.group(), t.group()[2:-1]))
            pos += len(t.group())
        elif (t := re.match(r"(NS_)?(\d+)", sym[pos:])):       # a struct, with or without the enclosing namespace
            pos += len(t.group())
            args.append(sym[pos:pos + int(t.group(2))])
            pos += int(t.group(2)) + (1 if t.group(1) else 0)
        else:
            return name + "<" + sym[pos:] + ">"
    return f"{name}<{', '.join(args)}>"


def main(argv):
    renames = {}
    while argv and argv[0] == "--rename":
        old, new = argv[1].split("=", 1)
        renames[old.strip()] = new.strip()
        argv = argv[2:]
    print("| file | kernel | instructions parent / head | VGPR | AGPR | SGPR | scratch | LDS | stream |")
    print("|---|---|---|---|---|---|---|---|---|")
    worst = 0
    for a, b in zip(argv[0::2], argv[1::2]):
        ka, kb = kernels(open(a).read()), kernels(open(b).read())
        # symbols move with namespaces and argument types: pair the kernels by name and template arguments
        by_a = {renames.get(short_name(n), short_name(n)): v for n, v in ka.items()}
        by_b = {short_name(n): v for n, v in kb.items()}
        for name in sorted(set(by_a) | set(by_b)):
            if name not in by_a or name not in by_b:
                print(f"| {a.split('/')[-1]} | `{name}` | {'only parent' if name in by_a else 'only head'} | | | | | | |")
                worst = max(worst, 1)
                continue
            (ia, fa), (ib, fb) = by_a[name], by_b[name]
            # symbols, and the function index of a basic-block label (.LBB<function>_<block>), move with the file's text
            strip = lambda lines: [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", s)) for s in lines]
            ia, ib = strip(ia), strip(ib)
            diff = sum(1 for d in difflib.unified_diff(ia, ib, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
            cols = " | ".join(f"{fa[k]} / {fb[k]}" if fa[k] != fb[k] else f"{fa[k]}" for k in FIGURES)
            if fa["ScratchSize"] == 0 and fb["ScratchSize"] != 0:
                worst = max(worst, 2)
            print(f"| {a.split('/')[-1]} | `{name}` | {len(ia)} / {len(ib)} | {cols} | {'identical' if diff == 0 else f'{diff} lines differ'} |")
    return worst


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
