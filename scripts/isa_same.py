#!/usr/bin/env python3
"""Are two device-assembly builds of trace.hip the same code, kernel by kernel?

A kernel is the text from its label to its .Lfunc_end (the .amdhsa_kernel block lies in between), without
comments, with the function number taken out of basic-block labels (.LBB12_3 -> .LBB_3) and the kernel's own name
replaced.  Kernels are matched by identifier and template arguments (the argument types may differ);
--rename OLD=NEW matches a renamed one, e.g. --rename k_emit_power=k_emit<1> (template arguments as the mangled
name spells them: <2,0,1>).  Exit status 1 when a kernel of OLD has no identical counterpart in NEW.
usage: hipcc ... --cuda-device-only -S csrc/device/trace.hip -o new.s   (and old.s from the other tree)
       python scripts/isa_same.py old.s new.s [--rename OLD=NEW ...] [--show 12]
"""
from __future__ import annotations

import argparse
import difflib
import re


def kernel_key(sym):
    """identifier<template arguments> of a mangled kernel name in the anonymous namespace"""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", sym)
    if not m:  # (a library's kernel: the whole symbol)
        return sym
    k = m.end() + int(m.group(1))
    ident, args = sym[m.end():k], []
    if sym[k:k + 1] == "I":
        k += 1
        while sym[k] == "L":  # integral literals only: Li2E, Lb0E, Lj64E
            e = sym.index("E", k)
            args.append(sym[k + 2:e])
            k = e + 1
    return ident + ("<" + ",".join(args) + ">" if args else "")


def kernels(path):
    lines = open(path).read().splitlines()
    names = {ln.split()[1] for ln in lines if ln.startswith("\t.amdhsa_kernel ")}
    out, name, start = {}, None, 0
    for k, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None and m.group(1) in names:
            name, start = m.group(1), k + 1
        elif name is not None and ln.startswith(".Lfunc_end"):
            body = []
            for x in lines[start:k]:
                x = re.sub(r"\.LBB\d+_", ".LBB_", x.split(";")[0])
                x = x.replace(name, "KERNEL").replace(name[2:], "KERNEL").strip()  # ([2:]: inside a nested symbol)
                if x:
                    body.append(x)
            key = kernel_key(name)
            assert key not in out, key
            out[key] = body
            name = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--show", type=int, default=12, help="differing lines printed per kernel")
    a = ap.parse_args()
    ren = dict(r.split("=", 1) for r in a.rename)
    old, new = kernels(a.old), kernels(a.new)
    differ = 0
    for key, body in old.items():
        to = ren.get(key, key)
        if to not in new:
            differ += 1
            print(f"MISSING {key} -> {to}")
        elif new[to] != body:
            differ += 1
            d = [x for x in difflib.unified_diff(body, new[to], lineterm="", n=0)
                 if x[:1] in "+-" and x[:3] not in ("+++", "---")]
            print(f"DIFFERS {key} -> {to}: {len(body)} -> {len(new[to])} lines, {len(d)} diff lines")
            for x in d[:a.show]:
                print("    " + x)
    print(f"{len(old)} kernels compared, {differ} differing ({len(new)} kernels in the new file)")
    raise SystemExit(1 if differ else 0)


if __name__ == "__main__":
    main()
