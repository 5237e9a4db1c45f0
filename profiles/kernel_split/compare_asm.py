#!/usr/bin/env python3
"""Device code of two builds, function by function: compare_asm.py PARENT_BUILD NEW_BUILD, the two
directories `make BUILD=... asm` filled with one .s per .hip.  For every function symbol, whichever
file holds it: the lines from its label to its .Lfunc_end (the instructions and, for a kernel, its
.amdhsa_ descriptor block: VGPR / AGPR / SGPR counts, LDS and private segment sizes), `;` comments
stripped and the function's index in .L local labels (.LBB40_17) normalised.  Exits 1 on any
difference and on any function in one build and not the other."""
import collections
import pathlib
import re
import sys


def functions(build):
    """{symbol: (file, cleaned lines, is a kernel)}"""
    out = {}
    for path in sorted(pathlib.Path(build).glob("*.s")):
        typed, name, body = set(), None, []
        for line in path.read_text().splitlines():
            line = line.split(";")[0].rstrip()
            if m := re.match(r"\s*\.type\s+([^\s,]+),@function", line):
                typed.add(m.group(1))
            elif name is None and line.endswith(":") and line[:-1] in typed:
                name, body = line[:-1], []
            elif name is not None and line.startswith(".Lfunc_end"):
                key = name if name not in out else f"{name}@{path.name}"  # two files' same-named locals
                out[key] = (path.name, body, any(".amdhsa_kernel" in b for b in body))
                name = None
            elif name is not None and line.strip():
                body.append(re.sub(r"(\.L[A-Za-z_]*?)\d+_", r"\1N_", line))
    return out


old, new = functions(sys.argv[1]), functions(sys.argv[2])
bad = 0
for sym in sorted(old.keys() | new.keys()):
    if sym not in old or sym not in new:
        print(f"ONLY IN {'parent' if sym in old else 'new'}: {sym} ({(old.get(sym) or new.get(sym))[0]})")
    elif old[sym][1] != new[sym][1]:
        n = sum(a != b for a, b in zip(old[sym][1], new[sym][1])) + abs(len(old[sym][1]) - len(new[sym][1]))
        print(f"DIFFERS: {sym} ({old[sym][0]} -> {new[sym][0]}): {n} lines")
    else:
        continue
    bad += 1
moves = collections.Counter((old[s][0], new[s][0], old[s][2]) for s in old.keys() & new.keys())
for (a, b, kern), n in sorted(moves.items()):
    print(f"{n:3d} {'kernels' if kern else 'other functions'}: {a} -> {b}")
print(f"parent: {sum(v[2] for v in old.values())} kernels, {len(old)} functions; "
      f"new: {sum(v[2] for v in new.values())} kernels, {len(new)} functions; {bad} differences")
sys.exit(1 if bad else 0)
