#!/usr/bin/env python3
"""The a-trous kernels' resources and instruction counts in two builds' device assembly:
asm_table.py PARENT_BUILD NEW_BUILD (the directories `make BUILD=... asm` filled).  Per kernel and
build: LDS bytes, private segment bytes, VGPRs (the descriptor's next-free VGPR, and the waves per
SIMD that allocation leaves: 512 registers in granules of 8), blocks per CU the LDS admits (160 KB,
at most the 8 blocks of 4 waves that 32 wave slots hold), and the counts of global_load*, ds_* and
all instructions.  Prints a markdown table."""
import pathlib
import re
import sys


def kernels(build):
    out = {}
    for path in sorted(pathlib.Path(build).glob("*.s")):
        name, body = None, []
        for line in path.read_text().splitlines():
            line = line.split(";")[0].rstrip()
            if name is None and re.match(r"_ZN12_GLOBAL__N_1\d+k_atrous\w*:$", line):
                name, body = line[:-1], []
            elif name is not None and line.startswith(".Lfunc_end"):
                out[name], name = body, None
            elif name is not None and line.strip():
                body.append(line.strip())
    return out


def short(sym):
    m = re.match(r"_ZN12_GLOBAL__N_1\d+(k_atrous(?:_var)?(?:_lds)?)(?:ILi(\d)EE)?", sym)
    return m.group(1) + (f"<{m.group(2)}>" if m.group(2) else "")


def figures(body):
    def field(key):
        return next(int(l.split()[1]) for l in body if l.startswith(key + " "))

    ins = [l.split()[0] for l in body if not l.startswith(".") and not l.endswith(":")]
    vgpr, lds = field(".amdhsa_next_free_vgpr"), field(".amdhsa_group_segment_fixed_size")
    alloc = -(-vgpr // 8) * 8
    return [lds, field(".amdhsa_private_segment_fixed_size"), vgpr, min(8, 512 // alloc),
            min(8, 160 * 1024 // lds) if lds else 8, sum(i.startswith("global_load") for i in ins),
            sum(i.startswith("ds_") for i in ins), len(ins)]


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
print("| kernel | build | LDS B | private B | VGPRs | waves/SIMD | blocks/CU | global_load | ds_ | instructions |")
print("|---|---|---|---|---|---|---|---|---|---|")
for sym in sorted(old, key=short):
    for tag, b in (("parent", old), ("new", new)):
        print(f"| `{short(sym)}` | {tag} | " + " | ".join(str(v) for v in figures(b[sym])) + " |")
