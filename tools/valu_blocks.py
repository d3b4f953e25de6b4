#!/usr/bin/env python3
"""Static VALU count of a kernel from its gfx950 assembly, per basic block.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -Iinclude -S plonky2.5_amd/csrc/kernels_ntt.hip -o ntt.s
    tools/valu_blocks.py ntt.s k_ntt_tile

Prints, for every function whose (mangled) name contains the pattern, its basic blocks with their `v_` instruction
counts (blocks of at least 8), the LDS / global accesses in them and where the block's last branch goes, so that loop bodies can be multiplied by
their trip counts by hand (profiles/r11_ntt_addressing.txt was made this way)."""
import re
import sys


def main():
    path, pat = sys.argv[1], sys.argv[2]
    fn, blocks, cur = None, [], None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            name = m.group(1)
            if not name.startswith(".L"):
                fn = name if pat in name else None
                if fn:
                    print(f"\n== {fn}")
            if fn:
                cur = {"label": name, "valu": 0, "mul": 0, "ds": 0, "glob": 0, "br": ""}
                blocks.append(cur)
            continue
        if not fn or cur is None or not s or s.startswith((";", ".")):
            if fn and s.startswith(".end_amdhsa_kernel") or (fn and s.startswith(".Lfunc_end")):
                total = sum(b["valu"] for b in blocks)
                for b in blocks:
                    if b["valu"] >= 8:   # the rest is branch glue
                        print(f"  {b['label'][:14]:<14} valu {b['valu']:5d}  (mul_lo/hi_u32+mad_u64 {b['mul']:4d})  ds {b['ds']:3d}  "
                              f"global {b['glob']:3d}  {b['br']}")
                print(f"  static total {total}")
                fn, blocks, cur = None, [], None
            continue
        op = s.split()[0]
        if op.startswith("v_"):
            cur["valu"] += 1
            if op.startswith(("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32")):
                cur["mul"] += 1
        elif op.startswith("ds_"):
            cur["ds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_")):
            cur["glob"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            cur["br"] += f"{op}->{s.split()[-1]} "


if __name__ == "__main__":
    main()
