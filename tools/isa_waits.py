#!/usr/bin/env python3
"""The vector-memory waits of one kernel, in program order, from the ISA that `hipcc -save-temps` keeps.

Lists every global load, store and atomic, every `s_waitcnt` with a vmcnt, every `s_barrier` and every loop header of the
kernel whose symbol contains KERNEL (the first match), with its line in the .s file.  On gfx9 vmcnt counts stores as well
as loads: a vmcnt(0) placed after a run of stores waits for all of them.

usage: isa_waits.py <file.s> <kernel symbol substring>
  the .s of the library: cd phagefilter_amd/csrc && hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall \\
      -Wno-unused-function -ffp-contract=off --cuda-device-only -save-temps -c pfq_kernels.hip -o /tmp/k.o"""
import re
import sys

VMEM = re.compile(r"^\s*(global_|buffer_|flat_)\w+")
WAIT = re.compile(r"^\s*s_waitcnt\b.*vmcnt")
LABEL = re.compile(r"^(\.LBB\w+):.*")


def main() -> None:
    path, name = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_\w*" + re.escape(name) + r"\w*:", l))
    sym = lines[start].split(":")[0]
    print(f"; {sym}  ({path})")
    header = None
    for i in range(start + 1, len(lines)):
        l = lines[i]
        if l.strip().startswith("s_endpgm"):
            break
        m = LABEL.match(l)
        if m:
            header = m.group(1)
            continue
        if "Loop Header" in l and header:
            print(f"{i + 1:7d}  {header}:  {l.split(';', 1)[1].strip()}")
            continue
        if VMEM.match(l) or WAIT.match(l) or l.strip().startswith("s_barrier"):
            print(f"{i + 1:7d}      {l.strip()}")


if __name__ == "__main__":
    main()
