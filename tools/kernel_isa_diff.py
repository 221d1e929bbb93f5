#!/usr/bin/env python3
"""Compare the instruction streams of kernels in two device-assembly files (hipcc -O3 --offload-arch=gfx950 -S
--cuda-device-only), with symbol names taken out: a change that must leave a kernel alone shows as identical here.

  python tools/kernel_isa_diff.py OLD.s NEW.s KERNEL_FRAGMENT [KERNEL_FRAGMENT ...]

A fragment has to name exactly one kernel in each file (a part of its mangled name, e.g. backend_kernelILi109ELb0ELb0E).
Exit status 0 when every listed kernel is identical."""
import re
import sys


def bodies(path):
    text = open(path).read().splitlines()
    out, name, body = {}, None, []
    for line in text:
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end") or re.match(r"^\s*\.size\s", line):
                out[name] = body
                name = None
                continue
            body.append(line)
    return out


def normalise(lines):
    res = []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()             # comments carry register counts and such
        if not line.strip():
            continue
        line = re.sub(r"_Z\w+", "SYM", line)              # mangled names: kernels, LDS globals, constants
        line = re.sub(r"\.L\w+", ".L", line)               # local labels are numbered per file
        res.append(line)
    return res


def main():
    if len(sys.argv) < 4:
        print(__doc__)
        return 2
    old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
    bad = 0
    for frag in sys.argv[3:]:
        ko = [k for k in old if frag in k]
        kn = [k for k in new if frag in k]
        if len(ko) != 1 or len(kn) != 1:
            print(f"{frag}: {len(ko)} / {len(kn)} kernels match")
            bad += 1
            continue
        a, b = normalise(old[ko[0]]), normalise(new[kn[0]])
        same = a == b
        bad += not same
        print(f"{'identical' if same else 'DIFFERENT'}  {len(a):6d} / {len(b):6d} lines  {kn[0]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
