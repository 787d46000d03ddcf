"""Diff the gfx950 kernels of two builds of liblmi_hip.so (CPU only): for every
kernel symbol, the disassembled instruction text with addresses stripped, and
the resource numbers of the code object's metadata (VGPR, AGPR, SGPR, LDS,
scratch).  A refactor of host code must leave both equal.

    python tools/codeobj_diff.py OLD.so NEW.so [substring of the symbols to compare]
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from test_codeobj import OBJDUMP, _disassembly, _functions  # noqa: E402

READELF = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(lib):
    """{symbol: (instruction lines, {resource: value})}"""
    from pathlib import Path
    with tempfile.TemporaryDirectory() as tmp:
        funcs = _functions(_disassembly(Path(tmp), lib))
        notes = "\n".join(subprocess.run([READELF, "--notes", str(f)], check=True, capture_output=True,
                                         text=True).stdout
                          for f in sorted(Path(tmp).iterdir()) if "amdgcn" in f.name and "gfx950" in f.name)
    res = {}
    for block in notes.split("- .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        sym = re.search(r"\.symbol:\s+'?([^\s']+?)\.kd'?\s", block).group(1)
        res[sym] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in KEYS}
    strip = lambda l: re.sub(r"//\s*[0-9A-Fa-f]+:", "//", l)
    # (not instructions: the next code object's banner, elided padding)
    return {n: ([strip(l) for l in ins if "file format" not in l and l != "..."], res.get(n))
            for n, ins in funcs.items() if n in res}


def main(old, new, only=""):
    a, b = kernels(old), kernels(new)
    names = sorted(n for n in set(a) | set(b) if only in n)
    bad = 0
    for n in names:
        if n not in a or n not in b:
            print(("only in new: " if n in b else "only in old: ") + n)
        elif a[n] != b[n]:
            d = sum(x != y for x, y in zip(a[n][0], b[n][0])) + abs(len(a[n][0]) - len(b[n][0]))
            print(f"differs ({d} lines; resources {a[n][1]} -> {b[n][1]}): {n}")
        else:
            continue
        bad += 1
    print(f"{len(names)} kernels compared, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
