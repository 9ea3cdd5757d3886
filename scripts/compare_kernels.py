#!/usr/bin/env python3
"""Do two builds of the library hold the same device code?  No GPU needed.

  scripts/compare_kernels.py OLD.so NEW.so

Unbundles the gfx950 code objects of both libraries and compares, per symbol,
  * the disassembled instruction text (addresses and encodings dropped: they move with the layout; the padding behind a function's
    last instruction is dropped too), and
  * per kernel, the register, spill, LDS and scratch figures of the code objects' metadata notes.
The order of the symbols inside a code object is not compared: it follows the order of instantiation in the source.
Prints one summary line and exits 0 when nothing differs, 1 otherwise.  The tool for a refactor of the host-side dispatch, and the first
thing to run after a change that is meant to add or remove instantiations only."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import helpers as H  # noqa: E402

META = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
PADDING = re.compile(r"^(\.\.\.|s_code_end|s_nop 0|v_illegal)$")


def bodies(listing):
    """symbol -> instruction lines of an `llvm-objdump -d` listing"""
    syms, cur = {}, None
    for line in listing.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:\s*$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s+", " ", re.sub(r"\s*//.*$", "", line)).strip())
    for body in syms.values():
        while body and PADDING.match(body[-1]):
            body.pop()
    return syms


def metadata(workdir, obj):
    """kernel name -> the META figures of the code object's amdhsa.kernels note"""
    text = subprocess.run([os.path.join(H.LLVM, "llvm-readelf"), "--notes", obj], cwd=workdir, check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for line in text.splitlines():
        m = re.match(r"^  (- |  )(\.\w+):\s*(.*)$", line)   # a kernel's own keys: one list level below `amdhsa.kernels:`
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if m.group(2) == ".name":
            out[m.group(3).strip("'\"")] = cur
        elif m.group(2) in META:
            cur[m.group(2)] = m.group(3)
    return out


def load(lib):
    code, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in H.extract_code_objects(lib, tmp):
            for sym, body in bodies(H.disassemble(tmp, obj)).items():
                code.setdefault(sym, []).append(body)
            meta.update(metadata(tmp, obj))
    return code, meta


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    (ca, ma), (cb, mb) = load(sys.argv[1]), load(sys.argv[2])
    only_a, only_b = sorted(set(ca) - set(cb)), sorted(set(cb) - set(ca))
    code_diff = sorted(s for s in ca if s in cb and ca[s] != cb[s])
    meta_diff = sorted(k for k in set(ma) | set(mb) if ma.get(k) != mb.get(k))
    for title, names in (("only in " + sys.argv[1], only_a), ("only in " + sys.argv[2], only_b), ("instructions differ", code_diff),
                         ("metadata differs", meta_diff)):
        for n in names[:20]:
            print("%s: %s" % (title, n))
    for s in code_diff[:5]:
        x, y = ca[s][0], cb[s][0]
        i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        print("  %s: %d / %d instructions, first difference at %d: %s | %s" % (s[:80], len(x), len(y), i, x[i] if i < len(x) else "-", y[i] if i < len(y) else "-"))
    print("%d / %d symbols, %d / %d kernels with metadata (%d of them with every figure); only in one: %d, instructions differ: %d, metadata differs: %d"
          % (len(ca), len(cb), len(ma), len(mb), sum(1 for v in mb.values() if len(v) == len(META)), len(only_a) + len(only_b), len(code_diff), len(meta_diff)))
    return 1 if only_a or only_b or code_diff or meta_diff else 0


if __name__ == "__main__":
    sys.exit(main())
