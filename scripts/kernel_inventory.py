#!/usr/bin/env python3
"""Kernel inventory of the built library, and what a traced test run launched of it.  No GPU needed.

  scripts/kernel_inventory.py                       every project kernel in the gfx950 code objects of muopdb_amd/libmuopdb_hip.so,
                                                    one demangled name per line (library kernels, rocprim::, are left out)
  scripts/kernel_inventory.py --families            the same, counted by template
  scripts/kernel_inventory.py A.csv B.csv ...       the project kernels that the traced run(s) never launched.  The files are the
                                                    *_kernel_stats.csv / *_kernel_trace.csv of
                                                      rocprofv3 --kernel-trace --stats --output-format csv -- python -m pytest tests -q -m gpu ...
                                                    (kernel trace only, in a run of its own); child processes' files count as well
  ... --launched                                    print the launched project kernels instead
  ... --write-record tests/kernel_launch_record.json --commit REV
                                                    rewrite the record's `commit` and `launched` from the trace, keeping its `exempt` map

Names are the keys of tests.helpers.kernel_key: `ivf_scan_pq2_kernel<1, 16, 4, false, true>`."""
import argparse
import collections
import csv
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import helpers as H  # noqa: E402


def inventory(lib_path):
    with tempfile.TemporaryDirectory() as tmp:
        return sorted(k for k in H.library_kernels(lib_path, tmp) if H.is_project_kernel(k))


def traced_names(paths):
    """kernel keys of every row of the given rocprofv3 CSV files (the stats file's `Name`, the trace file's `Kernel_Name`)"""
    csv.field_size_limit(1 << 30)
    names = set()
    for path in paths:
        with open(path, newline="") as f:
            rd = csv.DictReader(f)
            col = next((c for c in ("Kernel_Name", "Name") if c in (rd.fieldnames or [])), None)
            if col is None:
                raise SystemExit("%s: neither a Kernel_Name nor a Name column" % path)
            for row in rd:
                if row[col]:
                    names.add(H.kernel_key(row[col]))
    return names


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("csv", nargs="*", help="kernel stats / kernel trace CSV files of a traced run")
    ap.add_argument("--lib", default=os.path.join(ROOT, "muopdb_amd", "libmuopdb_hip.so"))
    ap.add_argument("--families", action="store_true")
    ap.add_argument("--launched", action="store_true")
    ap.add_argument("--write-record")
    ap.add_argument("--commit", default="")
    a = ap.parse_args()
    inv = inventory(a.lib)
    if not a.csv:
        if a.families:
            for fam, cnt in collections.Counter(k.split("<")[0] for k in inv).most_common():
                print("%4d %s" % (cnt, fam))
        else:
            print("\n".join(inv))
        print("%d project kernels" % len(inv), file=sys.stderr)
        return 0
    seen = traced_names(a.csv)
    launched = sorted(set(inv) & seen)
    never = sorted(set(inv) - seen)
    foreign = sorted(k for k in seen - set(inv) if "_kernel" in k and H.is_project_kernel(k) and not k.startswith(("at::", "void at::")))
    print("\n".join(launched if a.launched else never))
    print("%d project kernels, %d launched, %d never launched" % (len(inv), len(launched), len(never)), file=sys.stderr)
    if foreign:   # a name the library does not hold: another build was traced, or the two demanglers disagree
        print("traced *_kernel names that are not in the library: %s" % "; ".join(foreign[:10]), file=sys.stderr)
    if a.write_record:
        rec = {"exempt": {}}
        if os.path.exists(a.write_record):
            with open(a.write_record) as f:
                rec = json.load(f)
        rec["commit"] = a.commit or rec.get("commit", "")
        rec["launched"] = launched
        rec.setdefault("exempt", {})
        with open(a.write_record, "w") as f:
            json.dump({k: rec[k] for k in ("commit", "launched", "exempt")}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
