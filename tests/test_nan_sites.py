"""Every place a kernel raises MDB_FLAG_NAN (muopdb_amd/csrc) has its own idea of when a NaN distance counts: the reference panics
only on distances it EVALUATES (NotNan::new(..).unwrap()), and several kernels compute distances it never does.  So each raise must
be claimed by a GPU test that reaches it — the table SITES of tests/test_gpu_nonfinite.py — and a new raise, or a claim on a test
that is gone, fails here with a message saying to add a case.  Runs without a GPU."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muopdb_amd", "csrc")

_NOT_A_DEFINITION = ("template", "typedef", "using", "struct", "class", "namespace", "extern", "return", "enum", "union")


def _definition_name(line):
    """the function that a column-0 line `[static] [__global__] [__launch_bounds__(..)] type name(` defines or declares, or None"""
    if not line or not (line[0].isalpha() or line[0] == "_") or line.split(None, 1)[0] in _NOT_A_DEFINITION:
        return None
    head = re.sub(r"__launch_bounds__\s*\([^)]*\)", " ", line)
    if "(" not in head:
        return None
    words = re.findall(r"[A-Za-z_]\w*", head[:head.index("(")])
    return words[-1] if len(words) >= 2 else None   # (a lone word before the parenthesis is a macro call, not a definition)


def nan_sites():
    """{"file::function": number of `atomicOr(.., MDB_FLAG_NAN)` raises in it}"""
    sites = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not path.endswith((".hip", ".h")):
            continue
        with open(path) as f:
            lines = f.read().splitlines()
        current = None
        for line in lines:
            name = _definition_name(line)
            if name:
                current = name
            if re.search(r"atomicOr\s*\([^;]*\bMDB_FLAG_NAN\b", line):
                assert current, "%s: a NaN raise before any definition" % path
                key = "%s::%s" % (os.path.basename(path), current)
                sites[key] = sites.get(key, 0) + 1
    return sites


def claimed_sites():
    """the dict literal SITES of tests/test_gpu_nonfinite.py, read as text: {"file::function": (raises, "module::test")}"""
    with open(os.path.join(ROOT, "tests", "test_gpu_nonfinite.py")) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "SITES" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("tests/test_gpu_nonfinite.py defines no SITES table")


def _module_tests(module):
    """names of the module-level test functions of tests/<module>.py"""
    with open(os.path.join(ROOT, "tests", module + ".py")) as f:
        tree = ast.parse(f.read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_site_scan_finds_the_known_raises():
    sites = nan_sites()
    assert sites.get("mdb_flat.hip::flat_scan_kernel") == 1 and sites.get("mdb_hnsw.hip::hnsw_beam_kernel", 0) >= 3
    assert sum(sites.values()) >= 26
    assert not any("mdb_core.hip" in k or "mdb_common.h" in k for k in sites)   # the flag's definition and its reader raise nothing


def test_every_nan_raise_is_claimed_by_a_gpu_test():
    sites, claimed = nan_sites(), claimed_sites()
    missing = sorted(k for k in sites if k not in claimed)
    assert not missing, "kernels that raise MDB_FLAG_NAN and no case of tests/test_gpu_nonfinite.py claims (add a hit / miss case " \
                        "that reaches the kernel and name it in SITES): %s" % ", ".join(missing)
    grown = sorted("%s (%d raises, %d claimed)" % (k, n, claimed[k][0]) for k, n in sites.items() if claimed[k][0] != n)
    assert not grown, "the number of MDB_FLAG_NAN raises changed (check that the claiming case reaches the new raise, then update " \
                      "SITES): %s" % ", ".join(grown)


def test_claims_name_live_sites_and_live_tests():
    sites, claimed = nan_sites(), claimed_sites()
    stale = sorted(set(claimed) - set(sites))
    assert not stale, "SITES claims kernels that raise MDB_FLAG_NAN no longer: %s" % ", ".join(stale)
    gone = []
    for key, (_, test_id) in sorted(claimed.items()):
        module, _, name = test_id.partition("::")
        module = module.rsplit(".", 1)[-1]
        if not os.path.exists(os.path.join(ROOT, "tests", module + ".py")) or name not in _module_tests(module):
            gone.append("%s -> %s" % (key, test_id))
    assert not gone, "SITES names tests that do not exist (add a case that reaches the kernel): %s" % "; ".join(gone)
