"""Every tuning / test switch of MDB_OPTIONS (muopdb_amd/csrc/mdb_common.h) selects a kernel form or a threshold of the dispatch, so
each one must be named by some GPU test (tests/test_gpu_*.py) — or be listed below with the reason it needs none.  Runs without a GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# print-only switches: they add diagnostics to stderr and change no kernel form or result
EXEMPT = {
    "MDB_MF_DBG": "prints the batched flat path's candidate counts; no form or result changes",
    "MDB_CM_DBG": "prints the coarse matrix-core search's candidates per query; no form or result changes",
    "MDB_HNSW_DBG": "prints HNSW traversal diagnostics; no form or result changes",
    "MDB_PQF_DBG": "prints the fused IVF-PQ step's phase cycle counts; no form or result changes",
}


def option_names():
    with open(os.path.join(ROOT, "muopdb_amd", "csrc", "mdb_common.h")) as f:
        src = f.read()
    block = src[src.index("#define MDB_OPTIONS(X)"):]
    block = block[:block.index("struct mdb_options")]
    return re.findall(r'X\(\s*\w+\s*,\s*"(MDB_[A-Z0-9_]+)"', block)


def gpu_test_text():
    text = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))):
        with open(path) as f:
            text.append(f.read())
    return "\n".join(text)


def test_option_table_parses():
    names = option_names()
    assert len(names) == len(set(names)) >= 60
    assert "MDB_FLAT_NO_MFMA" in names and "MDB_PQ3_BLOCK" in names


def test_every_option_is_named_by_a_gpu_test():
    names = option_names()
    text = gpu_test_text()
    # a name counts where it stands whole: as a string ("MDB_X") or as a keyword (MDB_X=1), never as the prefix of a longer name
    missing = [n for n in names if n not in EXEMPT and not re.search(r"(?<![A-Z0-9_])%s(?![A-Z0-9_])" % n, text)]
    assert not missing, "options no GPU test names (add a parity case, or an exemption with its reason): %s" % ", ".join(missing)


def test_exemptions_are_live_options():
    names = set(option_names())
    stale = sorted(set(EXEMPT) - names)
    assert not stale, "exempted names that are no longer options: %s" % ", ".join(stale)
    assert all(r.strip() for r in EXEMPT.values())
