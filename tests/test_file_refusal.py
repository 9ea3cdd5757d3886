"""The loaders' host halves (muopdb_amd/csrc/mdb_files.cpp) against the mutation table (tests/file_mutations.py), without a GPU.

`mdb_*_load` takes host mappings of on-disk files and turns them into device offsets the kernels trust: what the host half lets through,
a kernel later dereferences.  The host half of each loader is one function that the loader calls first and the `mdb_*_check_files` entry
calls alone, so every status asserted here is the loader's (tests/test_gpu_file_refusal.py holds the loaders to it on a device).

- every case returns its expected status; a refusal carries a message that names the check the case aims at, an acceptance none;
- every MDB_ERR_FORMAT / MDB_ERR_UNSUPPORTED message of the host half is produced by at least one case (UNREACHED: a cap, not a
  measurement);
- the same cases through a stand-alone program built with -fsanitize=address,undefined, every file in a heap block of exactly its
  length: no report, the same statuses;
- the whole table runs in seconds: a case that does not has found an allocation sized by a file field."""
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

from muopdb_amd import lib as L
from tests import file_mutations as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muopdb_amd", "csrc")

# Refusals of the host half that no file of the table reaches, with the reason.  At most three: past that, delete dead checks.
UNREACHED = {
    "HNSW point ids are u32": "needs a vector file of 2^32 - 1 rows: every smaller file that claims so many is refused for its length first",
    "IVF point ids are u32": "needs a doc-id section of 64 GiB: every smaller one is too short for the header's count and refused for that first",
    "too many posting-list slots": "needs 2^28 16-slot units — e.g. 16 384 lists over one 262 144-id Elias-Fano blob: 1.5 MB of files, but "
                                   "3 GB of tile tables before the sum passes the limit; the check runs per list, before the next list's rows "
                                   "are appended",
}


@pytest.fixture(scope="module")
def results():
    """{case name: (status, message, seconds)} of the whole table through the ctypes checkers"""
    L.load()
    out = {}
    for c in M.cases():
        t = time.perf_counter()
        st, msg = M.check(c)
        out[c.name] = (st, msg, time.perf_counter() - t)
    return out


def test_the_table_holds_what_it_says():
    cases = M.cases()
    names = {c.name for c in cases}
    assert len(cases) >= 1000 and len(names) == len(cases)
    by_loader = {l: sum(c.loader == l for c in cases) for l in M.LOADER_IDS}
    assert all(by_loader[l] >= 100 for l in by_loader), by_loader
    assert sum(c.status == M.OK for c in cases) >= 12 and sum(c.status == M.UNSUPPORTED for c in cases) >= 8
    # the base files are what the issue asks for: >= 3 layers, 7 lists with an empty one, 3 users
    B = M.base()
    assert M.hnsw_layout(B["hnsw"][1]["index"])["num_layers"] == 3 and M.hnsw_layout(B["hnsw_pq"][1]["index"])["quantized_dimension"] == M.M
    lay = M.ivf_layout(B["ivf"][1]["index"])
    assert lay["num_clusters"] == 7 and lay["num_vectors"] == 300
    assert 0 in [int(np.frombuffer(B["ivf"][1]["index"][o:o + 8], np.uint64)[0]) for o in lay["lists"]]
    assert len(B["multi"][1]["user_table"]) == 3 * 112


def test_every_case_returns_its_status_and_a_message(results):
    wrong = []
    for c in M.cases():
        st, msg, _ = results[c.name]
        if st != c.status:
            wrong.append("%s: expected %s, got %s (%r)" % (c.name, L.STATUS_NAMES[c.status], L.STATUS_NAMES.get(st, st), msg))
        elif (st == M.OK) != (msg == ""):
            wrong.append("%s: status %s with message %r" % (c.name, L.STATUS_NAMES[st], msg))
        elif c.aim not in msg:
            wrong.append("%s: refused by %r, the case aims at %r" % (c.name, msg, c.aim))
    assert not wrong, "%d of %d cases:\n%s" % (len(wrong), len(M.cases()), "\n".join(wrong))


def test_unmutated_files_are_accepted():
    for name, (loader, files, args) in M.base().items():
        st, msg = M.check(M.Case("base." + name, loader, files, args, M.OK, ""))
        assert (st, msg) == (M.OK, ""), (name, st, msg)


def test_the_table_runs_in_seconds(results):
    """nothing is allocated from a field before the field is bounded: the fields set to 2^63 and 2^64 - 1 cost what the others cost"""
    slow = sorted(((t, n) for n, (_, _, t) in results.items()), reverse=True)[:3]
    first = M.cases()[0].name                      # (the first call also loads the library)
    assert all(t < 1.0 for t, n in slow if n != first), slow
    assert sum(t for _, _, t in results.values()) < 20.0


def _literal_pattern(lit):
    """a printf literal as a regular expression over the message it formats"""
    parts = re.split(r"%(?:zu|llu|u|d|s)", lit)
    return re.compile("^" + ".*".join(re.escape(p) for p in parts) + "$", re.S)


def refusal_sites():
    """{message literal: status name} of every `fail(why, MDB_ERR_FORMAT | MDB_ERR_UNSUPPORTED, "...")` of mdb_files.cpp and every message
    ef_header_error (mdb_files.h) returns — the host half's refusals, read from the sources as tests/test_nan_sites.py reads its raises"""
    with open(os.path.join(CSRC, "mdb_files.cpp")) as f:
        text = f.read()
    found = [(m.group(2), m.group(1)) for m in re.finditer(r'fail\(why,\s*MDB_ERR_(FORMAT|UNSUPPORTED),\s*"((?:[^"\\]|\\.)*)"', text)]
    sites = dict(found)
    # one message per site: a literal shared by two checks would let either be dead behind the other's case
    assert len(sites) == len(found), sorted(lit for lit, _ in found if [l for l, _ in found].count(lit) > 1)
    assert len(re.findall(r"MDB_ERR_(?:FORMAT|UNSUPPORTED)", text)) == \
        len(re.findall(r'fail\(why,\s*MDB_ERR_(?:FORMAT|UNSUPPORTED),\s*"', text)), "a refusal of mdb_files.cpp that is not `fail(why, status, \"literal\"`"
    with open(os.path.join(CSRC, "mdb_files.h")) as f:
        head = f.read()
    body = head[head.index("ef_header_error("):]
    body = body[:body.index("return nullptr;")]
    for m in re.finditer(r'return\s+"((?:[^"\\]|\\.)*)";', body):
        sites[m.group(1)] = "FORMAT"
    return sites


def test_the_loaders_hold_no_refusal_of_their_own():
    """the rules are in ONE place: what is left of the loaders in the .hip files decides nothing from a file's bytes"""
    for name, body_start, body_end in (("mdb_hnsw.hip", "mdb_status HnswSet::load(", "// ---- uploads"),
                                       ("mdb_ivf.hip", "mdb_status IvfSet::load(", "// ---- uploads")):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        head = text[text.index(body_start):]
        head = head[:head.index(body_end)]
        assert "plan_files(" in head and "MDB_ERR_FORMAT" not in head and "MDB_ERR_UNSUPPORTED" not in head and "rd_u" not in head, name
    # the SPANN loaders plan BOTH halves with the checkers' own function before they upload either
    with open(os.path.join(CSRC, "mdb_spann.hip")) as f:
        spann = f.read()
    for entry in ("mdb_status mdb_spann_load(", "mdb_status mdb_multi_spann_load("):
        body = spann[spann.index(entry):]
        body = body[:body.index("\n}\n")]
        assert "spann_plan_files(" in body and body.index("spann_plan_files(") < body.index(".upload(") and ".load(" not in body, entry
        assert "MDB_ERR_FORMAT" not in body and "MDB_ERR_UNSUPPORTED" not in body, entry
    with open(os.path.join(CSRC, "mdb_files.cpp")) as f:
        host = f.read()
    assert host.count("spann_plan_files(") == 3   # its definition, mdb_spann_check_files, mdb_multi_spann_check_files
    with open(os.path.join(CSRC, "mdb_files.h")) as f:
        host += f.read()
    assert not re.search(r"#include\s*[<\"]hip/|\bhip[A-Z]\w*\s*\(|__global__|__device__", host), "the host half must compile without HIP headers"
    assert "mdb_ctx" not in re.sub(r"//[^\n]*", "", host) and "getenv" not in host


def test_every_refusal_site_is_reached(results):
    sites = refusal_sites()
    assert len(sites) >= 40, sorted(sites)
    assert len(UNREACHED) <= 3 and set(UNREACHED) <= set(sites), sorted(set(UNREACHED) - set(sites))
    produced = [(st, msg) for st, msg, _ in results.values() if st in (M.FORMAT, M.UNSUPPORTED)]
    missing, wrong_status = [], []
    for lit, status in sorted(sites.items()):
        pat = _literal_pattern(lit)
        # ef_header_error's messages arrive inside "posting list %u: %s"
        hits = [st for st, msg in produced if pat.match(msg) or pat.match(msg.split(": ", 1)[-1])]
        if not hits and lit not in UNREACHED:
            missing.append(lit)
        if hits and lit in UNREACHED:
            missing.append("%s (listed in UNREACHED, but reached)" % lit)
        if any(L.STATUS_NAMES[st] != "MDB_ERR_" + status for st in hits):
            wrong_status.append(lit)
    assert not missing, "refusals of the host half that no case of tests/file_mutations.py produces (add a file that reaches the check, or " \
                        "delete a dead check):\n%s" % "\n".join(missing)
    assert not wrong_status, wrong_status


def _sanitizer_compiler():
    """(compiler, extra flags) for a binary with the sanitizer runtimes linked STATICALLY: it then runs in whatever environment the
    suite runs in (a dynamically linked runtime insists on being the first library loaded).  clang++ links them statically by default."""
    for cxx, flags in (("/opt/rocm/llvm/bin/clang++", []), ("clang++", []), ("g++", ["-static-libasan", "-static-libubsan"])):
        path = shutil.which(cxx)
        if path:
            return path, flags
    return None, []


def test_the_table_under_the_host_sanitizers(results, tmp_path):
    """tests/host/check_files_main.cpp + the host half alone, -fsanitize=address,undefined, run as a child process in the suite's own environment: every
    file in a heap block of exactly its length.  An entry point no layer lists, an edge of a slot no search reads, a length that wraps an
    offset: what reads a host array out of bounds on the way to a plan ends this run with a report."""
    cxx, static_runtime = _sanitizer_compiler()
    assert cxx, "no host C++ compiler"
    exe, bundle = str(tmp_path / "check_files"), str(tmp_path / "cases.bin")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_runtime,
                            os.path.join(ROOT, "tests", "host", "check_files_main.cpp"), os.path.join(CSRC, "mdb_files.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    M.write_bundle(bundle, M.cases())
    run = subprocess.run([exe, bundle], capture_output=True, text=True, timeout=300)   # the suite's own environment, untouched
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, \
        "exit %d after %d cases\n%s" % (run.returncode, len(run.stdout.splitlines()), run.stderr[-6000:])
    got = dict(line.rsplit(" ", 1) for line in run.stdout.splitlines())
    assert got == {c.name: str(results[c.name][0]) for c in M.cases()}
