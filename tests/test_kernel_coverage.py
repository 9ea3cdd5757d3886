"""Every kernel compiled into libmuopdb_hip.so has been launched under the GPU suite's parity checks, or is listed with the dispatch
condition that keeps every input away from it.  Runs without a GPU.

tests/kernel_launch_record.json holds the project kernels that a kernel-traced run of `pytest tests -m gpu` launched (taken with
scripts/kernel_inventory.py at the commit it names) and an `exempt` map from a kernel name, or an fnmatch pattern over its template
arguments, to a one-line reason.  The inventory of the built library (the `.kd` descriptors of its gfx950 code objects, rocprim's
left out) must equal launched + exempt exactly: a new instantiation needs a test and a fresh record, or a reason; a name that is
gone must leave the record.

The record is only as fresh as its last traced GPU run.  This test guards the SET of kernels, not their behaviour: a test that
stops reaching an instantiation without the library changing goes unnoticed until the suite is traced again."""
import collections
import fnmatch
import json
import os

import pytest

from muopdb_amd import lib as L
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "kernel_launch_record.json")
MAX_EXEMPT_SHARE = 0.05

pytestmark = pytest.mark.skipif(not H.have_llvm_tools("llvm-objdump", "llvm-readelf"), reason="llvm-objdump / llvm-readelf not installed")


@pytest.fixture(scope="module")
def inventory(tmp_path_factory):
    return {k for k in H.library_kernels(L.LIB_PATH, tmp_path_factory.mktemp("code_objects")) if H.is_project_kernel(k)}


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        return json.load(f)


def _family(key):
    return key.split("<")[0]


def _exempted(inventory, patterns):
    return {k for k in inventory if any(fnmatch.fnmatchcase(k, p) for p in patterns)}


def test_inventory_reads_the_library(inventory):
    fam = collections.Counter(_family(k) for k in inventory)
    assert len(inventory) >= 500 and fam["ivf_scan_pq2_kernel"] >= 32 and fam["hnsw_beam_kernel"] >= 32
    assert "remap_kernel" in inventory and not any(k.startswith("rocprim::") for k in inventory)
    assert H.kernel_key("void ivf_scan_f32_kernel<0, 256>(ScanArgs, HIP_vector_type<float, 4u> const*, DistPlan, float const*, int) (.kd)") == \
        H.kernel_key("void ivf_scan_f32_kernel<0, 256>(ScanArgs, HIP_vector_type<float, 4u> const*, DistPlan, float const*, int)") == \
        "ivf_scan_f32_kernel<0, 256>"


def test_every_kernel_is_launched_or_exempt(inventory, record):
    launched, exempt = set(record["launched"]), _exempted(inventory, record["exempt"])
    assert len(launched) == len(record["launched"]), "duplicate names in the record"
    missing = sorted(inventory - launched - exempt)
    assert not missing, ("%d kernels in the library with no recorded launch and no exemption (add a parity case and trace the suite "
                         "again, or stop instantiating them): %s" % (len(missing), "; ".join(missing[:12])))
    gone = sorted(launched - inventory)
    assert not gone, "%d recorded kernels that the library no longer holds: %s" % (len(gone), "; ".join(gone[:12]))
    both = sorted(launched & exempt)
    assert not both, "kernels recorded as launched AND exempt: %s" % "; ".join(both[:12])


def test_exemptions_are_few_live_and_reasoned(inventory, record):
    assert record.get("commit"), "the record names the commit it was taken at"
    exempt = _exempted(inventory, record["exempt"])
    dead = sorted(p for p in record["exempt"] if not any(fnmatch.fnmatchcase(k, p) for k in inventory))
    assert not dead, "exemptions that match no kernel of the library: %s" % "; ".join(dead)
    assert all(isinstance(r, str) and len(r.strip()) >= 20 for r in record["exempt"].values()), "every exemption says which dispatch condition excludes it"
    assert len(exempt) <= MAX_EXEMPT_SHARE * len(inventory), "%d of %d kernels exempt: more than 5 %%" % (len(exempt), len(inventory))
    sizes = collections.Counter(_family(k) for k in inventory)
    whole = sorted(f for f, c in collections.Counter(_family(k) for k in exempt).items() if c == sizes[f])
    assert not whole, "whole kernel families exempt: %s" % ", ".join(whole)
