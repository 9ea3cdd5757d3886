"""The "Limits" block of include/muopdb_hip.h, its copy in INTEGRATION.md and the sources say the same (no GPU needed): the numbers
a binder reads are MDB_MAX_K, HNSW_MAX_STRIDE and the shard merges' LDS formulas as the code has them today."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muopdb_amd", "csrc")


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def define(text, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, flags=re.M)
    assert m, "#define %s not found" % name
    return int(m.group(1))


def header_rows():
    text = read(ROOT, "include", "muopdb_hip.h")
    block = text[text.index("---- Limits"):]
    block = block[:block.index("*/")]
    return block, [ln[3:].strip() for ln in block.splitlines() if ln.startswith(" * | ")]


def integration_rows():
    text = read(ROOT, "INTEGRATION.md")
    sec = text[text.index("## 7. Limits"):]
    return sec, [ln.strip() for ln in sec.splitlines() if ln.startswith("| ") and not ln.startswith("|---")]


def row_of(rows, entry):
    hits = [r for r in rows if entry in r.split("|")[1]]
    assert len(hits) == 1, (entry, hits)
    return hits[0]


def test_the_two_tables_are_the_same():
    _, h = header_rows()
    _, m = integration_rows()
    assert len(h) >= 15 and h == m


def test_documented_numbers_follow_the_sources():
    max_k = define(read(CSRC, "mdb_files.h"), "MDB_MAX_K")
    hnsw = read(CSRC, "mdb_hnsw.hip")
    stride = define(hnsw, "HNSW_MAX_STRIDE")
    # the checks the table's ef and layer limits restate (the ef limit is the route's: mdb_hnsw_route.h)
    assert "ef > MDB_MAX_K * 2" in read(CSRC, "mdb_hnsw_route.h") and "o.num_layers > 255" in hnsw
    assert "max_neighbors > 64" in read(CSRC, "mdb_hnsw_build.hip")
    assert "num_bits must be 1..8" in read(CSRC, "mdb_core.hip")
    # the loaders' own limits are checked by their host half (mdb_files.cpp), with numbers the kernels' file holds equal to its own
    files, files_h = read(CSRC, "mdb_files.cpp"), read(CSRC, "mdb_files.h")
    assert define(files_h, "MDB_HNSW_MAX_DEGREE") == stride and define(files_h, "MDB_HNSW_MAX_LAYERS") == 255
    assert "static_assert(HNSW_MAX_STRIDE == MDB_HNSW_MAX_DEGREE && MDB_HNSW_MAX_LAYERS == 255" in hnsw
    assert "o.num_layers > MDB_HNSW_MAX_LAYERS" in files and "S0 > MDB_HNSW_MAX_DEGREE || SU > MDB_HNSW_MAX_DEGREE" in files
    assert 'MDB_ERR_UNSUPPORTED, "PQ codes are u8: num_bits must be 1..8"' in files
    for block, rows in (header_rows(), integration_rows()):
        assert "MDB_MAX_K = %d" % max_k in block and "2 * MDB_MAX_K = %d" % (2 * max_k) in block and "HNSW_MAX_STRIDE = %d" % stride in block
        for entry in ("mdb_flat_search", "mdb_ivf_search,", "mdb_hnsw_ann_search"):
            assert "k <= %d" % max_k in row_of(rows, entry), entry
        assert "ef <= %d" % (2 * max_k) in row_of(rows, "mdb_hnsw_ann_search")
        for entry in ("mdb_ivf_find_nearest_centroids", "mdb_ivf_coarse_keys", "mdb_ivf_merge_coarse_keys"):
            assert re.search(r"num_probes <= (min\()?%d\b" % max_k, row_of(rows, entry)), entry
        assert "max_clusters_per_vector <= min(%d," % max_k in row_of(rows, "mdb_ivf_assign")
        assert "node degree <= %d" % stride in row_of(rows, "mdb_hnsw_load") and "num_layers <= 255" in row_of(rows, "mdb_hnsw_load")
        assert "max_neighbors <= 64" in row_of(rows, "mdb_hnsw_select_neighbors")
        sp = row_of(rows, "mdb_spann_search*")
        assert "top_k <= %d" % max_k in sp and "num_explored_centroids <= %d" % max_k in sp and "ef_construction <= %d" % (2 * max_k) in sp


def test_documented_merge_capacities_follow_the_formulas_in_the_sources():
    max_k = define(read(CSRC, "mdb_files.h"), "MDB_MAX_K")
    ivf, spann = read(CSRC, "mdb_ivf.hip"), read(CSRC, "mdb_spann.hip")
    # IvfSet::merge_points and merge_shards_launch: the formulas and the budget as the table states them
    assert "lds = world * k * 8 + k * 20 + (world + 1) * 4 + 16;\n    if (lds > 150 * 1024)" in ivf
    assert "lds = world * k * 20 + (world + 1) * 4 + 16;\n    if (lds > 150 * 1024)" in spann
    budget = 150 * 1024

    def points(world):
        return min(max_k, (budget - (world + 1) * 4 - 16) // (world * 8 + 20))

    def rows_(world):
        return (budget - (world + 1) * 4 - 16) // (world * 20)

    for _, rows in (header_rows(), integration_rows()):
        p = row_of(rows, "mdb_ivf_merge_shards")
        assert "world * k * 8 + k * 20 + (world + 1) * 4 + 16 <= %d" % budget in p
        assert points(6) == max_k and "(k <= %d up to world = 6, %d at world = 7, %d at world = 8)" % (max_k, points(7), points(8)) in p
        r = row_of(rows, "mdb_merge_shards,")
        assert "world * k * 20 + (world + 1) * 4 + 16 <= %d" % budget in r
        assert "(k <= %d / %d / %d at world = 2 / 4 / 8)" % (rows_(2), rows_(4), rows_(8)) in r
