// hnsw_route_main.cpp — muopdb_amd/csrc/mdb_hnsw_route.h alone, as a program: reads one case per line from stdin and prints its route.
// A case is blank-separated `key=value` words: the shape's (the words of mdb_hnsw_describe_search's `shape` line), the call's
// (b, k, ef, qstride, users, fuse, filter) and options by their field name (hnsw_rank=3); what a line leaves out keeps its default.
// Per case: the launch lines in the format of mdb_hnsw_describe_search (or `unsupported`), a `# launches`, a `# scratch` and a
// `# facts` line, then `end`.  tests/test_hnsw_route.py builds it plain and under -fsanitize=address,undefined; no HIP header, no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../muopdb_amd/csrc/mdb_hnsw_route.h"

static bool set_word(const std::string& key, long long v, HnswShape& s, HnswCall& c, HnswRouteOpts& o) {
#define F(obj, name, field, type) \
    if (key == name) { obj.field = (type)v; return true; }
    F(s, "kind", kind, int) F(s, "metric", metric, int) F(s, "dimension", dimension, uint32_t) F(s, "dpad", dpad, int)
    F(s, "max_n", max_n, uint32_t) F(s, "max_stride", max_stride, uint32_t) F(s, "max_rows0", max_rows0, uint32_t)
    F(s, "max_rowsU", max_rowsU, uint32_t) F(s, "all_dense", all_dense, bool) F(s, "pq_m", pq_m, int) F(s, "pq_K", pq_K, int)
    F(s, "pq_subdim", pq_subdim, int) F(s, "nu", nu, uint32_t) F(s, "nu2", nu2, uint32_t) F(s, "su", su, uint32_t)
    F(s, "layers", layers, uint32_t) F(s, "small_layer", small_layer, uint32_t) F(s, "ntiles", ntiles, uint64_t)
    F(s, "ntiles2", ntiles2, uint64_t) F(s, "rows_nat", rows_nat, bool) F(s, "map21", map21, bool)
    F(c, "b", b, uint64_t) F(c, "k", k, uint64_t) F(c, "ef", ef, uint32_t) F(c, "qstride", qstride, int)
    F(c, "users", per_query_users, bool) F(c, "fuse", fuse, bool) F(c, "filter", filter, bool)
#define X(field, dflt) F(o, #field, field, long long)
    HNSW_ROUTE_OPTS(X)
#undef X
#undef F
    return false;
}

int main() {
    std::string line;
    static char text[8192];
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        HnswShape s;
        HnswCall c;
        HnswRouteOpts o;
        std::istringstream words(line);
        std::string w;
        while (words >> w) {
            const size_t eq = w.find('=');
            if (eq == std::string::npos || !set_word(w.substr(0, eq), atoll(w.c_str() + eq + 1), s, c, o)) {
                fprintf(stderr, "unknown word `%s`\n", w.c_str());
                return 2;
            }
        }
        const HnswRoute r = hnsw_route(s, c, o);
        if (r.status != MDB_OK) {
            printf("unsupported\nend\n");
            continue;
        }
        hnsw_route_text(r, text, sizeof text);
        fputs(text, stdout);
        printf("# launches");   // per launch what the argument builder reads: layer_hi/handover/fb_role/zero16/q_first/cl_tlds
        for (int i = 0; i < r.n; ++i) {
            const HnswLaunch& l = r.launch[i];
            printf(" %d/%d/%d/%d/%u/%d", l.layer_hi, (int)l.handover, l.fb_role, (int)l.zero16, l.q_first, (int)l.cl_tlds);
        }
        printf("\n");
        printf("# scratch table=%zu out=%zu hand=%zu vis=%zu ovf=%zu cnt=%zu visw=%zu fb=%zu\n", r.table_bytes, r.out_bytes, r.hand_bytes,
               r.vis_bytes, r.st_ovf, r.st_cnt, r.st_vis, r.st_fb);
        printf("# facts ef=%u vis_lds=%d table=%d fuse=%d cf=%d local=%d wcap=%d stage=%u,%u,%u\n", r.ef, (int)r.vis_lds, (int)r.table,
               (int)r.fuse_done, (int)r.cf_done, (int)r.local, r.wcap, r.stage.dtab_off, r.stage.rows0_off, r.stage.rowsU_off);
        printf("end\n");
    }
    return 0;
}
