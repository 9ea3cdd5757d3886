// check_files_main.cpp — runs a bundle of cases (tests/file_mutations.py: write_bundle) through the host-only file checkers and
// prints `name status` per case.  tests/test_file_refusal.py builds this file together with muopdb_amd/csrc/mdb_files.cpp under
// -fsanitize=address,undefined: every file of a case is copied into a heap block of EXACTLY its length, so a checker that reads one
// byte past a file, indexes a host array with an unchecked file field or wraps an offset ends the run with a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/muopdb_hip.h"

struct Reader {
    FILE* f;
    bool ok = true;
    void bytes(void* dst, size_t n) {
        if (n && fread(dst, 1, n, f) != n) ok = false;
    }
    uint32_t u32() { uint32_t v = 0; bytes(&v, 4); return v; }
    uint64_t u64() { uint64_t v = 0; bytes(&v, 8); return v; }
};

// a file of the case in a block of exactly its length (an empty file: a one-byte block that is never to be read, length 0)
struct Blob {
    uint8_t* p = nullptr;
    size_t len = 0;
    void read(Reader& r) {
        len = (size_t)r.u64();
        if (!r.ok || len > ((size_t)1 << 30)) { r.ok = false; len = 0; return; }
        p = (uint8_t*)malloc(len ? len : 1);
        r.bytes(p, len);
    }
    ~Blob() { free(p); }
};

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s BUNDLE\n", argv[0]); return 2; }
    Reader r{fopen(argv[1], "rb")};
    if (!r.f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t count = r.u32();
    for (uint32_t c = 0; c < count && r.ok; ++c) {
        std::string name(r.u32(), '\0');
        r.bytes(&name[0], name.size());
        const uint32_t loader = r.u32();
        uint64_t a[16];
        r.bytes(a, sizeof a);
        Blob files[7], codebook;   // index, vectors, hnsw_index, hnsw_vectors, ivf_index, ivf_vectors, user_table
        for (Blob& b : files) b.read(r);
        codebook.read(r);
        if (!r.ok) break;
        mdb_quant_desc q{};
        q.kind = (mdb_quant_kind)a[3];
        q.metric = (mdb_metric)a[4];
        q.dimension = (uint32_t)a[5];
        q.subvector_dimension = (uint32_t)a[6];
        q.num_bits = (uint32_t)a[7];
        q.codebook = a[8] ? (const float*)codebook.p : nullptr;
        q.codebook_len = a[8] ? codebook.len / 4 : 0;
        const mdb_quant_desc* qp = a[2] ? &q : nullptr;
        char why[600];
        memset(why, 'x', sizeof why);
        mdb_status st = MDB_ERR_INVALID_ARG;
        switch (loader) {
        case 0:
            st = mdb_hnsw_check_files(files[0].p, files[0].len, (size_t)a[0], files[1].p, files[1].len, (size_t)a[1], qp, why, sizeof why);
            break;
        case 1:
            st = mdb_ivf_check_files(files[0].p, files[0].len, (size_t)a[0], files[1].p, files[1].len, (size_t)a[1], qp, (uint32_t)a[10],
                                     (uint32_t)a[11], why, sizeof why);
            break;
        case 2:
            st = mdb_spann_check_files(files[2].p, files[2].len, 0, files[3].p, files[3].len, 0, files[4].p, files[4].len, 0, files[5].p,
                                       files[5].len, 0, qp, why, sizeof why);
            break;
        case 3: {
            // the records in an array of exactly n_users elements, like the files
            const size_t n = files[6].len / sizeof(mdb_user_index_info);
            std::vector<mdb_user_index_info> users(n);
            if (n) memcpy(users.data(), files[6].p, n * sizeof(mdb_user_index_info));
            st = mdb_multi_spann_check_files(n ? users.data() : nullptr, n, (uint32_t)a[9], files[2].p, files[2].len, files[3].p, files[3].len,
                                             files[4].p, files[4].len, files[5].p, files[5].len, qp, (uint32_t)a[10], (uint32_t)a[11], why,
                                             sizeof why);
            break;
        }
        default:
            r.ok = false;
        }
        // a refusal carries a message, an acceptance the empty string: both NUL-terminated inside the buffer
        if (!memchr(why, 0, sizeof why) || (st == MDB_OK) != (why[0] == 0)) {
            fprintf(stderr, "%s: status %d with message '%.*s'\n", name.c_str(), (int)st, (int)sizeof why, why);
            return 3;
        }
        printf("%s %d\n", name.c_str(), (int)st);
    }
    fclose(r.f);
    if (!r.ok) { fprintf(stderr, "malformed bundle\n"); return 2; }
    return 0;
}
