// scratch_arena_check.cpp — stand-alone check of mdb_arena (muopdb_amd/csrc/mdb_arena.h) with malloc / free as the injected
// allocator.  Built and run by tests/test_scratch_arena.py under AddressSanitizer + UBSan; exit status 0 = every property held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../muopdb_amd/csrc/mdb_arena.h"

static long g_allocs = 0, g_frees = 0;
static int counting_malloc(void*, size_t bytes, void** out) {
    ++g_allocs;
    *out = malloc(bytes);
    return *out ? 0 : 1;
}
static void counting_free(void*, void* p) {
    ++g_frees;
    free(p);
}

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

// one simulated API call: begin, the requests, every buffer filled with its own byte, all verified at the end
// (disjoint, and pointers handed out before a new chunk was added are still good)
static std::vector<void*> run_call(mdb_arena& a, const std::vector<size_t>& req) {
    CHECK(a.begin());
    std::vector<void*> ptrs;
    for (size_t i = 0; i < req.size(); ++i) {
        void* p = a.alloc(req[i]);
        CHECK(p != nullptr);
        CHECK(((uintptr_t)p & 255) == 0);
        memset(p, (int)(i + 1), req[i]);
        ptrs.push_back(p);
    }
    for (size_t i = 0; i < req.size(); ++i) {
        const unsigned char* p = (const unsigned char*)ptrs[i];
        if (req[i]) CHECK(p[0] == (unsigned char)(i + 1) && memcmp(p, p + 1, req[i] - 1) == 0);   // every byte is the buffer's own
        for (size_t j = 0; j < i; ++j) CHECK(ptrs[i] != ptrs[j]);   // zero-length requests are distinct too
    }
    return ptrs;
}

int main() {
    {
        mdb_arena a;
        a.alloc_cb = counting_malloc;
        a.release_cb = counting_free;
        std::mt19937_64 rng(12345);
        auto random_call = [&](size_t max_bytes) {
            std::vector<size_t> req(1 + rng() % 20);
            for (size_t& r : req) {
                const unsigned kind = (unsigned)(rng() % 8);
                r = kind == 0 ? 0 : kind == 1 ? 1 + rng() % 255 : kind < 6 ? rng() % 65536 : rng() % (max_bytes + 1);
            }
            return req;
        };
        // ---- random calls: alignment, disjointness, survival across growth (sizes up to 8 MB force extra chunks)
        for (int call = 0; call < 220; ++call) run_call(a, random_call(call % 3 == 0 ? (8u << 20) : (256u << 10)));

        // ---- an identical call repeated: from the third repetition on no allocator call, the same addresses
        std::vector<size_t> big = {0, 100, 3u << 20, 7, 8u << 20, 65536, 1u << 20, 0, 4097};
        run_call(a, big);
        run_call(a, big);
        std::vector<void*> ref = run_call(a, big);
        for (int rep = 0; rep < 5; ++rep) {
            const long n0 = g_allocs, f0 = g_frees;
            CHECK(run_call(a, big) == ref);
            CHECK(g_allocs == n0 && g_frees == f0);
        }
        // ---- a smaller call after a larger one: no allocator call
        {
            const long n0 = g_allocs, f0 = g_frees;
            run_call(a, {5, 1u << 20, 0, 300});
            run_call(a, {2u << 20});
            CHECK(g_allocs == n0 && g_frees == f0);
        }
        // ---- a larger call grows, and is steady again within two repetitions
        {
            std::vector<size_t> bigger = big;
            bigger.push_back(6u << 20);
            bigger.push_back(a.capacity());   // more than the arena holds
            const long n0 = g_allocs;
            run_call(a, bigger);
            CHECK(g_allocs > n0);
            run_call(a, bigger);
            const long n1 = g_allocs, f1 = g_frees;
            std::vector<void*> r1 = run_call(a, bigger);
            CHECK(run_call(a, bigger) == r1);
            CHECK(g_allocs == n1 && g_frees == f1);
        }
        // ---- mark / rewind in a loop inside one call: the capacity of one iteration, the buffers of before the loop intact
        {
            mdb_arena b;
            b.alloc_cb = counting_malloc;
            b.release_cb = counting_free;
            const size_t X = 3u << 20;
            CHECK(b.begin());   // the capacity one iteration needs, measured on an arena of its own
            CHECK(b.alloc(1000) && b.alloc(X) && b.alloc(X / 2));
            const size_t one = b.capacity();
            CHECK(one >= 1000 + X + X / 2);
            mdb_arena c;
            c.alloc_cb = counting_malloc;
            c.release_cb = counting_free;
            CHECK(c.begin());
            unsigned char* keep = (unsigned char*)c.alloc(1000);
            CHECK(keep);
            memset(keep, 0xAB, 1000);
            void *first_x = nullptr, *first_y = nullptr;
            long allocs_after_first = 0;
            for (int i = 0; i < 1000; ++i) {
                const mdb_arena::Mark m = c.mark();
                void* x = c.alloc(X);
                void* y = c.alloc(X / 2);
                CHECK(x && y && ((uintptr_t)x & 255) == 0 && ((uintptr_t)y & 255) == 0);
                memset(x, i & 0x7F, X);
                memset(y, 0x80 | (i & 0x7F), X / 2);
                if (i == 0) { first_x = x; first_y = y; allocs_after_first = g_allocs; }
                CHECK(x == first_x && y == first_y);
                c.rewind(m);
            }
            CHECK(g_allocs == allocs_after_first);
            for (int j = 0; j < 1000; ++j) CHECK(keep[j] == 0xAB);
            CHECK(c.capacity() == one);
            // the next call consolidates to one chunk of the iteration's high-water mark + 25 % and loops without growing
            CHECK(c.begin());
            const size_t cap = c.capacity();
            CHECK(c.alloc(1000));
            for (int i = 0; i < 1000; ++i) {
                const mdb_arena::Mark m = c.mark();
                CHECK(c.alloc(X) && c.alloc(X / 2));
                c.rewind(m);
            }
            CHECK(c.capacity() == cap);
        }
        // ---- an allocator that refuses: nullptr and the refused size, nothing handed out
        {
            mdb_arena d;
            d.alloc_cb = [](void*, size_t, void** out) { *out = nullptr; return 2; };
            d.release_cb = counting_free;
            CHECK(d.begin());
            CHECK(d.alloc(4096) == nullptr);
            CHECK(d.fail_code == 2 && d.fail_bytes >= 4096);
        }
    }   // destructors: every chunk goes back (LeakSanitizer checks at exit; the counters here)
    CHECK(g_allocs == g_frees);
    printf("scratch arena ok: %ld allocator calls\n", g_allocs);
    return 0;
}
