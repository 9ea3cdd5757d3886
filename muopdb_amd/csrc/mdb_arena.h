// mdb_arena.h — bump arena for the temporary buffers of ONE API call (plain C++17; the backing allocator is injected).
//   begin()        starts a call: everything handed out before it is dead.  A previous call that spilled into more than one
//                  chunk is consolidated into ONE chunk of its high-water mark + 25 %; otherwise only the offset is reset.
//   alloc(bytes)   non-null, 256-byte aligned, valid until the next begin(), disjoint from the call's other allocations.
//                  A full chunk is followed by a new one: no chunk is freed or moved during a call.  nullptr: the allocator
//                  refused (fail_bytes / fail_code say what).
//   mark / rewind  for loops inside one call: rewind gives back everything allocated since the mark.
// A repeated call with the same or smaller requests makes no allocator call and gets the same addresses.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct mdb_arena {
    static constexpr size_t ALIGN = 256;
    using alloc_fn = int (*)(void* user, size_t bytes, void** out);  // 0, or the allocator's own error code
    using release_fn = void (*)(void* user, void* p);
    struct Mark { size_t chunk, off, used; };

    alloc_fn alloc_cb = nullptr;
    release_fn release_cb = nullptr;
    void* user = nullptr;
    size_t fail_bytes = 0;
    int fail_code = 0;

    mdb_arena() = default;
    mdb_arena(const mdb_arena&) = delete;
    mdb_arena& operator=(const mdb_arena&) = delete;
    ~mdb_arena() { release_all(); }

    bool begin() {
        if (chunks.size() > 1) {
            const size_t want = peak + peak / 4;
            release_all();
            if (!add_chunk(want)) return false;
        }
        cur = off = used = peak = 0;
        return true;
    }
    void* alloc(size_t bytes) {
        const size_t need = ((bytes ? bytes : 16) + ALIGN - 1) & ~(ALIGN - 1);
        while (cur < chunks.size() && off + need > chunks[cur].cap) { ++cur; off = 0; }
        if (cur == chunks.size() && !add_chunk(need + need / 4)) return nullptr;
        char* p = chunks[cur].base + off;
        off += need;
        used += need;
        if (used > peak) peak = used;
        return p;
    }
    Mark mark() const { return Mark{cur, off, used}; }
    void rewind(const Mark& m) { cur = m.chunk; off = m.off; used = m.used; }
    size_t capacity() const {
        size_t c = 0;
        for (const Chunk& k : chunks) c += k.cap;
        return c;
    }
    void release_all() {
        for (const Chunk& k : chunks) release_cb(user, k.raw);
        chunks.clear();
        cur = off = used = 0;
    }

private:
    struct Chunk { void* raw; char* base; size_t cap; };
    std::vector<Chunk> chunks;
    size_t cur = 0, off = 0;      // bump position: chunk index and byte offset in it
    size_t used = 0, peak = 0;    // bytes live now / the call's high-water mark

    bool add_chunk(size_t cap) {
        cap = (cap + ALIGN - 1) & ~(ALIGN - 1);
        void* raw = nullptr;
        const int e = alloc_cb(user, cap + ALIGN, &raw);   // + ALIGN: the base is aligned here, whatever the allocator returns
        if (e != 0 || !raw) { fail_bytes = cap + ALIGN; fail_code = e; return false; }
        char* base = (char*)(((uintptr_t)raw + ALIGN - 1) & ~(uintptr_t)(ALIGN - 1));
        chunks.push_back(Chunk{raw, base, cap});
        return true;
    }
};
