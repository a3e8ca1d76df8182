// dev_table.h -- how the table of a table-driven launch (its boxes, then the prefix array over them) reaches the device.
// Host code only; DESIGN.md "Device tables".
//   StagedTable  one buffer of the context that every call overwrites: two asynchronous copies on the caller's stream.
//   TableCache   a device copy per table content: a table the context has seen costs no copy, no allocation and no
//                synchronisation, so the call can be captured into a graph.
// Both lay the table out alike: the first part at the start of the buffer, the second at the next multiple of 256 bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "../../include/castro_hydro_amd.h"

namespace cad {

inline size_t table_part2(size_t bytes1) { return (bytes1 + 255) & ~(size_t)255; }

// The one rule callers rely on: successive users of one StagedTable are ordered on ONE stream.  The copies of a call queue
// behind the kernels of the call before, which read the previous table; the source is pageable memory, which the runtime has
// staged when hipMemcpyAsync returns, so the caller's host vectors may go out of scope.  A launch family that can have two tables
// in flight (the sources with diffusion) has two StagedTables.
struct StagedTable {
    void* p = nullptr;
    size_t bytes = 0;

    // a[0, na) and b[0, nb) to the device; da / db: where the kernels read them.  Grows when the two parts need more than the
    // buffer holds: synchronises `stream`, frees, allocates twice the need.  0, CASTRO_AMD_ERR_NOMEM or CASTRO_AMD_ERR_HIP
    template <class A, class B>
    int stage(const A* a, size_t na, const B* b, size_t nb, hipStream_t stream, const A*& da, const B*& db)
    {
        const size_t ba = na * sizeof(A), bb = nb * sizeof(B), off = table_part2(ba), need = off + bb;
        if (need > bytes) {
            release(stream);
            if (hipMalloc(&p, 2 * need) != hipSuccess) { p = nullptr; return CASTRO_AMD_ERR_NOMEM; }
            bytes = 2 * need;
        }
        da = (const A*)p;
        db = (const B*)((const char*)p + off);
        if (hipMemcpyAsync(p, a, ba, hipMemcpyHostToDevice, stream) != hipSuccess) return CASTRO_AMD_ERR_HIP;
        if (hipMemcpyAsync((char*)p + off, b, bb, hipMemcpyHostToDevice, stream) != hipSuccess) return CASTRO_AMD_ERR_HIP;
        return 0;
    }

    void release(hipStream_t stream = nullptr)
    {
        if (p) { (void)hipStreamSynchronize(stream); (void)hipFree(p); }
        p = nullptr; bytes = 0;
    }
};

// Lookup by content (every byte of the parts: fill a table field by field over zeroed storage).  A miss evicts the oldest
// table once `cap` are kept -- after a synchronisation of `stream`, whose kernels may still read it -- and copies with a blocking
// hipMemcpy: an asynchronous copy from the caller's host vector could not be captured.
struct TableCache {
    struct Entry { std::vector<char> host; void* dev = nullptr; };
    size_t cap;
    std::vector<Entry> entries;

    explicit TableCache(size_t cap_) : cap(cap_) {}

    template <class A, class B>
    int find(const A* a, size_t na, const B* b, size_t nb, hipStream_t stream, const A*& da, const B*& db)
    {
        const size_t ba = na * sizeof(A), bb = nb * sizeof(B), off = bb ? table_part2(ba) : ba;
        std::vector<char> key(off + bb, 0);
        std::memcpy(key.data(), a, ba);
        if (bb) std::memcpy(key.data() + off, b, bb);
        const Entry* hit = nullptr;
        for (const Entry& e : entries) if (e.host == key) { hit = &e; break; }
        if (!hit) {
            if (entries.size() >= cap) {
                (void)hipStreamSynchronize(stream);
                (void)hipFree(entries.front().dev);
                entries.erase(entries.begin());
            }
            void* d = nullptr;
            if (hipMalloc(&d, key.size()) != hipSuccess) return CASTRO_AMD_ERR_NOMEM;
            if (hipMemcpy(d, key.data(), key.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return CASTRO_AMD_ERR_HIP; }
            entries.push_back(Entry());
            entries.back().host.swap(key);
            entries.back().dev = d;
            hit = &entries.back();
        }
        da = (const A*)hit->dev;
        db = (const B*)((const char*)hit->dev + off);
        return 0;
    }

    // a table of one part
    template <class A>
    int find(const A* a, size_t na, hipStream_t stream, const A*& da)
    {
        const char* none = nullptr;
        return find(a, na, none, 0, stream, da, none);
    }

    void release()
    {
        for (Entry& e : entries) (void)hipFree(e.dev);
        entries.clear();
    }
};

} // namespace cad
