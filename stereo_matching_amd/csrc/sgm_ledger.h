// sgm_ledger.h -- the handle's device memory: every live allocation with its size, their sum
// (sgm_device_bytes), and the rollback of a group of allocations that did not all succeed.  Host-pure:
// two function pointers allocate and release (sgm_handle.h: hipMalloc, hipFree; tests/cpp/ledger_main.cpp: malloc).
#pragma once

#include <assert.h>
#include <stddef.h>
#include <vector>

namespace sgm {

struct __attribute__((visibility("hidden"))) Ledger {  // (kept out of the library's exported symbols)
    typedef int (*Get)(void **p, size_t bytes);  // 0, or the allocator's error code
    typedef void (*Put)(void *p);
    struct Entry { void *p; size_t bytes; };
    struct Group;

    Get get;
    Put put;
    std::vector<Entry> live;
    size_t sum = 0;         // of live's bytes
    Group *open = nullptr;  // the group allocations join

    // *slot: `bytes` of new memory, or null (nothing asked for, or the allocator failed: its code)
    int alloc(void **slot, size_t bytes);
    // Releases *slot, whose size the ledger knows, and nulls it (null, or not the ledger's: nulled only).
    void free(void **slot) {
        for (size_t k = 0; k < live.size(); ++k)
            if (live[k].p == *slot) {
                put(*slot);
                sum -= live[k].bytes;
                live.erase(live.begin() + k);
                break;
            }
        *slot = nullptr;
    }
    void free_all() {
        for (const Entry &e : live) put(e.p);
        live.clear();
        sum = 0;
    }
};

// All or nothing: unless commit() is reached, the scope's end frees every allocation made since the
// group opened, by whomever, and nulls its pointer (which has to outlive the group).  What was
// allocated before, or freed inside, is not touched.  Groups do not nest (asserted).
struct Ledger::Group {
    Ledger &l;
    std::vector<void **> slots;
    explicit Group(Ledger &ledger) : l(ledger) { assert(!l.open), l.open = this; }
    void commit() {  // (closes the group: later allocations join none)
        slots.clear();
        l.open = nullptr;
    }
    ~Group() {
        for (void **s : slots) l.free(s);
        commit();
    }
};

inline int Ledger::alloc(void **slot, size_t bytes) {
    *slot = nullptr;
    if (bytes == 0) return 0;
    if (int rc = get(slot, bytes)) return *slot = nullptr, rc;
    live.push_back({*slot, bytes});
    sum += bytes;
    if (open) open->slots.push_back(slot);
    return 0;
}

}  // namespace sgm
