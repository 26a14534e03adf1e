// The handle's memory ledger (stereo_matching_amd/csrc/sgm_ledger.h) on the CPU,
// for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all ledger_main.cpp
// It drives the ledger with malloc / free, and with an allocator that fails on
// its k-th call, through the paths no GPU test can reach: a group of
// allocations that fails at every position.  ASan is what proves that no path
// leaks or frees twice.  Prints "ok <checks>" and exits 0, or the line of the
// first check that failed and exits 1.  With an argument it nests two groups
// instead, which must abort on the constructor's assert.  tests/test_ledger_cpu.py runs it.
#include "../../stereo_matching_amd/csrc/sgm_ledger.h"

#include <stdio.h>
#include <stdlib.h>

using sgm::Ledger;

static int checks = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            printf("line %d: %s\n", __LINE__, #cond);                 \
            return 1;                                                 \
        }                                                             \
    } while (0)

static int calls = 0, fail_at = 0;  // the allocator fails on call number fail_at (0: never)
static int get(void **p, size_t bytes) {
    if (++calls == fail_at) return 2;  // (any code but 0; *p is left as it was)
    *p = malloc(bytes);
    return *p ? 0 : 2;
}
static void put(void *p) { free(p); }

// the sum is the live entries' bytes
static bool consistent(const Ledger &l) {
    size_t n = 0;
    for (const Ledger::Entry &e : l.live) n += e.bytes;
    return n == l.sum;
}

static int run() {
    Ledger l{get, put};
    char *a = (char *)&l, *b = nullptr;  // (a: not null before the call)
    CHECK(l.alloc((void **)&a, 0) == 0 && a == nullptr && l.live.empty() && l.sum == 0);
    l.free((void **)&a);  // a null pointer: nothing
    CHECK(l.live.empty() && l.sum == 0);

    // two buffers of different sizes: each free subtracts its own, no size passed in
    CHECK(l.alloc((void **)&a, 100) == 0 && a && l.sum == 100 && consistent(l));
    CHECK(l.alloc((void **)&b, 7) == 0 && b && l.sum == 107 && l.live.size() == 2 && consistent(l));
    a[99] = b[6] = 1;
    l.free((void **)&a);
    CHECK(a == nullptr && l.sum == 7 && l.live.size() == 1 && l.live[0].p == b && consistent(l));
    l.free((void **)&a);  // twice: nothing
    CHECK(l.sum == 7 && consistent(l));
    char mine = 0, *stray = &mine;  // a pointer the ledger does not hold: nulled, nothing released or subtracted
    l.free((void **)&stray);
    CHECK(stray == nullptr && l.sum == 7 && l.live.size() == 1 && consistent(l));

    // a group of three, the allocator failing at each position: all three null, the sum as
    // before the group, the buffer from before it still live and counted
    for (int k = 1; k <= 3; ++k) {
        char *g[3] = {nullptr, nullptr, nullptr};
        int rc = 0;
        {
            Ledger::Group group(l);
            calls = 0;
            fail_at = k;
            for (int i = 0; i < 3 && !rc; ++i) {
                rc = l.alloc((void **)&g[i], 10 * (i + 1));
                CHECK(consistent(l) && (rc != 0) == (i + 1 == k) && (g[i] != nullptr) == !rc);
            }
            fail_at = 0;
            CHECK(rc == 2 && l.live.size() == (size_t)k);  // (b and the k - 1 that succeeded)
            if (!rc) group.commit();
        }
        CHECK(!g[0] && !g[1] && !g[2]);
        CHECK(l.sum == 7 && l.live.size() == 1 && l.live[0].p == b && consistent(l) && l.open == nullptr);
        b[6] = (char)k;  // (still ours: ASan would object)
    }

    // what a group frees itself stays freed, and what was allocated before it is not rolled back
    {
        char *c = nullptr;
        Ledger::Group group(l);
        CHECK(l.alloc((void **)&c, 33) == 0 && l.sum == 40);
        l.free((void **)&b);
        l.free((void **)&c);
        CHECK(l.sum == 0 && l.live.empty());
        CHECK(l.alloc((void **)&b, 7) == 0 && l.sum == 7);
        group.commit();
    }
    CHECK(b && l.sum == 7 && l.live.size() == 1 && consistent(l));

    // a committed group survives its scope
    char *g[3] = {nullptr, nullptr, nullptr};
    {
        Ledger::Group group(l);
        for (int i = 0; i < 3; ++i) CHECK(l.alloc((void **)&g[i], 10 * (i + 1)) == 0);
        group.commit();
        CHECK(l.open == nullptr && l.alloc((void **)&a, 3) == 0);  // after the commit, in its scope: joins no group
    }
    CHECK(a && l.sum == 70);
    l.free((void **)&a);
    CHECK(g[0] && g[1] && g[2] && l.sum == 67 && l.live.size() == 4 && consistent(l));
    g[0][9] = g[1][19] = g[2][29] = 1;
    l.free((void **)&g[1]);  // from the middle
    CHECK(!g[1] && l.sum == 47 && l.live.size() == 3 && consistent(l));
    // an allocation outside any group joins none: a later group's rollback leaves it
    CHECK(l.alloc((void **)&a, 5) == 0 && l.sum == 52);
    { Ledger::Group group(l); }
    CHECK(a && l.sum == 52 && consistent(l));

    l.free_all();
    CHECK(l.sum == 0 && l.live.empty());
    return 0;
}

int main(int argc, char **) {
    if (argc > 1) {  // any argument: a group inside a group, which the constructor's assert refuses (abort)
        Ledger l{get, put};
        Ledger::Group outer(l), inner(l);
        return 0;
    }
    if (run()) return 1;
    printf("ok %d\n", checks);
    return 0;
}
