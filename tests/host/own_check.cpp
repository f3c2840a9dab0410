// own_check.cpp -- the handle core of csrc/uva_own.h as a program of its own: no HIP header, a policy that counts instead of
// freeing.  tests/test_own_sanitized.py compiles it with the host compiler under AddressSanitizer and
// UndefinedBehaviorSanitizer and runs it as a child process.  Prints "own_check: <n> checks: ok", or the first failure.
#define UVA_OWN_CORE_ONLY
#include "../../upscale_video_amd/csrc/uva_own.h"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

namespace {

// a resource is an int on the heap (so that the sanitizer sees a double free or a leak as well); destroy() logs its value
struct Counting {
    static std::atomic<long long>& live() { static std::atomic<long long> n{0}; return n; }
    static std::vector<int>& log() { static std::vector<int> v; return v; }
    static bool& alloc_fails() { static bool f = false; return f; }
    static long long& allocs() { static long long n = 0; return n; }
    static void destroy(int* p) { log().push_back(*p); delete p; }
    static int alloc(void** p, size_t bytes)
    {
        if (alloc_fails()) return 2;
        ++allocs();
        *p = new int((int)bytes);
        return 0;
    }
};
using H = uva::Owned<int*, Counting>;
using B = uva::Buf<int*, Counting>;

int g_checks = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            std::printf("own_check: line %d: %s\n", __LINE__, #cond);          \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

long long live() { return Counting::live().load(); }
size_t freed(int v)
{
    size_t n = 0;
    for (int x : Counting::log()) n += x == v;
    return n;
}

struct Three {                   // members are destroyed in reverse order of declaration
    H a, b, c;
};

}  // namespace

int main()
{
    CHECK(live() == 0);
    {   // construction, get, bool, reset
        H h;
        CHECK(!h && h.get() == nullptr && live() == 0);
        h.reset(new int(1));
        CHECK(h && *h.get() == 1 && live() == 1);
        int* view = h;           // a handle converts to a view of what it holds
        CHECK(view == h.get());
        h.reset(new int(2));     // reset with a new resource frees the old one
        CHECK(freed(1) == 1 && live() == 1 && *h.get() == 2);
        h.reset();
        CHECK(freed(2) == 1 && !h && live() == 0);
        h.reset();               // (an empty handle: nothing to free)
        CHECK(Counting::log().size() == 2);
    }
    {   // move construction: the resource changes hands and is freed once
        H a(new int(3));
        H b(std::move(a));
        CHECK(!a && b && *b.get() == 3 && live() == 1 && freed(3) == 0);
    }
    CHECK(freed(3) == 1 && live() == 0);
    {   // move assignment frees what the target held, exactly once
        H a(new int(4)), b(new int(5));
        CHECK(live() == 2);
        b = std::move(a);
        CHECK(freed(5) == 1 && freed(4) == 0 && !a && *b.get() == 4 && live() == 1);
        H& self = b;
        b = std::move(self);     // self-move: nothing is freed, nothing is lost
        CHECK(b && *b.get() == 4 && freed(4) == 0 && live() == 1);
    }
    CHECK(freed(4) == 1 && freed(5) == 1 && live() == 0);
    {   // a vector of handles survives reallocation
        std::vector<H> v;
        for (int i = 0; i < 100; ++i) v.emplace_back(new int(100 + i));
        CHECK(live() == 100);
        for (int i = 0; i < 100; ++i) CHECK(*v[i].get() == 100 + i && freed(100 + i) == 0);
        v.erase(v.begin() + 10);
        CHECK(freed(110) == 1 && live() == 99);
    }
    for (int i = 0; i < 100; ++i) CHECK(freed(100 + i) == 1);
    CHECK(live() == 0);
    {   // a struct's members go in reverse order of declaration
        const size_t at = Counting::log().size();
        {
            Three t;
            t.a.reset(new int(201)); t.b.reset(new int(202)); t.c.reset(new int(203));
        }
        const std::vector<int>& log = Counting::log();
        CHECK(log.size() == at + 3 && log[at] == 203 && log[at + 1] == 202 && log[at + 2] == 201);
        // ... and a struct assigned from a fresh one releases them in the order of declaration
        Three t;
        t.a.reset(new int(211)); t.b.reset(new int(212)); t.c.reset(new int(213));
        t = Three();
        CHECK(log.size() == at + 6 && log[at + 3] == 211 && log[at + 4] == 212 && log[at + 5] == 213 && live() == 0);
    }
    {   // the growing buffer
        B b;
        CHECK(!b && b.cap() == 0 && b.get() == nullptr);
        CHECK(b.grow(1064) == 0 && b && b.cap() == 1064 && *b.get() == 1064 && live() == 1);
        int* const before = b.get();
        const long long allocs = Counting::allocs();
        CHECK(b.grow(1064) == 0 && b.grow(1010) == 0);          // no-op grows: the same buffer, the same capacity
        CHECK(b.get() == before && b.cap() == 1064 && Counting::allocs() == allocs && freed(1064) == 0);
        CHECK(b.grow(1128) == 0 && b.cap() == 1128 && *b.get() == 1128 && freed(1064) == 1 && live() == 1);
        Counting::alloc_fails() = true;                     // a failed grow: the error handed on, the buffer empty
        CHECK(b.grow(1256) == 2 && !b && b.cap() == 0 && b.get() == nullptr && freed(1128) == 1 && live() == 0);
        CHECK(b.grow(0) == 0 && b.grow(1100) == 2 && b.cap() == 0 && !b);
        Counting::alloc_fails() = false;
        CHECK(b.grow(1032) == 0 && b.cap() == 1032 && live() == 1);
        B c(std::move(b));                                  // buffers move as handles do, and leave capacity 0 behind
        CHECK(c.cap() == 1032 && *c.get() == 1032 && !b && b.cap() == 0 && live() == 1);
        b = std::move(c);
        CHECK(b.cap() == 1032 && *b.get() == 1032 && !c && c.cap() == 0 && live() == 1 && freed(1032) == 0);
    }
    CHECK(freed(1032) == 1);
    CHECK(live() == 0);
    std::printf("own_check: %d checks: ok\n", g_checks);
    return 0;
}
