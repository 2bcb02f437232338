// hip_owner_check.cpp -- xfr_amd/csrc/hip_owner.h against the stand-in runtime of hip/hip_runtime.h: ownership, grow, failed creations, the
// all-or-nothing group idiom and the status mapping; and xfr_amd/csrc/scoped.h, the guard: a scope's value goes back on every way out.  All on the host
// compiler alone (tests/test_hip_owner.py builds and runs it under the sanitizers).
// Exit status 0: every case holds; otherwise the failing case is printed.
#include "../../xfr_amd/csrc/hip_owner.h"
#include "../../xfr_amd/csrc/scoped.h"

#include <cstdio>
#include <type_traits>
#include <utility>

using namespace xfr;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __func__, __LINE__, #cond); return 1; } \
    } while (0)

static bool none_live() { return !fake::live[fake::DEVICE] && !fake::live[fake::PINNED] && !fake::live[fake::EVENT] && !fake::live[fake::STREAM]; }
static int total_live() { return fake::live[fake::DEVICE] + fake::live[fake::PINNED] + fake::live[fake::EVENT] + fake::live[fake::STREAM]; }

static int basic_ownership()
{
    {
        DevBuf<float> d;
        PinnedBuf<int> h;
        Event ev, timed;
        Stream s, low;
        CHECK(!d && !h && !ev && !s && d.cap == 0);
        CHECK(d.alloc(7) == XFR_OK && h.alloc(5) == XFR_OK && ev.create() == XFR_OK && timed.create(true) == XFR_OK);
        CHECK(s.create() == XFR_OK && low.create(-1) == XFR_OK);
        CHECK(d.cap == 7 && h.cap == 5 && fake::live[fake::DEVICE] == 1 && fake::live[fake::PINNED] == 1);
        CHECK(fake::live[fake::EVENT] == 2 && fake::live[fake::STREAM] == 2);
        float* raw = d;                                   // the implicit conversions: handles, arithmetic
        hipEvent_t raw_ev = ev;
        hipStream_t raw_s = s;
        CHECK(raw && d + 3 == raw + 3 && raw_ev && raw_s);
        DevBuf<float> d2(std::move(d));                   // move construction and assignment empty their source
        CHECK(!d && d.cap == 0 && d2 == raw && d2.cap == 7 && fake::live[fake::DEVICE] == 1);
        DevBuf<float> d3;
        CHECK(d3.alloc(2) == XFR_OK && fake::live[fake::DEVICE] == 2);
        d3 = std::move(d2);                               // ... and assignment releases what the target held
        CHECK(d3 == raw && d3.cap == 7 && !d2 && fake::live[fake::DEVICE] == 1);
        PinnedBuf<int> h2;
        h2 = std::move(h);
        Event ev2(std::move(ev));
        Stream s2;
        s2 = std::move(s);
        CHECK(!h && !ev && !s && h2.cap == 5 && ev2 == raw_ev && s2 == raw_s && total_live() == 6);
        d3.reset(); h2.reset(); ev2.reset(); s2.reset();
        CHECK(!d3 && d3.cap == 0 && !h2 && h2.cap == 0 && !ev2 && !s2 && total_live() == 2);
        d3.reset();                                       // (an empty owner's reset is nothing)
        CHECK(total_live() == 2);
    }                                                     // `timed` and `low` go with the scope
    CHECK(none_live());
    return 0;
}

static int grow_keeps_and_grows()
{
    DevBuf<double> d;
    CHECK(d.grow(10) == XFR_OK && d.cap == 10);
    double* first = d;
    fake::calls.clear();
    CHECK(d.grow(10) == XFR_OK && d.grow(3) == XFR_OK);   // large enough: the same pointer, no call
    CHECK(d == first && d.cap == 10 && fake::calls.empty());
    CHECK(d.grow(11) == XFR_OK && d.cap == 11 && fake::live[fake::DEVICE] == 1);
    CHECK(fake::calls == "Yfm");                          // synchronise, free, allocate
    d.reset();
    CHECK(none_live());
    return 0;
}

static int failed_grow()
{
    DevBuf<int> d;
    CHECK(d.grow(4) == XFR_OK);
    fake::fail_in = 1;
    CHECK(d.grow(8) == XFR_OOM && !d && d.cap == 0 && none_live());
    CHECK(g_err.find("hipMalloc") != std::string::npos);
    CHECK(d.grow(8) == XFR_OK && d && d.cap == 8 && fake::live[fake::DEVICE] == 1);
    return 0;
}

// five mixed resources that one test stands for, built as the engine's groups are: into locals, moved into the members once all exist
struct Group {
    Stream s;
    Event ev;
    DevBuf<float> a;
    DevBuf<int> b;
    PinnedBuf<int> h;
};

static xfr_status ensure_group(Group& g)
{
    if (g.a) return XFR_OK;
    DevBuf<float> a;
    DevBuf<int> b;
    PinnedBuf<int> h;
    Event ev;
    Stream s;
    XFR_TRY(a.alloc(16));
    XFR_TRY(b.alloc(16));
    XFR_TRY(h.alloc(16));
    XFR_TRY(ev.create());
    XFR_TRY(s.create());
    g.a = std::move(a); g.b = std::move(b); g.h = std::move(h); g.ev = std::move(ev); g.s = std::move(s);
    return XFR_OK;
}

static int groups()
{
    for (int k = 1; k <= 5; ++k) {
        Group g;
        fake::fail_in = k;
        CHECK(ensure_group(g) == XFR_OOM);
        CHECK(fake::fail_in == 0);                        // (the switch fired)
        CHECK(!g.a && !g.b && !g.h && !g.ev && !g.s && none_live());
        CHECK(ensure_group(g) == XFR_OK);                 // the retry
        CHECK(g.a && g.b && g.h && g.ev && g.s && total_live() == 5);
        CHECK(fake::live[fake::DEVICE] == 2 && fake::live[fake::PINNED] == 1 && fake::live[fake::EVENT] == 1 && fake::live[fake::STREAM] == 1);
        fake::calls.clear();
        CHECK(ensure_group(g) == XFR_OK && fake::calls.empty());      // complete: nothing is created again
    }
    CHECK(none_live());
    return 0;
}

static xfr_status tried(hipError_t e)
{
    HIP_TRY(e);
    return XFR_OK;
}

static int status_mapping()
{
    CHECK(tried(hipSuccess) == XFR_OK);
    CHECK(tried(hipErrorOutOfMemory) == XFR_OOM && g_err.find("out of memory") != std::string::npos);
    CHECK(tried(hipErrorUnknown) == XFR_HIP_ERROR && tried(1) == XFR_HIP_ERROR);
    fake::fail_with = hipErrorUnknown;                    // a creation that fails for another reason
    fake::fail_in = 1;
    Event ev;
    CHECK(ev.create() == XFR_HIP_ERROR && !ev && none_live());
    fake::fail_with = hipErrorOutOfMemory;
    fake::fail_in = 1;
    PinnedBuf<char> h;
    CHECK(h.alloc(1) == XFR_OOM && !h && h.cap == 0 && none_live());
    return 0;
}

static_assert(!std::is_copy_constructible<Scoped<int>>::value && !std::is_copy_assignable<Scoped<int>>::value, "a guard is not copied");
static_assert(!std::is_copy_constructible<Scoped<const float*>>::value && !std::is_copy_assignable<Scoped<const float*>>::value, "a guard is not copied");

// leaves through the early return when `early`, through the end otherwise; `seen` is what the callee read
static xfr_status scoped_callee(int& slot, bool early, int& seen)
{
    Scoped<int> g(slot, 7);
    seen = slot;
    if (early) return fail(XFR_INVALID_ARG, "an early way out");
    XFR_TRY(tried(hipSuccess));
    return XFR_OK;
}

static int scoped_values()
{
    int slot = 3;                                         // the previous value comes back, not a constant
    {
        Scoped<int> g(slot, 5);
        CHECK(slot == 5);
    }
    CHECK(slot == 3);
    int seen = -1;                                        // an early return restores it, like the end of the function
    CHECK(scoped_callee(slot, true, seen) == XFR_INVALID_ARG && seen == 7 && slot == 3);
    slot = 4;
    CHECK(scoped_callee(slot, false, seen) == XFR_OK && seen == 7 && slot == 4);
    {                                                     // two guards on one variable go in reverse order
        Scoped<int> outer(slot, 1);
        {
            Scoped<int> inner(slot, 2);
            CHECK(slot == 2);
        }
        CHECK(slot == 1);
        Scoped<int> again(slot, 9);                       // (same scope: `again` goes first, then `outer`)
        CHECK(slot == 9);
    }
    CHECK(slot == 4);
    const float a[2] = {1.f, 2.f};                        // a pointer, to null and back; a bool
    const float* bank = a;
    bool on = false;
    {
        Scoped<const float*> g(bank, nullptr);
        Scoped<bool> h(on, true);
        CHECK(bank == nullptr && on);
        {
            Scoped<const float*> k(bank, a + 1);
            CHECK(bank == a + 1);
        }
        CHECK(bank == nullptr);
    }
    CHECK(bank == a && !on);
    DevBuf<float> d;                                      // what the engine does: an owner converts to the pointer the guard writes
    CHECK(d.alloc(4) == XFR_OK);
    float* cur = nullptr;
    {
        Scoped<float*> g(cur, d);
        CHECK(cur == d.p);
    }
    CHECK(cur == nullptr && d.cap == 4);
    d.reset();
    CHECK(none_live());
    return 0;
}

int main()
{
    if (basic_ownership() || grow_keeps_and_grows() || failed_grow() || groups() || status_mapping() || scoped_values()) return 1;
    printf("hip_owner_check: all cases hold\n");
    return 0;
}
