// frames_host_check.cpp -- drives csrc/ntsc_frames.hpp (the host logic every device stage shares) without a GPU: plain C++
// with its own main, compiled and run by tests/test_frames_host.py.  Frame "addresses" are numbers except where rows are
// copied.  Prints one line per failed check and returns their count.
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "ntsc_frames.hpp"

using namespace ntscsim;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

struct Touched { Span wr; std::vector<Span> rd; };                 // what one descriptor touches
typedef std::vector<std::pair<int, int>> Runs;                     // (index of first descriptor, count) per launch

static int plan(const std::vector<Touched> &call, int cap, Runs &runs, int fail_at = -1)
{
    runs.clear();
    return frames_in_order((int)call.size(), cap, [&](int i, std::vector<Span> &rd) {
        rd.insert(rd.end(), call[(size_t)i].rd.begin(), call[(size_t)i].rd.end());
        return call[(size_t)i].wr;
    }, [&](int first, int m) {
        runs.push_back({first, m});
        return (int)runs.size() - 1 == fail_at ? NTSCSIM_E_HIP : NTSCSIM_OK;
    });
}

// The rule once more, as the obvious quadratic loop: descriptor i starts a new run if the run is at the cap or if i
// conflicts with any single descriptor already in the run.
static bool conflict(const Touched &later, const Touched &earlier)
{
    if (overlaps(later.wr, earlier.wr)) return true;
    for (const Span &r : earlier.rd) if (overlaps(later.wr, r)) return true;
    for (const Span &r : later.rd) if (overlaps(r, earlier.wr)) return true;
    return false;
}

static Runs restated(const std::vector<Touched> &call, int cap)
{
    Runs runs;
    const int n = (int)call.size();
    int first = 0;
    for (int i = 1; i <= n; i++) {
        bool cut = i == n || i - first >= cap;
        for (int j = first; !cut && j < i; j++) cut = conflict(call[(size_t)i], call[(size_t)j]);
        if (cut) { runs.push_back({first, i - first}); first = i; }
    }
    return runs;
}

// 6 slots 256 bytes apart: a short span (240 bytes) stays in its slot, a tall one (480 bytes) reaches over the next
static Span slot_span(int slot, bool tall) { return Span{(uintptr_t)0x100000 + 256u * (uintptr_t)slot, (uintptr_t)0x100000 + 256u * (uintptr_t)slot + (tall ? 480u : 240u)}; }

static void planner_random()
{
    std::mt19937 rng(0x5eed1234u);
    const int caps[4] = {1, 2, 12, 65535};
    int calls = 0, launches = 0, cut_by_hazard = 0;
    for (int it = 0; it < 4000; it++) {
        const int n = (int)(rng() % 41u), cap = caps[rng() % 4u];
        std::vector<Touched> call((size_t)n);
        for (Touched &t : call) {
            t.wr = slot_span((int)(rng() % 6u), (rng() & 1u) != 0);
            const int nr = (int)(rng() % 4u);
            for (int r = 0; r < nr; r++) t.rd.push_back(slot_span((int)(rng() % 6u), (rng() & 1u) != 0));
        }
        Runs got;
        const Runs want = restated(call, cap);
        CHECK(plan(call, cap, got) == NTSCSIM_OK);
        CHECK(got == want);
        calls++;
        launches += (int)got.size();
        for (const auto &r : got) cut_by_hazard += r.second < cap && r.first + r.second < n;
    }
    CHECK(cut_by_hazard > 1000);                                                                     // the draw does exercise the hazards
    std::printf("planner: %d random calls, %d launches, %d cut by a hazard\n", calls, launches, cut_by_hazard);
}

static void planner_edges()
{
    const Span f0{0x1000, 0x10f0}, f1{0x2000, 0x20f0}, f2{0x3000, 0x30f0}, f3{0x4000, 0x40f0};
    Runs r;
    CHECK(plan({}, 65535, r) == NTSCSIM_OK && r.empty());                                            // n = 0: no launch
    CHECK(plan({{f0, {}}}, 1, r) == NTSCSIM_OK && r == Runs({{0, 1}}));
    // a span that touches is not an overlap: written after written, written after read, read after written
    CHECK(plan({{f0, {}}, {Span{f0.b, f0.b + 0xf0}, {}}}, 65535, r) == NTSCSIM_OK && r == Runs({{0, 2}}));
    CHECK(plan({{f0, {f1}}, {Span{f1.b, f1.b + 0xf0}, {}}}, 65535, r) == NTSCSIM_OK && r == Runs({{0, 2}}));
    CHECK(plan({{f0, {}}, {f2, {Span{f0.a - 0xf0, f0.a}}}}, 65535, r) == NTSCSIM_OK && r == Runs({{0, 2}}));
    // an overlap by the last 4 bytes is one, in each of the three roles
    CHECK(plan({{f0, {}}, {Span{f0.b - 4, f0.b + 0xec}, {}}}, 65535, r) == NTSCSIM_OK && r == Runs({{0, 1}, {1, 1}}));
    CHECK(plan({{f0, {f1}}, {Span{f1.b - 4, f1.b + 0xec}, {}}}, 65535, r) == NTSCSIM_OK && r == Runs({{0, 1}, {1, 1}}));
    CHECK(plan({{f0, {}}, {f2, {Span{f0.a - 0xec, f0.a + 4}}}}, 65535, r) == NTSCSIM_OK && r == Runs({{0, 1}, {1, 1}}));
    // two descriptors may read the same frame; the second of three read spans counts as much as the first
    CHECK(plan({{f0, {f3}}, {f1, {f3}}}, 65535, r) == NTSCSIM_OK && r == Runs({{0, 2}}));
    CHECK(plan({{f0, {}}, {f1, {f2, f0, f3}}}, 65535, r) == NTSCSIM_OK && r == Runs({{0, 1}, {1, 1}}));
    // what a run touched is forgotten at a cut: descriptor 2 depends on 0, which is not of its run
    CHECK(plan({{f0, {}}, {f1, {f0}}, {f2, {f0}}}, 65535, r) == NTSCSIM_OK && r == Runs({{0, 1}, {1, 2}}));
    // a failing launch ends the call: later runs are not started
    const std::vector<Touched> four = {{f0, {}}, {f1, {}}, {f2, {}}, {f3, {}}};
    CHECK(plan(four, 1, r, 1) == NTSCSIM_E_HIP && r == Runs({{0, 1}, {1, 1}}));
    CHECK(plan(four, 3, r, 0) == NTSCSIM_E_HIP && r == Runs({{0, 3}}));
    CHECK(plan(four, 3, r, 1) == NTSCSIM_E_HIP && r == Runs({{0, 3}, {3, 1}}));                      // the last run fails
    CHECK(plan(four, 3, r) == NTSCSIM_OK && r == Runs({{0, 3}, {3, 1}}));
}

static void writes_checks()
{
    const uintptr_t F = 0xf0;
    const Span o0{0x3000, 0x3000 + F}, o1{0x1000, 0x1000 + F}, o2{0x2000, 0x2000 + F};              // not in address order
    { CallWrites w; CHECK(w.sort() == NTSCSIM_OK && !w.hits(o0) && !w.hits(Span{0, ~(uintptr_t)0})); }   // the empty set
    {   // two outputs that overlap by their last dword; two that touch
        CallWrites w; w.add(o0); w.add(o1); w.add(Span{o1.b - 4, o1.b - 4 + F});
        CHECK(w.sort() == NTSCSIM_E_ARG);
        CallWrites t; t.add(o0); t.add(Span{o1.b, o1.b + F}); t.add(o1);
        CHECK(t.sort() == NTSCSIM_OK);
        CallWrites same; same.add(o0); same.add(o0);
        CHECK(same.sort() == NTSCSIM_E_ARG);
    }
    {   // a source over the first, the last and a middle output (in address order: o1, o2, o0), from either side
        CallWrites w; w.add(o0); w.add(o1); w.add(o2);
        CHECK(w.sort() == NTSCSIM_OK);
        for (const Span &o : {o1, o2, o0}) {
            CHECK(w.hits(o));
            CHECK(w.hits(Span{o.b - 4, o.b - 4 + F}) && w.hits(Span{o.a + 4 - F, o.a + 4}));       // by one dword
            CHECK(!w.hits(Span{o.b, o.b + F}) && !w.hits(Span{o.a - F, o.a}));                       // only touching
            CHECK(w.hits(Span{o.a - 8, o.b + 8}) && w.hits(Span{o.a + 8, o.a + 12}));                // around it, within it
        }
        CHECK(w.hits(Span{0x1800, 0x2004}) && !w.hits(Span{0x1800, 0x2000}));                        // between two outputs
        CHECK(!w.hits(Span{0x100, 0x200}) && !w.hits(Span{0x9000, 0x9100}));                         // in front of all, behind all
        CHECK(w.hits(Span{0x100, 0x9000}));                                                          // over all of them
    }
}

static void plane_and_rows_checks()
{
    const int W = 10;
    alignas(16) static unsigned char mem[16];
    for (int aligned = 0; aligned < 2; aligned++) {
        const bool al = aligned != 0;
        CHECK(plane_check(mem, 4 * W - 4, W, al) == NTSCSIM_E_SIZE);
        CHECK(plane_check(mem, 4 * W, W, al) == NTSCSIM_OK);
        CHECK(plane_check(mem, 4 * W + 2, W, al) == (al ? NTSCSIM_E_SIZE : NTSCSIM_OK));
        CHECK(plane_check(mem + 2, 4 * W, W, al) == (al ? NTSCSIM_E_SIZE : NTSCSIM_OK));
        CHECK(plane_check(mem + 2, 4 * W - 4, W, al) == NTSCSIM_E_SIZE);
        CHECK(plane_check(mem + 4, 4 * W + 4, W, al) == NTSCSIM_OK);
    }
    // 6 rows of 40 bytes from pitch 40 to pitch 48 and back: the 8 bytes behind each destination row stay
    const int H = 6;
    std::vector<unsigned char> a((size_t)40 * H), b((size_t)48 * H, 0xEE), c((size_t)40 * H, 0);
    for (size_t i = 0; i < a.size(); i++) a[i] = (unsigned char)(i * 7 + 1);
    copy_rows(b.data(), 48, a.data(), 40, 40, H);
    for (int y = 0; y < H; y++) {
        CHECK(std::memcmp(b.data() + 48 * y, a.data() + 40 * y, 40) == 0);
        for (int x = 40; x < 48; x++) CHECK(b[(size_t)(48 * y + x)] == 0xEE);
    }
    copy_rows(c.data(), 40, b.data(), 48, 40, H);
    CHECK(c == a);
    copy_rows(c.data(), 40, b.data(), 48, 40, 0);                                                    // no rows: nothing is touched
    CHECK(c == a);
}

int main()
{
    CHECK(overlaps(Span{0, 4}, Span{3, 8}) && !overlaps(Span{0, 4}, Span{4, 8}) && !overlaps(Span{4, 8}, Span{0, 4}));
    planner_random();
    planner_edges();
    writes_checks();
    plane_and_rows_checks();
    std::printf("%s: %d failed\n", "frames_host_check", g_failed);
    return g_failed;
}
