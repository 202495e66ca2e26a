// mixed_plan_check.cpp -- csrc/mixed_plan.hpp on the host (tests/test_mixed_plan_host.py builds this with g++, plain and
// with the address and undefined-behaviour sanitizers, and runs it): for hand-made and pseudo-random calls
//   * groups stand in order of first use, and a group's fields in the caller's order (stable);
//   * every group starts at a multiple of 64 rows, holds nf * Lslot rows, and no two groups overlap;
//   * the block tables cover every row of every group exactly once (encoder: 64 rows a block; decoder: 63 rows a block,
//     a class's table holding exactly that class's groups), and no block spans two groups;
//   * the rand() positions equal a plain serial walk in the caller's order, explicit and AUTO positions mixed;
//   * the limits trip where the single-set call's would, computed for the padded space.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "mixed_plan.hpp"

using namespace ntscsim::mixed;

static long long checks = 0, bad = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        checks++;                                                                          \
        if (!(cond)) { if (bad++ < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static uint64_t lcg_state = 0x243F6A8885A308D3ull;
static uint32_t rnd()
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg_state >> 33);
}

static void check_plan(const std::vector<Field> &f, int n_sets, const std::vector<SetInfo> &info, int Lslot, int W,
                       uint64_t start)
{
    const int n = (int)f.size();
    Plan p;
    const int rc = make_plan(f.data(), n, n_sets, info.data(), Lslot, W, false, start, p);
    CHECK(rc == PLAN_OK);
    if (rc != PLAN_OK) return;

    // ---- groups: first-use order, stable inside
    std::vector<int> first_use;
    std::map<int, std::vector<int>> members;
    for (int i = 0; i < n; i++) {
        if (!members.count(f[(size_t)i].set)) first_use.push_back(f[(size_t)i].set);
        members[f[(size_t)i].set].push_back(i);
    }
    CHECK(p.groups.size() == first_use.size());
    CHECK((int)p.order.size() == n && (int)p.slot.size() == n && (int)p.group_of.size() == n);
    int at = 0;
    for (size_t g = 0; g < p.groups.size() && g < first_use.size(); g++) {
        const Group &G = p.groups[g];
        const std::vector<int> &m = members[first_use[g]];
        CHECK(G.set == first_use[g]);
        CHECK(G.nf == (int)m.size());
        CHECK(G.field0 == at);
        CHECK(G.cls == info[(size_t)(G.set + 1)].cls);
        for (size_t k = 0; k < m.size(); k++) {
            CHECK(p.order[(size_t)at + k] == m[k]);
            CHECK(p.slot[(size_t)m[k]] == at + (int)k);
            CHECK(p.group_of[(size_t)at + k] == (int)g);
        }
        at += G.nf;
    }
    CHECK(at == n);

    // ---- rows: bases, sizes, no overlap, Rpad
    long long end_prev = 0;
    for (const Group &G : p.groups) {
        CHECK(G.base % 64 == 0);
        CHECK(G.R == (long long)G.nf * Lslot);
        CHECK(G.base >= end_prev);
        CHECK(G.base - end_prev < 64);
        end_prev = (long long)G.base + G.R;
    }
    CHECK(p.R == end_prev);
    CHECK(p.Rpad % 64 == 0 && p.Rpad >= p.R + 64 && p.Rpad < p.R + 128);

    // ---- block tables: every row of every group exactly once, no block across two groups
    {
        std::vector<unsigned char> enc((size_t)p.Rpad, 0), dec((size_t)p.Rpad, 0);
        size_t b = 0;
        for (const BlockRef &r : p.enc_tab) {
            CHECK(r.group >= 0 && (size_t)r.group < p.groups.size());
            const Group &G = p.groups[(size_t)r.group];
            CHECK((int)b == G.enc_block0 + r.block);
            CHECK(r.block >= 0 && r.block < G.enc_blocks);
            for (int l = 0; l < 64; l++) {
                const long long rho = (long long)r.block * 64 + l;
                if (rho < G.R) enc[(size_t)(G.base + rho)]++;
            }
            b++;
        }
        for (int c = 0; c < N_CLS; c++) {
            b = 0;
            for (const BlockRef &r : p.dec_tab[c]) {
                CHECK(r.group >= 0 && (size_t)r.group < p.groups.size());
                const Group &G = p.groups[(size_t)r.group];
                CHECK(G.cls == c);
                CHECK((int)b == G.dec_block0 + r.block);
                CHECK(r.block >= 0 && r.block < G.dec_blocks);
                for (int l = 1; l < 64; l++) {          // lane 0 is the halo: it stores nothing
                    const long long gidx = (long long)r.block * 63 + l - 1;
                    if (gidx < G.R) dec[(size_t)(G.base + gidx)]++;
                }
                b++;
            }
        }
        std::vector<unsigned char> want((size_t)p.Rpad, 0);
        for (const Group &G : p.groups)
            for (int r = 0; r < G.R; r++) want[(size_t)(G.base + r)]++;
        bool ok_e = true, ok_d = true, ok_w = true;
        for (size_t r = 0; r < want.size(); r++) {
            ok_w = ok_w && want[r] <= 1;
            ok_e = ok_e && enc[r] == want[r];
            ok_d = ok_d && dec[r] == want[r];
        }
        CHECK(ok_w); CHECK(ok_e); CHECK(ok_d);
    }

    // ---- rand(): a plain serial walk in the caller's order
    uint64_t pos = start;
    bool ok = (int)p.rng_start.size() == n;
    for (int i = 0; i < n && ok; i++) {
        if (f[(size_t)i].rng_pos != RNG_AUTO) pos = f[(size_t)i].rng_pos;
        ok = p.rng_start[(size_t)i] == pos;
        pos += info[(size_t)(f[(size_t)i].set + 1)].calls[f[(size_t)i].parity & 1u];
    }
    CHECK(ok);
    CHECK(p.rng_end == pos);
}

static std::vector<SetInfo> make_info(int n_sets)
{
    std::vector<SetInfo> info((size_t)n_sets + 1);
    for (size_t s = 0; s < info.size(); s++) {
        info[s].calls[0] = rnd() % 400000u;
        info[s].calls[1] = info[s].calls[0] - (info[s].calls[0] ? rnd() % 2u : 0u);
        info[s].cls = (int)(rnd() % (unsigned)N_CLS);
    }
    return info;
}

static void hand_made()
{
    // nothing to do
    {
        Plan p;
        CHECK(make_plan(nullptr, 0, 0, nullptr, 8, 64, false, 77, p) == PLAN_OK);
        CHECK(p.groups.empty() && p.rng_end == 77 && p.enc_tab.empty());
        CHECK(make_plan(nullptr, -1, 0, nullptr, 8, 64, false, 0, p) == PLAN_E_ARG);
        CHECK(make_plan(nullptr, 1, 0, nullptr, 8, 64, false, 0, p) == PLAN_E_ARG);
    }
    // sets 2, -1, 2, 0, -1 with Lslot 63: groups {2: 0, 2}, {-1: 1, 4}, {0: 3}
    {
        std::vector<SetInfo> info = {{{10, 9}, CLS_VCR_COMP}, {{100, 99}, CLS_TV}, {{0, 0}, CLS_TV}, {{1000, 999}, CLS_VCR_SVIDEO}};
        std::vector<Field> f = {{2, 1, RNG_AUTO}, {-1, 0, RNG_AUTO}, {2, 0, 5000}, {0, 1, RNG_AUTO}, {-1, 1, RNG_AUTO}};
        Plan p;
        CHECK(make_plan(f.data(), 5, 3, info.data(), 63, 64, false, 7, p) == PLAN_OK);
        CHECK(p.groups.size() == 3);
        if (p.groups.size() == 3) {
            CHECK(p.groups[0].set == 2 && p.groups[1].set == -1 && p.groups[2].set == 0);
            CHECK(p.groups[0].base == 0 && p.groups[0].R == 126 && p.groups[0].enc_blocks == 2 && p.groups[0].dec_blocks == 2);
            CHECK(p.groups[1].base == 128 && p.groups[1].R == 126);
            CHECK(p.groups[2].base == 256 && p.groups[2].R == 63 && p.groups[2].enc_blocks == 1 && p.groups[2].dec_blocks == 1);
            CHECK(p.R == 319 && p.Rpad == 384);
            CHECK(p.order == (std::vector<int32_t>{0, 2, 1, 4, 3}));
            CHECK(p.rng_start == (std::vector<uint64_t>{7, 7 + 999, 5000, 6000, 6099}));
            CHECK(p.rng_end == 6099 + 9);
            CHECK(p.dec_tab[CLS_VCR_SVIDEO].size() == 2 && p.dec_tab[CLS_VCR_COMP].size() == 2 && p.dec_tab[CLS_TV].size() == 1);
        }
        check_plan(f, 3, info, 63, 64, 7);
    }
    // group row counts on, one short of and one past multiples of 63 and 64
    for (int Lslot : {62, 63, 64, 65}) {
        std::vector<SetInfo> info = make_info(3);
        for (int rev = 0; rev < 2; rev++) {
            std::vector<Field> f;
            for (int s = 0; s < 3; s++) {
                const int set = rev ? 2 - s : s;
                for (int k = 0; k <= set; k++) f.push_back(Field{set, (uint32_t)(k & 1), RNG_AUTO});
            }
            check_plan(f, 3, info, Lslot, 64, 0);
        }
    }
}

static void limits()
{
    std::vector<SetInfo> info = make_info(2);
    Plan p;
    // the single-set limit on rows: n * Lslot <= 2^30 ...
    {
        const int Lslot = 8192, n = 131072;                        // exactly 2^30 rows, one group: the plane is the limit
        std::vector<Field> f((size_t)n, Field{0, 0, RNG_AUTO});
        CHECK(make_plan(f.data(), n, 2, info.data(), Lslot, 16, false, 0, p) == PLAN_E_SIZE);     // Rpad * 16 > 2^31
        CHECK(make_plan(f.data(), n / 16, 2, info.data(), Lslot, 16, false, 0, p) == PLAN_OK);
        CHECK(make_plan(f.data(), n / 8, 2, info.data(), Lslot, 16, false, 0, p) == PLAN_E_SIZE); // 2^27 rows + 64 pad, W 16
    }
    // ... and the padding between groups counts: two groups of 1 field, Lslot 1, W 16384 -- Rpad = 64 + 1 -> 128 + 64
    {
        std::vector<Field> f = {{0, 0, RNG_AUTO}, {1, 0, RNG_AUTO}};
        CHECK(make_plan(f.data(), 2, 2, info.data(), 1, 16384, false, 0, p) == PLAN_OK);
        CHECK(p.R == 65 && p.Rpad == 192);
    }
    // plane limit Rpad * W <= 2^31 for the padded space: W = 16384 allows Rpad <= 131072.  2047 groups of one row (Lslot 1)
    // end at row 2046 * 64 + 1 = 130945 -> Rpad 131072: allowed; 2048 groups -> Rpad 131136: refused, although the same
    // 2048 fields in ONE group (Rpad 2112) pass, as they do in the single-set call
    {
        std::vector<SetInfo> many = make_info(2048);
        std::vector<Field> f;
        for (int s = 0; s < 2047; s++) f.push_back(Field{s, 0, RNG_AUTO});
        CHECK(make_plan(f.data(), 2047, 2048, many.data(), 1, 16384, false, 0, p) == PLAN_OK);
        CHECK(p.Rpad == 131072);
        f.push_back(Field{2047, 0, RNG_AUTO});
        CHECK(make_plan(f.data(), 2048, 2048, many.data(), 1, 16384, false, 0, p) == PLAN_E_SIZE);
        for (Field &x : f) x.set = 5;
        CHECK(make_plan(f.data(), 2048, 2048, many.data(), 1, 16384, false, 0, p) == PLAN_OK);
        CHECK(p.Rpad == 2112);
    }
    // row limit 2^30 with padding: groups of 1 row each at 64-row pitch reach it with 2^24 groups; W = 16 keeps the plane
    // limit (2^27 rows) in front of it, so the plane limit is the one that trips first for every allowed W
    // bob: one grid row per field
    {
        std::vector<Field> f(65536, Field{0, 0, RNG_AUTO});
        CHECK(make_plan(f.data(), 65536, 2, info.data(), 1, 16, true, 0, p) == PLAN_E_SIZE);
        CHECK(make_plan(f.data(), 65535, 2, info.data(), 1, 16, true, 0, p) == PLAN_OK);
        CHECK(make_plan(f.data(), 65536, 2, info.data(), 1, 16, false, 0, p) == PLAN_OK);
    }
}

static void random_calls()
{
    static const int LSLOTS[] = {1, 8, 62, 63, 64, 65, 243};
    for (int iter = 0; iter < 160; iter++) {
        const int Lslot = LSLOTS[iter % 7];
        const int n_sets = 1 + (int)(rnd() % 64u);
        const int n = iter < 8 ? 5000 - iter : 1 + (int)(rnd() % (iter % 5 == 0 ? 5000u : 200u));
        std::vector<SetInfo> info = make_info(n_sets);
        std::vector<Field> f((size_t)n);
        const unsigned style = rnd() % 3u;      // 0: any set, 1: a few sets, 2: runs of one set
        int run_set = -1;
        for (int i = 0; i < n; i++) {
            int set;
            if (style == 0) set = (int)(rnd() % (unsigned)(n_sets + 1)) - 1;
            else if (style == 1) set = (int)(rnd() % (unsigned)(n_sets < 3 ? n_sets : 3));
            else { if (i == 0 || rnd() % 7u == 0) run_set = (int)(rnd() % (unsigned)(n_sets + 1)) - 1; set = run_set; }
            const uint64_t pos = rnd() % 3u == 0 ? (uint64_t)rnd() * (rnd() % 1000u) : RNG_AUTO;
            f[(size_t)i] = Field{set, rnd() & 1u, pos};
        }
        check_plan(f, n_sets, info, Lslot, 64, (uint64_t)rnd());
    }
}

int main()
{
    hand_made();
    limits();
    random_calls();
    std::printf("mixed_plan: %lld checks, %lld bad\n", checks, bad);
    return bad ? 1 : 0;
}
