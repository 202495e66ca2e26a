// mixed_plan422_check.cpp -- what csrc/mixed_plan.hpp gained for ntscsim_mixed_fields422_device(), swept on the host
// (tests/test_mixed_plan422_host.py builds it with plain g++ and with the sanitizers and runs it):
//   - fields that draw nothing (Field::nodraw), mixed into AUTO and explicit positions, against a naive restatement;
//   - the composite-plane limit switched off: 65535 fields of Lslot 243 at W 720 pass, 65536 are refused;
//   - a plan with no such field and the limit on is the plan of a caller that knows of neither.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mixed_plan.hpp"

using namespace ntscsim::mixed;

static long long checks = 0, bad = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        checks++;                                                                      \
        if (!(cond)) { if (bad++ < 20) std::printf("line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17;
    return (uint32_t)(rnd_state >> 24);
}

static bool same_plan(const Plan &a, const Plan &b)
{
    if (a.groups.size() != b.groups.size() || a.order != b.order || a.slot != b.slot || a.group_of != b.group_of ||
        a.rng_start != b.rng_start || a.rng_end != b.rng_end || a.R != b.R || a.Rpad != b.Rpad) return false;
    for (size_t g = 0; g < a.groups.size(); g++) {
        const Group &x = a.groups[g], &y = b.groups[g];
        if (x.set != y.set || x.nf != y.nf || x.field0 != y.field0 || x.cls != y.cls || x.R != y.R || x.base != y.base ||
            x.enc_blocks != y.enc_blocks || x.dec_blocks != y.dec_blocks || x.enc_block0 != y.enc_block0 ||
            x.dec_block0 != y.dec_block0) return false;
    }
    auto same_tab = [](const std::vector<BlockRef> &p, const std::vector<BlockRef> &q) {
        if (p.size() != q.size()) return false;
        for (size_t i = 0; i < p.size(); i++) if (p[i].group != q[i].group || p[i].block != q[i].block) return false;
        return true;
    };
    if (!same_tab(a.enc_tab, b.enc_tab)) return false;
    for (int c = 0; c < N_CLS; c++) if (!same_tab(a.dec_tab[c], b.dec_tab[c])) return false;
    return true;
}

int main()
{
    static const int LSLOTS[] = {1, 8, 62, 63, 64, 65, 243};
    for (int round = 0; round < 200; round++) {
        const int n_sets = 1 + (int)(rnd() % 40);
        const int n = 1 + (int)(rnd() % 3000);
        const int Lslot = LSLOTS[rnd() % 7];
        const int W = 16 + 2 * (int)(rnd() % 360);
        std::vector<SetInfo> info((size_t)n_sets + 1);
        for (auto &s : info) { s.calls[0] = rnd() % 500000; s.calls[1] = rnd() % 500000; s.cls = CLS_TV; }
        const uint64_t start = rnd();
        std::vector<Field> f((size_t)n), plain((size_t)n);
        for (int i = 0; i < n; i++) {
            const int32_t set = (int32_t)(rnd() % (uint32_t)(n_sets + 1)) - 1;
            // explicit positions jump about, also backwards
            const uint64_t pos = (rnd() % 5 == 0) ? (uint64_t)(rnd() % 1000000) : RNG_AUTO;
            f[(size_t)i] = Field{set, rnd() & 1u, pos, (rnd() % 3 == 0) ? 1u : 0u};
            plain[(size_t)i] = Field{set, f[(size_t)i].parity, pos};
            CHECK(plain[(size_t)i].nodraw == 0u);      // the flag defaults to "draws"
        }
        Plan p;
        CHECK(make_plan(f.data(), n, n_sets, info.data(), Lslot, W, true, start, p, false) == PLAN_OK);
        // the naive restatement: walk the caller's order
        uint64_t pos = start;
        for (int i = 0; i < n; i++) {
            if (f[(size_t)i].rng_pos != RNG_AUTO) pos = f[(size_t)i].rng_pos;
            CHECK(p.rng_start[(size_t)i] == pos);
            if (f[(size_t)i].nodraw == 0u) pos += info[(size_t)(f[(size_t)i].set + 1)].calls[f[(size_t)i].parity];
        }
        CHECK(p.rng_end == pos);
        // the flag moves positions only: groups, rows and blocks are those of the plan without it
        Plan q, q0, q1;
        CHECK(make_plan(plain.data(), n, n_sets, info.data(), Lslot, W, true, start, q, false) == PLAN_OK);
        CHECK(p.order == q.order && p.group_of == q.group_of && p.R == q.R && p.Rpad == q.Rpad);
        CHECK(p.enc_tab.size() == q.enc_tab.size() && p.dec_tab[0].size() == q.dec_tab[0].size());
        // no such field, limit on (spelt out | left to the default): one and the same plan, with and without any_bob
        for (int bob = 0; bob < 2; bob++) {
            const int r0 = make_plan(plain.data(), n, n_sets, info.data(), Lslot, W, bob != 0, start, q0, true);
            const int r1 = make_plan(plain.data(), n, n_sets, info.data(), Lslot, W, bob != 0, start, q1);
            CHECK(r0 == r1);
            if (r0 == PLAN_OK && r1 == PLAN_OK) CHECK(same_plan(q0, q1));
            // ... and where the plane fits, the limit changes nothing
            if (r0 == PLAN_OK && bob) CHECK(same_plan(q0, q));
        }
        // every process block of 63 rows lies in one group: the rows of a group in exactly one block each
        long long rows = 0;
        for (const BlockRef &b : p.dec_tab[0]) {
            const Group &g = p.groups[(size_t)b.group];
            CHECK(b.block >= 0 && b.block < g.dec_blocks && (long long)b.block * 63 < g.R);
            const long long last = (long long)b.block * 63 + 63 < g.R ? (long long)b.block * 63 + 63 : g.R;
            rows += last - (long long)b.block * 63;
        }
        CHECK(rows == (long long)n * Lslot);
    }
    {   // the plane limit off: a frame library of 65535 fields of 720 x 486 passes, one more is refused (grid planes);
        // with the limit on even 65535 are refused (Rpad * W > 2^31)
        std::vector<SetInfo> info(2);
        info[0] = SetInfo{{1, 2}, CLS_TV}; info[1] = SetInfo{{3, 4}, CLS_TV};
        std::vector<Field> f(65536, Field{0, 0, RNG_AUTO});
        for (size_t i = 0; i < f.size(); i += 3) f[i].nodraw = 1;
        Plan p;
        CHECK(make_plan(f.data(), 65535, 1, info.data(), 243, 720, true, 7, p, false) == PLAN_OK);
        CHECK(p.R == 65535 * 243 && p.Rpad == ((65535 * 243 + 63) / 64) * 64 + 64);
        CHECK(p.dec_tab[0].size() == (size_t)((65535ll * 243 + 62) / 63));
        CHECK(p.rng_end == 7 + 3ull * (65535 - (65535 + 2) / 3));
        CHECK(make_plan(f.data(), 65536, 1, info.data(), 243, 720, true, 7, p, false) == PLAN_E_SIZE);
        CHECK(p.rng_end == 7);
        CHECK(make_plan(f.data(), 65535, 1, info.data(), 243, 720, true, 7, p, true) == PLAN_E_SIZE);
        CHECK(make_plan(f.data(), 65535, 1, info.data(), 243, 720, true, 7, p) == PLAN_E_SIZE);
        // the row limit stays whatever the plane limit (refused before anything is laid out)
        std::vector<Field> big((size_t)(1 << 16), Field{0, 0, RNG_AUTO});
        CHECK(make_plan(big.data(), (1 << 16) - 1, 1, info.data(), (1 << 14) + 1, 16, false, 0, p, false) == PLAN_E_SIZE);
        // a call of fields that all draw nothing leaves the position where it starts
        big[0].set = -1;
        for (auto &x : big) x.nodraw = 1;
        CHECK(make_plan(big.data(), 1 << 16, 1, info.data(), 3, 16, false, 99, p, false) == PLAN_OK);
        CHECK(p.rng_end == 99 && p.groups.size() == 2 && p.groups[1].base == 64);
    }
    std::printf("mixed_plan422: %lld checks, %lld bad\n", checks, bad);
    return bad ? 1 : 0;
}
