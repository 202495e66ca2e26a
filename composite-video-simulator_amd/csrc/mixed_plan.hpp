// mixed_plan.hpp -- the host plan of ntscsim_mixed_fields_device(): fields of one call that name different parameter
// sets, laid out so that every kernel of the chain runs ONCE over all of them.  No HIP in it: plain integer code over
// std::vector, so tests/mixed_plan_check.cpp sweeps it with g++ (plain and with the sanitizers).
//
//   1. groups   the descriptors sorted stably by the set they name, one group per named set, groups in order of first
//               use.  order[] is the sorted order (the records are uploaded in it), slot[] its inverse.
//   2. rows     group g holds nf_g fields = R_g = nf_g * Lslot scanlines of ONE common scanline space; its first row
//               base_g is a multiple of 64.  Rows R_g .. base_{g+1} - 1 belong to nobody.  The planes' row stride Rpad
//               is the whole space rounded as ntscsim_fields_device() rounds its own.
//   3. blocks   encoder blocks of 64 rows and decoder blocks of 63 rows (lane 0 of a decoder block is the halo of the
//               vertical blend) are counted WITHIN a group, and two tables map a launch-wide block index to (group,
//               block within the group): a workgroup never spans two groups, so its parameters are wave-uniform.  The
//               decoder has one table per decoder class (no VCR | VCR with composite out | VCR with S-Video out):
//               a class is a template instantiation, hence a launch of its own over its groups' blocks only.
//   4. rand()   every descriptor's start position in the CALLER's order: an explicit position stands, NTSCSIM_RNG_AUTO
//               continues behind the previous descriptor, which advanced by the draws of ITS set and parity -- or by
//               nothing, if it is marked `nodraw` (ntscsim_mixed_fields422_device(): NTSCSIM_422_NOCOMP).
//
// All sizes are computed in 64 bits and checked against the limits of the single-set call (prepare_records(),
// ntscsim_hip.hip) before anything is narrowed.
#pragma once
#include <cstdint>
#include <vector>

namespace ntscsim {
namespace mixed {

enum { PLAN_OK = 0, PLAN_E_ARG = -1, PLAN_E_SIZE = -2 };      // the values of NTSCSIM_OK / _E_ARG / _E_SIZE
enum { CLS_TV = 0, CLS_VCR_COMP = 1, CLS_VCR_SVIDEO = 2, N_CLS = 3 };

constexpr uint64_t RNG_AUTO = UINT64_MAX;                     // NTSCSIM_RNG_AUTO
constexpr long long MAX_ROWS = 1ll << 30;                     // rows of the scanline space
constexpr long long MAX_PLANE = 1ll << 31;                    // elements of the composite plane (Rpad * W)
constexpr int MAX_BOB_FIELDS = 65535;                         // k_bob / k_mixed_bob: one grid row per field

// what the plan needs to know of one descriptor
struct Field {
    int32_t set;          // -1 .. n_sets - 1
    uint32_t parity;      // 0 | 1
    uint64_t rng_pos;     // or RNG_AUTO
    uint32_t nodraw = 0;  // 1: the field draws nothing, the position stays where it starts (default: it draws)
};

// what it needs to know of one set; entry 0 is set -1 (the ctx's own parameters), entry s + 1 is sets[s].  Entries of
// sets that no descriptor names are never read.
struct SetInfo {
    uint64_t calls[2];    // rand() draws of one field, by parity
    int cls;              // CLS_*
};

struct Group {
    int32_t set;
    int32_t nf;           // fields
    int32_t field0;       // its first field in the sorted order
    int32_t cls;
    int32_t R;            // nf * Lslot
    int32_t base;         // first row, multiple of 64
    int32_t enc_blocks, dec_blocks;
    int32_t enc_block0;   // its first block in the encoder launch
    int32_t dec_block0;   // ... in its class's decoder launch
};

struct BlockRef { int32_t group, block; };

struct Plan {
    std::vector<Group> groups;
    std::vector<int32_t> order;                // sorted position -> caller index
    std::vector<int32_t> slot;                 // caller index -> sorted position
    std::vector<int32_t> group_of;             // sorted position -> group
    std::vector<BlockRef> enc_tab;
    std::vector<BlockRef> dec_tab[N_CLS];
    std::vector<uint64_t> rng_start;           // caller order
    uint64_t rng_end = 0;
    int32_t R = 0;                             // end of the last group's rows
    int32_t Rpad = 0;
};

// (set, parity) are taken as validated: set in -1 .. n_sets - 1, parity 0 | 1.  any_bob: some kernel of the caller has
// one grid plane per field.  plane_limit: the caller keeps a composite plane of Rpad * W elements (the YUV422P tool
// has none, its call switches the limit off).
inline int make_plan(const Field *f, int n, int n_sets, const SetInfo *info, int Lslot, int W, bool any_bob,
                     uint64_t start_pos, Plan &p, bool plane_limit = true)
{
    p = Plan();
    p.rng_end = start_pos;
    if (n < 0 || n_sets < 0 || Lslot < 1 || W < 1 || (n > 0 && (!f || !info))) return PLAN_E_ARG;
    if (n == 0) return PLAN_OK;
    if (any_bob && n > MAX_BOB_FIELDS) return PLAN_E_SIZE;
    if ((long long)n * Lslot > MAX_ROWS) return PLAN_E_SIZE;          // (the padded space is no smaller)

    // ---- 1. groups in order of first use, stable inside
    std::vector<int32_t> group_of_set((size_t)n_sets + 1, -1);
    for (int i = 0; i < n; i++) {
        const size_t s = (size_t)(f[i].set + 1);
        if (group_of_set[s] < 0) {
            group_of_set[s] = (int32_t)p.groups.size();
            Group g = Group();
            g.set = f[i].set;
            g.cls = info[s].cls;
            p.groups.push_back(g);
        }
        p.groups[(size_t)group_of_set[s]].nf++;
    }
    const size_t ng = p.groups.size();
    {
        int32_t at = 0;
        for (Group &g : p.groups) { g.field0 = at; at += g.nf; }
    }
    p.order.resize((size_t)n); p.slot.resize((size_t)n); p.group_of.resize((size_t)n);
    {
        std::vector<int32_t> fill(ng, 0);
        for (int i = 0; i < n; i++) {
            const int32_t g = group_of_set[(size_t)(f[i].set + 1)];
            const int32_t at = p.groups[(size_t)g].field0 + fill[(size_t)g]++;
            p.order[(size_t)at] = i; p.slot[(size_t)i] = at; p.group_of[(size_t)at] = g;
        }
    }

    // ---- 2. rows: 64 bits until the whole space has been checked
    long long row = 0, enc_total = 0, dec_total[N_CLS] = {0, 0, 0};
    for (Group &g : p.groups) {
        const long long R = (long long)g.nf * Lslot;
        if (row + R > MAX_ROWS) return PLAN_E_SIZE;
        g.base = (int32_t)row; g.R = (int32_t)R;
        g.enc_blocks = (int32_t)((R + 63) / 64);
        g.dec_blocks = (int32_t)((R + 62) / 63);
        g.enc_block0 = (int32_t)enc_total;
        g.dec_block0 = (int32_t)dec_total[g.cls];
        enc_total += g.enc_blocks;
        dec_total[g.cls] += g.dec_blocks;
        p.R = (int32_t)(row + R);
        row = ((row + R + 63) / 64) * 64;
    }
    const long long Rpad = (((long long)p.R + 63) / 64) * 64 + 64;
    if (plane_limit && Rpad * (long long)W > MAX_PLANE) return PLAN_E_SIZE;
    p.Rpad = (int32_t)Rpad;

    // ---- 3. block -> (group, block within the group)
    p.enc_tab.reserve((size_t)enc_total);
    for (int c = 0; c < N_CLS; c++) p.dec_tab[c].reserve((size_t)dec_total[c]);
    for (size_t g = 0; g < ng; g++) {
        const Group &G = p.groups[g];
        for (int32_t b = 0; b < G.enc_blocks; b++) p.enc_tab.push_back(BlockRef{(int32_t)g, b});
        for (int32_t b = 0; b < G.dec_blocks; b++) p.dec_tab[G.cls].push_back(BlockRef{(int32_t)g, b});
    }

    // ---- 4. rand() positions, in the caller's order
    p.rng_start.resize((size_t)n);
    uint64_t pos = start_pos;
    for (int i = 0; i < n; i++) {
        if (f[i].rng_pos != RNG_AUTO) pos = f[i].rng_pos;
        p.rng_start[(size_t)i] = pos;
        if (!f[i].nodraw) pos += info[(size_t)(f[i].set + 1)].calls[f[i].parity & 1u];
    }
    p.rng_end = pos;
    return PLAN_OK;
}

} // namespace mixed
} // namespace ntscsim
