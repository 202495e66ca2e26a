// mixed_forms_check.cpp -- csrc/mixed_forms.hpp on the host (tests/test_mixed_forms_host.py builds this with g++, plain and
// with the address and undefined-behaviour sanitizers, and runs it):
//   * make_form_tables over pseudo-random plans and form assignments: every group's blocks appear exactly once, in the
//     table of its form, in order, groups in the plan's order; the table sizes add up to the plan's totals; dec_max is the
//     largest decoder table; a form that does not fit the group's decoder class is refused;
//   * form_of swept over ALL combinations of the facts against a second statement of the rule, written form by form as
//     the list of conditions of that form (the launcher's comments, not the header's code);
//   * from a set and a call that take a hand-tuned form, every precondition flipped on its own changes exactly the forms
//     it guards: the source alignment the encoder only, the destination alignment the decoder only, ...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mixed_forms.hpp"

using namespace ntscsim::mixed;

static long long checks = 0, bad = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        checks++;                                                                          \
        if (!(cond)) { if (bad++ < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static uint64_t lcg_state = 0x13198A2E03707344ull;
static uint32_t rnd()
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg_state >> 33);
}

// ------------------------------------------------------------------------------------------------ tables
static void check_tables(int n, int n_sets, int Lslot)
{
    std::vector<Field> f((size_t)n);
    for (Field &x : f) { x.set = (int32_t)(rnd() % (uint32_t)(n_sets + 1)) - 1; x.parity = rnd() & 1u; x.rng_pos = RNG_AUTO; }
    std::vector<SetInfo> info((size_t)n_sets + 1);
    for (SetInfo &s : info) { s.calls[0] = 3; s.calls[1] = 5; s.cls = (int)(rnd() % N_CLS); }
    Plan p;
    CHECK(make_plan(f.data(), n, n_sets, info.data(), Lslot, 64, false, 0, p) == PLAN_OK);
    const size_t ng = p.groups.size();
    std::vector<int> ef(ng), df(ng);
    for (size_t g = 0; g < ng; g++) {
        ef[g] = (int)(rnd() % N_ENC);
        // the generic form of the group's OWN class, or any hand-tuned form
        const int d = (int)(rnd() % (N_DEC - N_CLS + 1));
        df[g] = d == 0 ? p.groups[g].cls : N_CLS + d - 1;
    }
    FormTables t;
    CHECK(make_form_tables(p, ef.data(), df.data(), t));

    size_t enc_sum = 0, dec_sum = 0, dec_plan = 0, dmax = 0;
    for (int e = 0; e < N_ENC; e++) enc_sum += t.enc[e].size();
    for (int d = 0; d < N_DEC; d++) { dec_sum += t.dec[d].size(); if (t.dec[d].size() > dmax) dmax = t.dec[d].size(); }
    for (int c = 0; c < N_CLS; c++) dec_plan += p.dec_tab[c].size();
    CHECK(enc_sum == p.enc_tab.size());
    CHECK(dec_sum == dec_plan);
    CHECK(t.dec_max == dmax);

    // walk every table: groups ascending, a group's blocks 0 .. blocks-1 in a row, and only groups of that form
    std::vector<int> enc_seen(ng, 0), dec_seen(ng, 0);
    for (int e = 0; e < N_ENC; e++) {
        size_t i = 0;
        int last_g = -1;
        while (i < t.enc[e].size()) {
            const int g = t.enc[e][i].group;
            CHECK(g > last_g && g >= 0 && (size_t)g < ng);
            if (g < 0 || (size_t)g >= ng) return;
            CHECK(ef[(size_t)g] == e);
            for (int b = 0; b < p.groups[(size_t)g].enc_blocks; b++, i++) {
                CHECK(i < t.enc[e].size() && t.enc[e][i].group == g && t.enc[e][i].block == b);
                if (i >= t.enc[e].size()) return;
            }
            enc_seen[(size_t)g]++;
            last_g = g;
        }
    }
    for (int d = 0; d < N_DEC; d++) {
        size_t i = 0;
        int last_g = -1;
        while (i < t.dec[d].size()) {
            const int g = t.dec[d][i].group;
            CHECK(g > last_g && g >= 0 && (size_t)g < ng);
            if (g < 0 || (size_t)g >= ng) return;
            CHECK(df[(size_t)g] == d);
            for (int b = 0; b < p.groups[(size_t)g].dec_blocks; b++, i++) {
                CHECK(i < t.dec[d].size() && t.dec[d][i].group == g && t.dec[d][i].block == b);
                if (i >= t.dec[d].size()) return;
            }
            dec_seen[(size_t)g]++;
            last_g = g;
        }
    }
    for (size_t g = 0; g < ng; g++) { CHECK(enc_seen[g] == 1); CHECK(dec_seen[g] == 1); }

    // all generic: the plan's own tables
    for (size_t g = 0; g < ng; g++) { ef[g] = ENC_GENERIC; df[g] = p.groups[g].cls; }
    CHECK(make_form_tables(p, ef.data(), df.data(), t));
    CHECK(t.enc[ENC_GENERIC].size() == p.enc_tab.size() && t.enc[ENC_FAST].empty() && t.enc[ENC_FAST_PRE].empty());
    for (size_t i = 0; i < p.enc_tab.size() && i < t.enc[0].size(); i++)
        CHECK(t.enc[0][i].group == p.enc_tab[i].group && t.enc[0][i].block == p.enc_tab[i].block);
    for (int c = 0; c < N_CLS; c++) {
        CHECK(t.dec[c].size() == p.dec_tab[c].size());
        for (size_t i = 0; i < p.dec_tab[c].size() && i < t.dec[c].size(); i++)
            CHECK(t.dec[c][i].group == p.dec_tab[c][i].group && t.dec[c][i].block == p.dec_tab[c][i].block);
    }
    for (int d = N_CLS; d < N_DEC; d++) CHECK(t.dec[d].empty());

    // refused: a form out of range, the generic form of another class
    if (ng) {
        const size_t g = rnd() % ng;
        df[g] = (p.groups[g].cls + 1) % N_CLS;
        CHECK(!make_form_tables(p, ef.data(), df.data(), t));
        df[g] = N_DEC;
        CHECK(!make_form_tables(p, ef.data(), df.data(), t));
        df[g] = p.groups[g].cls; ef[g] = -1;
        CHECK(!make_form_tables(p, ef.data(), df.data(), t));
        ef[g] = N_ENC;
        CHECK(!make_form_tables(p, ef.data(), df.data(), t));
    }
}

// ------------------------------------------------------------------------------------------------ the rule, restated
// Plane sizes for the sweep at W = 720: Rpad small enough for every head-switch range, for ranges 0 and 1 only, for 0 only,
// and for none (thresholds: span * Rpad * 4 < 0xFFF00000 with span = 720 | 793 | 1513).
static const int SW = 720;
static size_t rpad_limit(int hs_mode)      // the largest multiple of 64 that still passes
{
    const unsigned long long span = hs_mode == 0 ? 720ull : (hs_mode == 1 ? 720ull + 72 + 1 : 720ull + 792 + 1);
    unsigned long long r = (0xFFF00000ull - 1) / (span * 4);
    return (size_t)(r / 64 * 64);
}

static bool model_plane(size_t Rpad, int hs_mode)
{
    return Rpad <= rpad_limit(hs_mode);
}

static Forms model(const SetFacts &s, const CallFacts &c)
{
    Forms f;
    f.enc = ENC_GENERIC;
    f.dec = s.vhs ? (s.svideo ? DEC_GENERIC_VCR_SVIDEO : DEC_GENERIC_VCR_COMP) : DEC_GENERIC_TV;
    const bool switches = !c.force_generic && !c.no_fast;
    const int range = !s.hs ? 0 : (s.hs_small ? 1 : 2);       // the set's own head-switch range
    const int wrap_range = s.hs ? 2 : 0;                      // the forms whose loads wrap around
    // k_encode_fast / k_encode_fast_pre: input low-pass, luma noise, amplitude 50, even phases, aligned sources, plane
    const bool enc_ok = switches && s.in_lp && s.noise && s.amp == 50 && s.even_phase && c.src_al16 && model_plane(c.Rpad, range);
    if (enc_ok) f.enc = s.pre_on ? ENC_FAST_PRE : ENC_FAST;
    // every k_decode_fast*: colour, the lite output low-pass, amplitude 50, even phases, aligned destinations, plane
    const bool dec_ok = switches && !s.nocolor && s.out_lp == 1 && s.amp == 50 && s.even_phase && c.dst_al16 &&
                        model_plane(c.Rpad, range);
    const bool vhs_family = s.vhs && s.cnoise && s.pnoise, tv_family = !s.vhs && !s.cnoise && !s.pnoise;
    if (dec_ok && s.amp_back == 50) {
        if (vhs_family && !s.svideo) f.dec = s.hs_small ? DEC_FAST_VHS : DEC_FAST_VHS_WR;
        if (vhs_family && s.svideo && model_plane(c.Rpad, wrap_range)) f.dec = DEC_FAST_SV;
        if (tv_family && s.hs_small) f.dec = DEC_FAST_TV;
    }
    if (dec_ok && s.amp_back != 50 && s.amp_back >= 2) {
        if (vhs_family && !s.svideo && model_plane(c.Rpad, wrap_range)) f.dec = DEC_FAST_BK_VHS;
        if (tv_family && s.hs_small) f.dec = DEC_FAST_BK_TV;
    }
    return f;
}

static void sweep_rule()
{
    // the header's plane rule at its thresholds
    for (int m = 0; m < 3; m++) {
        CHECK(fast_plane_ok(rpad_limit(m), SW, m));
        CHECK(!fast_plane_ok(rpad_limit(m) + 64, SW, m));
    }
    CHECK(rpad_limit(0) > rpad_limit(1) && rpad_limit(1) > rpad_limit(2));
    const size_t rpads[5] = {128, rpad_limit(2), rpad_limit(1), rpad_limit(0), rpad_limit(0) + 64};
    const int amps[2] = {50, 30}, backs[4] = {50, 1, 2, 70}, outlps[3] = {0, 1, 2};
    for (unsigned bits = 0; bits < (1u << 11); bits++) {
        SetFacts s;
        s.in_lp = bits & 1; s.pre_on = bits & 2; s.noise = bits & 4; s.cnoise = bits & 8; s.pnoise = bits & 16;
        s.nocolor = bits & 32; s.even_phase = bits & 64; s.vhs = bits & 128; s.svideo = bits & 256; s.hs = bits & 512;
        s.hs_small = !s.hs || (bits & 1024);      // (no head switching: small by definition)
        if (!s.hs && (bits & 1024)) continue;
        for (int a : amps) for (int b : backs) for (int o : outlps) {
            s.amp = a; s.amp_back = b; s.out_lp = o;
            for (unsigned cb = 0; cb < 16; cb++) for (size_t rp : rpads) {
                CallFacts c;
                c.Rpad = rp; c.W = SW;
                c.src_al16 = cb & 1; c.dst_al16 = cb & 2; c.force_generic = cb & 4; c.no_fast = cb & 8;
                const Forms got = form_of(s, c), want = model(s, c);
                CHECK(got.enc == want.enc && got.dec == want.dec);
                // whatever the facts: a generic decoder form is the one of the set's class
                CHECK(got.dec >= N_CLS || got.dec == generic_dec_form(s));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ flips
struct Base { const char *name; SetFacts s; int enc, dec; };

static void flips()
{
    //                 in_lp pre    noise cn     pn     nocol  even  vhs    sv     hs     small amp back out_lp
    const Base bases[] = {
        {"default",   {true, false, true, false, false, false, true, false, false, false, true, 50, 50, 1}, ENC_FAST, DEC_FAST_TV},
        {"vhs",       {true, false, true, true,  true,  false, true, true,  false, true,  true, 50, 50, 1}, ENC_FAST, DEC_FAST_VHS},
        {"vhs_pal",   {true, false, true, true,  true,  false, true, true,  false, true,  false, 50, 50, 1}, ENC_FAST, DEC_FAST_VHS_WR},
        {"vhs_sv",    {true, false, true, true,  true,  false, true, true,  true,  true,  true, 50, 50, 1}, ENC_FAST, DEC_FAST_SV},
        {"catv",      {true, true,  true, false, false, false, true, false, false, false, true, 50, 70, 1}, ENC_FAST_PRE, DEC_FAST_BK_TV},
        {"catv_vhs",  {true, true,  true, true,  true,  false, true, true,  false, true,  true, 50, 70, 1}, ENC_FAST_PRE, DEC_FAST_BK_VHS},
    };
    for (const Base &b : bases) {
        CallFacts c;
        c.Rpad = 128; c.W = SW; c.src_al16 = c.dst_al16 = true; c.force_generic = c.no_fast = false;
        const int gen = generic_dec_form(b.s);
        Forms f = form_of(b.s, c);
        CHECK(f.enc == b.enc && f.dec == b.dec);
#define FLIP_CALL(stmt, want_enc, want_dec) \
        do { CallFacts k = c; stmt; const Forms r = form_of(b.s, k); CHECK(r.enc == (want_enc) && r.dec == (want_dec)); } while (0)
#define FLIP_SET(stmt, want_enc, want_dec) \
        do { SetFacts k = b.s; stmt; const Forms r = form_of(k, c); CHECK(r.enc == (want_enc) && r.dec == (want_dec)); } while (0)
        FLIP_CALL(k.src_al16 = false, ENC_GENERIC, b.dec);            // sources: the encoder only
        FLIP_CALL(k.dst_al16 = false, b.enc, gen);                    // destinations: the decoder only
        FLIP_CALL(k.force_generic = true, ENC_GENERIC, gen);
        FLIP_CALL(k.no_fast = true, ENC_GENERIC, gen);
        const int range = !b.s.hs ? 0 : (b.s.hs_small ? 1 : 2);
        // (the largest plane of the set's own range: the forms whose loads wrap around need the margin of range 2)
        FLIP_CALL(k.Rpad = rpad_limit(range), b.enc,
                  (b.dec == DEC_FAST_SV || b.dec == DEC_FAST_BK_VHS) && b.s.hs && range != 2 ? gen : b.dec);
        FLIP_CALL(k.Rpad = rpad_limit(range) + 64, ENC_GENERIC, gen); // the plane: both
        FLIP_SET(k.in_lp = false, ENC_GENERIC, b.dec);                // encoder-only switches
        FLIP_SET(k.noise = false, ENC_GENERIC, b.dec);
        FLIP_SET(k.pre_on = !k.pre_on, b.enc == ENC_FAST ? ENC_FAST_PRE : ENC_FAST, b.dec);
        FLIP_SET(k.amp = 30, ENC_GENERIC, gen);                       // both read the amplitude
        FLIP_SET(k.even_phase = false, ENC_GENERIC, gen);
        FLIP_SET(k.nocolor = true, b.enc, gen);                       // decoder-only switches
        FLIP_SET(k.out_lp = 2, b.enc, gen);
        FLIP_SET(k.out_lp = 0, b.enc, gen);
        FLIP_SET(k.amp_back = 1, b.enc, gen);
        FLIP_SET(k.cnoise = !k.cnoise, b.enc, gen);                   // half a chroma-noise family: no hand-tuned decoder
        FLIP_SET(k.pnoise = !k.pnoise, b.enc, gen);
#undef FLIP_CALL
#undef FLIP_SET
    }
}

int main()
{
    const int lslots[] = {1, 8, 62, 63, 64, 65, 243};
    for (int it = 0; it < 120; it++) {
        const int n = it < 4 ? it + 1 : 1 + (int)(rnd() % 600);
        check_tables(n, 1 + (int)(rnd() % 40), lslots[rnd() % 7]);
    }
    sweep_rule();
    flips();
    std::printf("mixed_forms: %lld checks, %lld bad\n", checks, bad);
    return bad ? 1 : 0;
}
