// cass_mixed_tracks_check -- the mixed tracks plan of csrc/cass_chain.hpp (parameters per track) on the host, as a
// stand-alone program (tests/test_cass_mixed_tracks_host.py builds it plain and with the address and undefined-behaviour
// sanitizers and runs it as the program it is).  Linked with csrc/glibc_rand.cpp for the rand() stream.
//
//   cass_mixed_tracks_check check  NSETS CFG.. IN L WF WB SPLIT RNGPOS TRACKS
//   cass_mixed_tracks_check expect NSETS CFG.. IN OUT STATES_OUT STATES_IN RNGPOS TRACKS
//   cass_mixed_tracks_check sines  NSETS CFG.. TRACKS
//
// CFG: as cass_chain_check's, one file per set of the caller's `sets` array.  IN: raw interleaved s16le stereo, the tracks
// back to back.  TRACKS: FRAMES:COUNT:SET[:n],... -- COUNT is the sample count of the track's first frame, SET its index
// among the CFGs, n gives the track a NULL state (zeros, end state dropped).
//
// check: L, WF, WB are the plan (WF -1: every track's own default warm-up; WB -1: the default).  SPLIT 1: two calls, the
// first third of every track and then the rest, on the same states -- which then start with a history in all
// CASS_HIST entries, so that every track carries one of its own length and has a rest that must stay -- and with the
// counts advanced; SPLIT 0: one call from zero states, as a fresh device buffer is.  Asserted: the set table
// holds the sets in order of first use; cass_mixed_layout equals a linear walk with every track's own taps and warm-up;
// the two lookups; the table of sines is one union per distinct rate, its entries are the sines themselves and
// cass_tilt_of_sin of them is cass_fill_tilt's head_tilt_final bit for bit; cass_run_mixed_tracks_planned equals
// cass_run_serial (every tap) run per track with that track's cfg, state and count -- output bytes, the 28 filter
// values, the WHOLE history array (the track's taps - 1 frames and the rest, which stays), the count, the taps -- and the
// per-track segments and repairs equal those of cass_run_planned on that track alone with its own warm-up.  Prints
// "mixed: <checks> checks, <bad> bad", the per-track stats of the last call, the rand() position and the sines evaluated.
//
// expect: cass_run_serial per track in order with that track's cfg, the rand() position running through, from the
// states of STATES_IN (raw CassState per track, "-": zeros; their count and taps fields are not read).  Writes the outputs
// to OUT and the end states to STATES_OUT as the mixed call must leave them.  Prints the position.
//
// sines: the layout of the table alone (no input): prints "tilt <entries>" and "runs <n>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "cass_chain.hpp"
#include "glibc_rand.hpp"

using namespace ntscsim;

static bool read_cfg(const char *path, CassCfg &c)
{
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    char d[8][64];
    int iv[5];
    bool ok = true;
    for (int i = 0; i < 5; i++) ok = ok && std::fscanf(f, "%d", &iv[i]) == 1;
    for (int i = 0; i < 8; i++) ok = ok && std::fscanf(f, "%63s", d[i]) == 1;
    std::fclose(f);
    if (!ok) return false;
    std::memset(&c, 0, sizeof(c));
    c.pre = iv[0]; c.post = iv[1]; c.mono = iv[2]; c.hiss_level = iv[3]; c.taps = iv[4];
    double *dv[8] = {&c.rate, &c.highpass_hz, &c.tilt, &c.waver, &c.a_lo, &c.a_hi, &c.a_pre, &c.a_post};
    for (int i = 0; i < 8; i++) *dv[i] = std::strtod(d[i], nullptr);
    return c.taps >= 1 && c.taps <= CASS_MAX_TAPS;
}

static std::vector<int16_t> read_s16(const char *path)
{
    std::vector<int16_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    int16_t buf[4096];
    for (size_t g; (g = std::fread(buf, 2, 4096, f)) > 0;) v.insert(v.end(), buf, buf + g);
    std::fclose(f);
    return v;
}

struct Track {
    uint64_t frames, at, count;          // at: first frame in IN
    int set;
    bool null_state;
};

static bool parse_tracks(const char *p, int nsets, std::vector<Track> &tracks, uint64_t &total)
{
    total = 0;
    while (*p) {
        char *e;
        Track t;
        t.frames = std::strtoull(p, &e, 10);
        if (*e != ':') return false;
        t.count = std::strtoull(e + 1, &e, 10);
        if (*e != ':') return false;
        t.set = (int)std::strtol(e + 1, &e, 10);
        if (t.set < 0 || t.set >= nsets) return false;
        t.null_state = false;
        if (e[0] == ':' && e[1] == 'n') { t.null_state = true; e += 2; }
        t.at = total;
        total += t.frames;
        tracks.push_back(t);
        if (*e == ',') e++;
        else if (*e) return false;
        p = e;
    }
    return true;
}

static bool state_same(const CassState &a, const CassState &b)
{
    return cass_front_same(a.front, b.front) && cass_back_same(a.back, b.back) && a.taps == b.taps &&
           cass_bits_same(&a.hist[0][0], &b.hist[0][0], CASS_HIST * 2);
}

static long checks = 0, bad = 0;
static void check(bool ok, const char *what, int t)
{
    checks++;
    if (!ok) {
        bad++;
        std::fprintf(stderr, "cass_mixed_tracks_check: %s, track %d\n", what, t);
    }
}

// the caller's sets -> the set table; tab[t].set filled in
static void make_table(const std::vector<CassCfg> &sets, const std::vector<Track> &tracks, std::vector<CassCfg> &table, std::vector<int32_t> &cfg_of)
{
    std::vector<int32_t> set_of, order;
    for (const Track &t : tracks) set_of.push_back(t.set);
    cass_mixed_set_table(set_of.data(), (int)tracks.size(), (int)sets.size(), order, cfg_of);
    table.clear();
    for (int32_t s : order) table.push_back(sets[(size_t)s]);
    // order of first use, by a linear walk
    std::vector<int32_t> seen;
    for (size_t t = 0; t < tracks.size(); t++) {
        size_t at = 0;
        while (at < seen.size() && seen[at] != tracks[t].set) at++;
        if (at == seen.size()) seen.push_back(tracks[t].set);
        check(cfg_of[t] == (int32_t)at, "set table place", (int)t);
    }
    check(seen == order, "set table order", -1);
}

static std::vector<CassMixedEnt> make_tab(const std::vector<Track> &tracks, const std::vector<int32_t> &cfg_of, int third)
{
    std::vector<CassMixedEnt> tab(tracks.size());
    for (size_t t = 0; t < tracks.size(); t++) {
        std::memset(&tab[t], 0, sizeof(CassMixedEnt));
        tab[t].frames = third ? tracks[t].frames / 3 : tracks[t].frames;
        tab[t].count = tracks[t].count;
        tab[t].set = cfg_of[t];
    }
    return tab;
}

// the layout and the lookups against a linear walk, the table of sines against brute-force sets of counts per rate
static uint64_t check_tables(const std::vector<CassCfg> &table, const std::vector<Track> &tracks, const std::vector<int32_t> &cfg_of, uint32_t L,
                             const uint32_t *warm_all, int third, size_t *nruns = nullptr)
{
    const int n = (int)tracks.size();
    std::vector<CassMixedEnt> tab = make_tab(tracks, cfg_of, third);
    const CassTracksTotals z = cass_mixed_layout(tab.data(), n, table.data(), L, warm_all);
    uint64_t j = 0, i = 0, plane = 0, xs = 0;
    for (int t = 0; t < n; t++) {
        const CassMixedEnt &e = tab[(size_t)t];
        const CassCfg &c = table[(size_t)e.set];
        check(e.seg0 == j && e.tile0 == i && e.plane == plane && e.xs == xs, "layout", t);
        check(e.warm == (warm_all ? *warm_all : cass_default_front_warmup(c)), "warm-up", t);
        for (uint64_t jl = 0; jl < audio_seg_count(e.frames, L); jl++, j++) {
            const int f = cass_track_of_seg(tab.data(), n, j);
            check(f == t && j - tab[(size_t)f].seg0 == jl, "segment lookup", t);
        }
        for (uint64_t il = 0; il < (e.frames + CASS_TILE_FRAMES - 1) / CASS_TILE_FRAMES; il++, i++) {
            const int f = cass_track_of_tile(tab.data(), n, i);
            check(f == t && i - tab[(size_t)f].tile0 == il, "tile lookup", t);
        }
        plane += e.frames;
        xs += (uint64_t)(c.taps - 1) + e.frames;                                // the track's own taps
    }
    check(j == z.segments && i == z.tiles && plane == z.frames && xs == z.xs_frames, "totals of the call", -1);

    std::vector<CassSineRun> runs;
    uint64_t total = 0;
    check(cass_sine_layout(tab.data(), n, table.data(), runs, &total), "sine layout refused", -1);
    if (nruns) *nruns = runs.size();
    std::vector<double> rates;                                                  // brute force: per rate, in order of first use, every count covered
    std::vector<std::set<uint64_t>> counts;
    for (int t = 0; t < n; t++) {
        if (!tab[(size_t)t].frames) continue;
        const double r = table[(size_t)tab[(size_t)t].set].rate;
        size_t at = 0;
        while (at < rates.size() && rates[at] != r) at++;
        if (at == rates.size()) { rates.push_back(r); counts.emplace_back(); }
        for (uint64_t f = 0; f < tab[(size_t)t].frames; f++) counts[at].insert(tab[(size_t)t].count + f);
    }
    std::vector<std::pair<double, uint64_t>> want;                              // (rate, count) at every table entry
    for (size_t r = 0; r < rates.size(); r++)
        for (uint64_t cnt : counts[r]) want.push_back({rates[r], cnt});
    check(total == want.size(), "union length", -1);
    std::vector<std::pair<double, uint64_t>> table_of;
    for (const CassSineRun &r : runs) {
        check(r.at == table_of.size(), "run offset", -1);
        for (uint64_t q = 0; q < r.n; q++) table_of.push_back({r.rate, r.count0 + q});
    }
    check(table_of == want, "runs are the sorted sets, rate by rate", -1);
    std::vector<double> whole((size_t)total + 1), parts((size_t)total + 1);
    cass_fill_sines_part(runs.data(), runs.size(), 0, total, whole.data());
    const uint64_t cutp = total / 3;
    cass_fill_sines_part(runs.data(), runs.size(), 0, cutp, parts.data());
    cass_fill_sines_part(runs.data(), runs.size(), cutp, total - cutp, parts.data());
    check(cass_bits_same(whole.data(), parts.data(), (int)total), "fill in parts", -1);
    for (int t = 0; t < n; t++) {
        const CassMixedEnt &e = tab[(size_t)t];
        const CassCfg &c = table[(size_t)e.set];
        bool ok = e.frames ? e.tilt + e.frames <= total : e.tilt == 0;
        for (uint64_t f = 0; ok && f < e.frames; f++) ok = table_of[(size_t)(e.tilt + f)] == std::make_pair(c.rate, e.count + f);
        check(ok, "sine offset", t);
        // the entries are the sines themselves; head_tilt_final made from them is cass_fill_tilt's
        bool same = true;
        for (uint64_t f = 0; ok && same && f < e.frames; f += (f < 64 ? 1 : 37)) {
            const double s = std::sin(cass_sin_arg(c, e.count + f)), tf_here = cass_tilt_of_sin(c, whole[(size_t)(e.tilt + f)]);
            double tf;
            cass_fill_tilt(c, e.count + f, 1, &tf);
            same = cass_bits_same(&s, &whole[(size_t)(e.tilt + f)], 1) && cass_bits_same(&tf, &tf_here, 1);
        }
        check(same, "sines and the tilt made from them", t);
    }
    return total;
}

static void check_overflow(const CassCfg &c)
{
    CassMixedEnt tab[3];
    std::memset(tab, 0, sizeof(tab));
    tab[0].frames = 10;
    tab[1].frames = 2; tab[1].count = UINT64_MAX - 1;                           // count + frames = 2^64
    tab[2].frames = 5; tab[2].count = 3;
    std::vector<CassSineRun> runs;
    uint64_t total = 0;
    check(!cass_sine_layout(tab, 3, &c, runs, &total), "overflow not reported", 1);
    tab[1].frames = 1;                                                          // the last count that exists
    check(cass_sine_layout(tab, 3, &c, runs, &total) && total == 11 && runs.size() == 2, "the last count refused", 1);
}

struct Args {
    std::vector<CassCfg> sets;
    char **rest;
    int nrest;
};

static int run_check(const Args &a)
{
    char **argv = a.rest;
    const std::vector<int16_t> in = read_s16(argv[0]);
    uint32_t L = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    const long wf = std::strtol(argv[2], nullptr, 10), wb = std::strtol(argv[3], nullptr, 10);
    const uint32_t wf_all = wf < 0 ? 0 : (uint32_t)wf, Wb = wb < 0 ? CASS_DEFAULT_BACK_WARMUP : (uint32_t)wb;
    const uint32_t *warm_all = wf < 0 ? nullptr : &wf_all;
    const bool split = std::atoi(argv[4]) != 0;
    uint64_t pos = std::strtoull(argv[5], nullptr, 10);
    std::vector<Track> tracks;
    uint64_t total = 0;
    if (!parse_tracks(argv[6], (int)a.sets.size(), tracks, total) || total * 2 != in.size()) {
        std::fprintf(stderr, "cass_mixed_tracks_check: %" PRIu64 " frames of tracks, %zu samples of input\n", total, in.size());
        return 2;
    }
    const int n = (int)tracks.size();
    std::vector<CassCfg> table;
    std::vector<int32_t> cfg_of;
    make_table(a.sets, tracks, table, cfg_of);
    check_tables(table, tracks, cfg_of, L ? L : 1, warm_all, 0);
    check_tables(table, tracks, cfg_of, L ? L : 1, warm_all, 1);
    check_overflow(a.sets[0]);

    std::vector<CassState> got((size_t)n), want((size_t)n), alone_state(1);
    for (int t = 0; t < n; t++) {
        std::memset(&got[(size_t)t], 0, sizeof(CassState));
        for (int k = 0; split && k < CASS_HIST; k++)                            // a carried history, and a rest that must stay
            for (int ch = 0; ch < CASS_CHANNELS; ch++) got[(size_t)t].hist[k][ch] = (double)((k * 7 + ch * 3 + t) % 23 - 11) / 16;
        want[(size_t)t] = got[(size_t)t];
        got[(size_t)t].front.count = 0xDEADBEEFu + (uint64_t)t;                 // what the state says of count and taps is not read
        got[(size_t)t].taps = 7777;
    }
    std::vector<int16_t> wout(in.size() + 1, (int16_t)0x5555), gout(in.size() + 1, (int16_t)0x5555), alone(in.size() + 1);
    std::vector<CassPlanStats> last_stats;
    std::vector<char> touched((size_t)n, 0);
    uint64_t tilt_frames = 0;
    for (int part = 0; part < (split ? 2 : 1); part++) {
        std::vector<CassMixedIO> io((size_t)n);
        std::vector<std::vector<int32_t>> hiss((size_t)n);
        std::vector<CassPlanStats> alone_stats((size_t)n);
        for (int t = 0; t < n; t++) {
            const Track &tr = tracks[(size_t)t];
            const CassCfg &c = a.sets[(size_t)tr.set];
            const bool hiss_on = c.hiss_level != 0;
            const uint64_t cut = tr.frames / 3;
            const uint64_t first = split && part == 1 ? cut : 0, frames = !split ? tr.frames : (part == 0 ? cut : tr.frames - cut);
            const size_t off = (size_t)(tr.at + first) * 2;
            const uint64_t count = tr.count + first;
            std::vector<double> tf((size_t)frames + 1);
            cass_fill_tilt(c, count, frames, tf.data());
            RandSeq seq(rand_state_at(pos));
            std::vector<int32_t> &h = hiss[(size_t)t];
            CassState &ws = want[(size_t)t];
            if (tr.null_state) std::memset(&ws, 0, sizeof(ws));
            ws.front.count = count;
            alone_state[0] = ws;
            cass_run_serial(c, ws, in.data() + off, wout.data() + off, frames, tf.data(), [&]() {
                const uint32_t r = seq.next();
                h.push_back(audio_hiss_num(r, c.hiss_level));
                pos++;
                return r;
            });
            if (frames) ws.taps = (uint32_t)c.taps;
            check(h.size() == (hiss_on ? (size_t)frames * 2 : 0), "draws", t);
            cass_run_planned(c, alone_state[0], in.data() + off, alone.data() + off, hiss_on ? h.data() : nullptr, tf.data(), frames, L,
                             warm_all ? *warm_all : cass_default_front_warmup(c), Wb, &alone_stats[(size_t)t]);
            if (!c.post) alone_stats[(size_t)t].repaired_back = 0;
            io[(size_t)t].io = CassTrackIO{in.data() + off, gout.data() + off, hiss_on ? h.data() : nullptr, frames, count, tr.null_state ? nullptr : &got[(size_t)t]};
            io[(size_t)t].set = cfg_of[(size_t)t];
        }
        std::vector<CassPlanStats> stats((size_t)n);
        check(cass_run_mixed_tracks_planned(table.data(), io.data(), n, L, warm_all, Wb, stats.data(), &tilt_frames), "the plan refused the set", -1);
        for (int t = 0; t < n; t++) {
            const Track &tr = tracks[(size_t)t];
            if (io[(size_t)t].io.frames) touched[(size_t)t] = 1;
            if (!tr.null_state && touched[(size_t)t])
                check(state_same(got[(size_t)t], want[(size_t)t]), "state", t);
            else if (!tr.null_state)
                check(got[(size_t)t].front.count == 0xDEADBEEFu + (uint64_t)t && got[(size_t)t].taps == 7777, "a track without frames wrote its state", t);
            check(stats[(size_t)t].segments == audio_seg_count(io[(size_t)t].io.frames, L ? L : 1), "segments", t);
            check(stats[(size_t)t].segments == alone_stats[(size_t)t].segments && stats[(size_t)t].repaired_front == alone_stats[(size_t)t].repaired_front &&
                      stats[(size_t)t].repaired_back == alone_stats[(size_t)t].repaired_back,
                  "repairs", t);
        }
        last_stats = stats;
    }
    for (int t = 0; t < n; t++) {
        const Track &tr = tracks[(size_t)t];
        check(std::memcmp(gout.data() + tr.at * 2, wout.data() + tr.at * 2, (size_t)tr.frames * 4) == 0, "bytes", t);
    }
    check(gout.back() == (int16_t)0x5555, "the sample behind the input", -1);
    std::printf("mixed: %ld checks, %ld bad\n", checks, bad);
    std::printf("stats");
    for (const CassPlanStats &ps : last_stats) std::printf(" %" PRIu64 "/%" PRIu64 "/%" PRIu64, ps.segments, ps.repaired_front, ps.repaired_back);
    std::printf("\npos %" PRIu64 "\ntilt %" PRIu64 "\n", pos, tilt_frames);
    return bad ? 1 : 0;
}

static int run_expect(const Args &a)
{
    char **argv = a.rest;
    const std::vector<int16_t> in = read_s16(argv[0]);
    uint64_t pos = std::strtoull(argv[4], nullptr, 10);
    std::vector<Track> tracks;
    uint64_t total = 0;
    if (!parse_tracks(argv[5], (int)a.sets.size(), tracks, total) || total * 2 != in.size()) {
        std::fprintf(stderr, "cass_mixed_tracks_check: %" PRIu64 " frames of tracks, %zu samples of input\n", total, in.size());
        return 2;
    }
    const size_t n = tracks.size();
    std::vector<CassState> states(n + 1), work(1);
    std::memset(states.data(), 0, (n + 1) * sizeof(CassState));
    if (std::strcmp(argv[3], "-")) {
        FILE *f = std::fopen(argv[3], "rb");
        if (!f) return 2;
        const size_t g = std::fread(states.data(), sizeof(CassState), n, f);
        std::fclose(f);
        if (g != n) return 2;
    }
    std::vector<int16_t> out(in.size() + 1);
    for (size_t t = 0; t < n; t++) {
        const Track &tr = tracks[t];
        const CassCfg &c = a.sets[(size_t)tr.set];
        if (tr.frames == 0) continue;                                           // its state stays as it came
        CassState &st = work[0];
        if (tr.null_state) std::memset(&st, 0, sizeof(st));
        else st = states[t];
        st.front.count = tr.count;
        std::vector<double> tf((size_t)tr.frames + 1);
        cass_fill_tilt(c, tr.count, tr.frames, tf.data());
        RandSeq seq(rand_state_at(pos));
        cass_run_serial(c, st, in.data() + tr.at * 2, out.data() + tr.at * 2, tr.frames, tf.data(), [&]() { pos++; return seq.next(); });
        st.taps = (uint32_t)c.taps;
        if (!tr.null_state) states[t] = st;
    }
    FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 2, in.size(), f);
    std::fclose(f);
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(states.data(), sizeof(CassState), n, f);
    std::fclose(f);
    std::printf("pos %" PRIu64 "\n", pos);
    return 0;
}

static int run_sines(const Args &a)
{
    std::vector<Track> tracks;
    uint64_t total = 0;
    if (!parse_tracks(a.rest[0], (int)a.sets.size(), tracks, total)) return 2;
    std::vector<CassCfg> table;
    std::vector<int32_t> cfg_of;
    make_table(a.sets, tracks, table, cfg_of);
    size_t nruns = 0;
    const uint64_t entries = check_tables(table, tracks, cfg_of, 64, nullptr, 0, &nruns);
    std::printf("mixed: %ld checks, %ld bad\ntilt %" PRIu64 "\nruns %zu\n", checks, bad, entries, nruns);
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::string mode = argv[1];
    const int nsets = std::atoi(argv[2]);
    if (nsets < 1 || argc < 3 + nsets) return 2;
    Args a;
    for (int s = 0; s < nsets; s++) {
        CassCfg c;
        if (!read_cfg(argv[3 + s], c)) {
            std::fprintf(stderr, "cass_mixed_tracks_check: bad cfg %s\n", argv[3 + s]);
            return 2;
        }
        a.sets.push_back(c);
    }
    a.rest = argv + 3 + nsets;
    a.nrest = argc - 3 - nsets;
    if (mode == "check" && a.nrest == 7) return run_check(a);
    if (mode == "expect" && a.nrest == 6) return run_expect(a);
    if (mode == "sines" && a.nrest == 1) return run_sines(a);
    return 2;
}
