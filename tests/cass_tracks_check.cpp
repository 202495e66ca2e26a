// cass_tracks_check -- the multi-track plan of csrc/cass_chain.hpp on the host, as a stand-alone program
// (tests/test_cass_tracks_host.py builds it plain and with the address and undefined-behaviour sanitizers and runs it as
// the program it is).  Linked with csrc/glibc_rand.cpp for the rand() stream.
//
//   cass_tracks_check check  CFG IN L WF WB SPLIT RNGPOS TRACKS
//   cass_tracks_check expect CFG IN OUT STATES_OUT STATES_IN RNGPOS TRACKS
//
// CFG: as cass_chain_check's.  IN: raw interleaved s16le stereo, the tracks back to back.  TRACKS: FRAMES:COUNT[:n],...
// -- COUNT is the sample count of the track's first frame, n gives the track a NULL state (zeros, end state dropped).
//
// check: L, WF, WB are the plan (WF -1 / WB -1: the default warm-ups).  SPLIT 1: two calls, the first third of every
// track and then the rest, on the same states and with the counts advanced.  Asserted: cass_run_tracks_planned equals
// cass_run_serial (every tap) run per track from that track's state and count -- output bytes, the 28 filter values and
// the taps - 1 history frames bitwise, the count, the taps -- the per-track segments and repairs equal those of
// cass_run_planned on that track alone, cass_track_of_seg and cass_track_of_tile map every call-wide index to the (track,
// local index) a linear walk finds, the offsets and the length of cass_tilt_layout agree with a brute-force set of the
// counts, and an overflowing count + frames is reported.  Prints "tracks: <checks> checks, <bad> bad", the per-track
// stats of the last call, the rand() position and the sines evaluated.
//
// expect: cass_run_serial per track in order, the rand() position running through, from the states of STATES_IN (raw
// CassState per track, "-": zeros; their count and taps fields are not read).  Writes the outputs to OUT and the end
// states to STATES_OUT as the tracks call must leave them: count + frames and the taps where the track has frames, the
// state as it came where it has none.  A NULL-state track's entry is written as it came.  Prints the position.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
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
    bool null_state;
};

static bool parse_tracks(const char *p, std::vector<Track> &tracks, uint64_t &total)
{
    total = 0;
    while (*p) {
        char *e;
        Track t;
        t.frames = std::strtoull(p, &e, 10);
        if (*e != ':') return false;
        t.count = std::strtoull(e + 1, &e, 10);
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

static bool state_same(const CassCfg &c, const CassState &a, const CassState &b)
{
    return cass_front_same(a.front, b.front) && cass_back_same(a.back, b.back) && a.taps == b.taps &&
           cass_bits_same(&a.hist[0][0], &b.hist[0][0], (c.taps - 1) * 2);
}

static long checks = 0, bad = 0;
static void check(bool ok, const char *what, int t)
{
    checks++;
    if (!ok) {
        bad++;
        std::fprintf(stderr, "cass_tracks_check: %s, track %d\n", what, t);
    }
}

// the two lookups against a linear walk, the tilt layout against a brute-force set of counts
static void check_tables(const CassCfg &c, const std::vector<Track> &tracks, uint32_t L, int third)
{
    const int n = (int)tracks.size();
    std::vector<CassTrackEnt> tab((size_t)n);
    for (int t = 0; t < n; t++) {
        std::memset(&tab[(size_t)t], 0, sizeof(CassTrackEnt));
        tab[(size_t)t].frames = third ? tracks[(size_t)t].frames / 3 : tracks[(size_t)t].frames;
        tab[(size_t)t].count = tracks[(size_t)t].count;
    }
    const CassTracksTotals z = cass_tracks_layout(tab.data(), n, L, c.taps);
    uint64_t j = 0, i = 0, plane = 0, xs = 0;
    for (int t = 0; t < n; t++) {
        const CassTrackEnt &e = tab[(size_t)t];
        check(e.seg0 == j && e.tile0 == i && e.plane == plane && e.xs == xs, "layout", t);
        for (uint64_t jl = 0; jl < audio_seg_count(e.frames, L); jl++, j++) {
            const int f = cass_track_of_seg(tab.data(), n, j);
            check(f == t && j - tab[(size_t)f].seg0 == jl, "segment lookup", t);
        }
        for (uint64_t il = 0; il < (e.frames + CASS_TILE_FRAMES - 1) / CASS_TILE_FRAMES; il++, i++) {
            const int f = cass_track_of_tile(tab.data(), n, i);
            check(f == t && i - tab[(size_t)f].tile0 == il, "tile lookup", t);
        }
        plane += e.frames;
        xs += (uint64_t)(c.taps - 1) + e.frames;
    }
    check(j == z.segments && i == z.tiles && plane == z.frames && xs == z.xs_frames, "totals of the call", -1);

    std::vector<CassTiltRun> runs;
    uint64_t total = 0;
    check(cass_tilt_layout(tab.data(), n, runs, &total), "tilt layout refused", -1);
    std::set<uint64_t> counts;                                                  // brute force: every count some track covers
    for (int t = 0; t < n; t++)
        for (uint64_t f = 0; f < tab[(size_t)t].frames; f++) counts.insert(tab[(size_t)t].count + f);
    check(total == counts.size(), "union length", -1);
    std::vector<uint64_t> table;                                                // the count at every table entry
    for (const CassTiltRun &r : runs) {
        check(r.at == table.size(), "run offset", -1);
        for (uint64_t q = 0; q < r.n; q++) table.push_back(r.count0 + q);
    }
    check(table.size() == total && std::vector<uint64_t>(counts.begin(), counts.end()) == table, "runs are the sorted set", -1);
    for (int t = 0; t < n; t++) {
        const CassTrackEnt &e = tab[(size_t)t];
        bool ok = e.frames ? e.tilt + e.frames <= total : e.tilt == 0;
        for (uint64_t f = 0; ok && f < e.frames; f++) ok = table[(size_t)(e.tilt + f)] == e.count + f;
        check(ok, "tilt offset", t);
    }
    // the fill in parts equals the fill in one piece, wherever the parts are cut
    std::vector<double> whole((size_t)total + 1), parts((size_t)total + 1);
    cass_fill_tilt_part(c, runs.data(), runs.size(), 0, total, whole.data());
    const uint64_t cutp = total / 3;
    cass_fill_tilt_part(c, runs.data(), runs.size(), 0, cutp, parts.data());
    cass_fill_tilt_part(c, runs.data(), runs.size(), cutp, total - cutp, parts.data());
    check(cass_bits_same(whole.data(), parts.data(), (int)total), "fill in parts", -1);
    for (uint64_t q = 0; q < total; q += 97) {
        double one;
        cass_fill_tilt(c, table[(size_t)q], 1, &one);
        check(cass_bits_same(&one, &whole[(size_t)q], 1), "fill entry", -1);
    }
}

static void check_overflow(const CassCfg &c)
{
    CassTrackEnt tab[3];
    std::memset(tab, 0, sizeof(tab));
    tab[0].frames = 10;
    tab[1].frames = 2; tab[1].count = UINT64_MAX - 1;                           // count + frames = 2^64
    tab[2].frames = 5; tab[2].count = 3;
    std::vector<CassTiltRun> runs;
    uint64_t total = 0;
    check(!cass_tilt_layout(tab, 3, runs, &total), "overflow not reported", 1);
    tab[1].frames = 1;                                                          // the last count that exists
    check(cass_tilt_layout(tab, 3, runs, &total) && total == 11 && runs.size() == 2, "the last count refused", 1);
    tab[1].frames = 0; tab[1].count = UINT64_MAX;                               // a track without frames at any count
    check(cass_tilt_layout(tab, 3, runs, &total) && total == 10 && runs.size() == 1, "an empty track at the last count", 1);
    int16_t in[4] = {1, 2, 3, 4}, out[4];
    CassTrackIO io{in, out, nullptr, 2, UINT64_MAX - 1, nullptr};
    CassPlanStats ps;
    CassCfg nohiss = c;
    nohiss.hiss_level = 0;
    check(!cass_run_tracks_planned(nohiss, &io, 1, 64, 0, 0, &ps), "overflow not reported by the plan", 0);
}

static int run_check(const CassCfg &c, char **argv)
{
    const std::vector<int16_t> in = read_s16(argv[3]);
    const uint32_t L = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const long wf = std::strtol(argv[5], nullptr, 10), wb = std::strtol(argv[6], nullptr, 10);
    const uint32_t Wf = wf < 0 ? cass_default_front_warmup(c) : (uint32_t)wf, Wb = wb < 0 ? CASS_DEFAULT_BACK_WARMUP : (uint32_t)wb;
    const bool split = std::atoi(argv[7]) != 0;
    uint64_t pos = std::strtoull(argv[8], nullptr, 10);
    std::vector<Track> tracks;
    uint64_t total = 0;
    if (!parse_tracks(argv[9], tracks, total) || total * 2 != in.size()) {
        std::fprintf(stderr, "cass_tracks_check: %" PRIu64 " frames of tracks, %zu samples of input\n", total, in.size());
        return 2;
    }
    const int n = (int)tracks.size();
    const bool hiss_on = c.hiss_level != 0;
    check_tables(c, tracks, L ? L : 1, 0);
    check_tables(c, tracks, L ? L : 1, 1);
    check_overflow(c);

    std::vector<CassState> got((size_t)n), want((size_t)n), alone_state(1);
    for (int t = 0; t < n; t++) {
        std::memset(&got[(size_t)t], 0, sizeof(CassState));
        got[(size_t)t].front.count = 0xDEADBEEFu + (uint64_t)t;                 // what the state says of count and taps is not read
        got[(size_t)t].taps = 7777;
        std::memset(&want[(size_t)t], 0, sizeof(CassState));
    }
    std::vector<int16_t> wout(in.size() + 1, (int16_t)0x5555), gout(in.size() + 1, (int16_t)0x5555), alone(in.size() + 1);
    std::vector<CassPlanStats> last_stats;
    std::vector<char> touched((size_t)n, 0);                                    // the track has had frames in some call
    uint64_t tilt_frames = 0;
    for (int part = 0; part < (split ? 2 : 1); part++) {
        std::vector<CassTrackIO> io((size_t)n);
        std::vector<std::vector<int32_t>> hiss((size_t)n);
        std::vector<CassPlanStats> alone_stats((size_t)n);
        for (int t = 0; t < n; t++) {
            const Track &tr = tracks[(size_t)t];
            const uint64_t cut = tr.frames / 3;
            const uint64_t first = split && part == 1 ? cut : 0, frames = !split ? tr.frames : (part == 0 ? cut : tr.frames - cut);
            const size_t off = (size_t)(tr.at + first) * 2;
            const uint64_t count = tr.count + first;
            std::vector<double> tf((size_t)frames + 1);
            cass_fill_tilt(c, count, frames, tf.data());
            // the serial run of this track, every tap, drawing from the stream where the tracks before it left it
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
            check(!hiss_on || h.size() == (size_t)frames * 2, "draws", t);
            // the single-track plan on this track alone: what its repairs should be
            cass_run_planned(c, alone_state[0], in.data() + off, alone.data() + off, hiss_on ? h.data() : nullptr, tf.data(), frames, L, Wf, Wb,
                             &alone_stats[(size_t)t]);
            io[(size_t)t] = CassTrackIO{in.data() + off, gout.data() + off, hiss_on ? h.data() : nullptr, frames, count, tr.null_state ? nullptr : &got[(size_t)t]};
        }
        std::vector<CassPlanStats> stats((size_t)n);
        check(cass_run_tracks_planned(c, io.data(), n, L, Wf, Wb, stats.data(), &tilt_frames), "the plan refused the set", -1);
        for (int t = 0; t < n; t++) {
            const Track &tr = tracks[(size_t)t];
            if (io[(size_t)t].frames) touched[(size_t)t] = 1;
            if (!tr.null_state && touched[(size_t)t])
                check(state_same(c, got[(size_t)t], want[(size_t)t]), "state", t);
            else if (!tr.null_state)                                            // no frames so far: the state is as it came
                check(got[(size_t)t].front.count == 0xDEADBEEFu + (uint64_t)t && got[(size_t)t].taps == 7777, "a track without frames wrote its state", t);
            check(stats[(size_t)t].segments == audio_seg_count(io[(size_t)t].frames, L ? L : 1), "segments", t);
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
    std::printf("tracks: %ld checks, %ld bad\n", checks, bad);
    std::printf("stats");                                                       // of the last call
    for (const CassPlanStats &ps : last_stats) std::printf(" %" PRIu64 "/%" PRIu64 "/%" PRIu64, ps.segments, ps.repaired_front, ps.repaired_back);
    std::printf("\npos %" PRIu64 "\ntilt %" PRIu64 "\n", pos, tilt_frames);
    return bad ? 1 : 0;
}

static int run_expect(const CassCfg &c, char **argv)
{
    const std::vector<int16_t> in = read_s16(argv[3]);
    uint64_t pos = std::strtoull(argv[7], nullptr, 10);
    std::vector<Track> tracks;
    uint64_t total = 0;
    if (!parse_tracks(argv[8], tracks, total) || total * 2 != in.size()) {
        std::fprintf(stderr, "cass_tracks_check: %" PRIu64 " frames of tracks, %zu samples of input\n", total, in.size());
        return 2;
    }
    const size_t n = tracks.size();
    std::vector<CassState> states(n + 1), work(1);
    std::memset(states.data(), 0, (n + 1) * sizeof(CassState));
    if (std::strcmp(argv[6], "-")) {
        FILE *f = std::fopen(argv[6], "rb");
        if (!f) return 2;
        const size_t g = std::fread(states.data(), sizeof(CassState), n, f);
        std::fclose(f);
        if (g != n) return 2;
    }
    std::vector<int16_t> out(in.size() + 1);
    for (size_t t = 0; t < n; t++) {
        const Track &tr = tracks[t];
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
    FILE *f = std::fopen(argv[4], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 2, in.size(), f);
    std::fclose(f);
    f = std::fopen(argv[5], "wb");
    if (!f) return 2;
    std::fwrite(states.data(), sizeof(CassState), n, f);
    std::fclose(f);
    std::printf("pos %" PRIu64 "\n", pos);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    CassCfg c;
    if (!read_cfg(argv[2], c)) {
        std::fprintf(stderr, "cass_tracks_check: bad cfg %s\n", argv[2]);
        return 2;
    }
    if (mode == "check" && argc == 10) return run_check(c, argv);
    if (mode == "expect" && argc == 9) return run_expect(c, argv);
    return 2;
}
