// cass_chain_check -- csrc/cass_chain.hpp on the host, as a stand-alone program (tests/test_cass_*.py build it plain and
// with the address and undefined-behaviour sanitizers and run it as the program it is).  Linked with
// csrc/glibc_rand.cpp for the rand() stream.
//
//   cass_chain_check serial   CFG IN OUT COUNT0 RNGPOS BLOCK SINES   the chain, serially and with every tap, BLOCK frames per call (0:
//                                                                    one call; or blocks=FRAMES:POS,... with a rand() position per
//                                                                    block, a = as it stands); prints the final state
//   cass_chain_check planned  CFG IN COUNT0 RNGPOS NONSILENT SINES   plan + run + verify + repair for L x (Wf, Wb), over calls of
//                                                                    unequal length, against the serial run; prints "<n> bad"
//   cass_chain_check plan     CFG IN COUNT0 RNGPOS L WF WB SINES     one planned call; prints its segments, its repairs and
//                                                                    which segments each pass repaired
//   cass_chain_check converge CFG IN COUNT0 RNGPOS SINES            frames a zero-state run of the front and of the back needs to
//                                                                    meet the true states bit for bit; prints the worst of each
//   cass_chain_check sines    CFG COUNT0 N OUT                       this host's sin() of N frames from COUNT0, as doubles
//
// CFG: a text file, the fields of CassCfg in order, doubles as hexadecimal floats.  IN / OUT: raw interleaved s16le
// stereo.  SINES: a file of doubles, sin() of the frames from COUNT0 on as recorded from the tool, or "-": this host's.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// head_tilt_final of `frames` frames from count0: from recorded sines, or from this host's libm
static bool tilt_table(const CassCfg &c, const char *sines, uint64_t count0, uint64_t frames, std::vector<double> &tf)
{
    tf.resize((size_t)frames + 1);
    if (!std::strcmp(sines, "-")) {
        cass_fill_tilt(c, count0, frames, tf.data());
        return true;
    }
    FILE *f = std::fopen(sines, "rb");
    if (!f) return false;
    std::vector<double> s((size_t)frames + 1);
    const size_t got = std::fread(s.data(), 8, (size_t)frames, f);
    std::fclose(f);
    if (got != frames) return false;
    for (uint64_t i = 0; i < frames; i++) tf[(size_t)i] = cass_tilt_of_sin(c, s[(size_t)i]);
    return true;
}

static void print_state(const CassCfg &c, const CassState &st, uint64_t pos)
{
    std::printf("state");
    const auto hex = [](double v) {
        uint64_t u;
        std::memcpy(&u, &v, 8);
        std::printf(" %016" PRIx64, u);
    };
    for (int i = 0; i < CASS_FRONT_VALUES; i++) hex(st.front.v[i]);
    for (int i = 0; i < 2; i++) hex(st.back.post[i]);
    std::printf(" count %" PRIu64 " pos %" PRIu64 " taps %d hist", st.front.count, pos, c.taps);
    for (int k = 0; k < c.taps - 1; k++)
        for (int ch = 0; ch < 2; ch++) hex(st.hist[k][ch]);
    std::printf("\n");
}

static bool state_same(const CassCfg &c, const CassState &a, const CassState &b)
{
    return cass_front_same(a.front, b.front) && cass_back_same(a.back, b.back) && cass_bits_same(&a.hist[0][0], &b.hist[0][0], (c.taps - 1) * 2);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    CassCfg c;
    if (!read_cfg(argv[2], c)) {
        std::fprintf(stderr, "cass_chain_check: bad cfg %s\n", argv[2]);
        return 2;
    }
    if (mode == "sines" && argc == 6) {
        const uint64_t count0 = std::strtoull(argv[3], nullptr, 10), n = std::strtoull(argv[4], nullptr, 10);
        std::vector<double> s((size_t)n + 1);
        for (uint64_t i = 0; i < n; i++) s[(size_t)i] = std::sin(cass_sin_arg(c, count0 + i));
        FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 2;
        std::fwrite(s.data(), 8, (size_t)n, f);
        std::fclose(f);
        return 0;
    }
    if (mode == "serial" && argc == 9) {
        std::vector<int16_t> a = read_s16(argv[3]);
        a.resize(a.size() + 1);
        const uint64_t frames = (a.size() - 1) / 2;
        CassState *st = new CassState();
        std::memset(st, 0, sizeof(*st));
        st->taps = (uint32_t)c.taps;
        st->front.count = std::strtoull(argv[5], nullptr, 10);
        uint64_t pos = std::strtoull(argv[6], nullptr, 10);
        std::vector<double> tf;
        if (!tilt_table(c, argv[8], st->front.count, frames, tf)) return 2;
        RandSeq seq(rand_state_at(pos));
        const auto run = [&](uint64_t f, uint64_t n) {
            int16_t *q = a.data() + f * 2;
            cass_run_serial(c, *st, q, q, n, tf.data() + f, [&]() { pos++; return seq.next(); });
        };
        if (!std::strncmp(argv[7], "blocks=", 7)) {                             // FRAMES:POS,... -- POS "a": where the stream stands
            uint64_t f = 0;
            for (const char *p = argv[7] + 7; *p;) {
                char *e;
                const uint64_t n = std::strtoull(p, &e, 10);
                if (*e != ':' || f + n > frames) return 2;
                p = e + 1;
                if (*p == 'a') p++;
                else {
                    pos = std::strtoull(p, &e, 10);
                    seq = RandSeq(rand_state_at(pos));
                    p = e;
                }
                if (*p == ',') p++;
                run(f, n);
                f += n;
            }
            if (f != frames) return 2;
        } else {
            uint64_t block = std::strtoull(argv[7], nullptr, 10);
            if (block == 0) block = frames ? frames : 1;
            for (uint64_t f = 0; f < frames; f += block) run(f, frames - f < block ? frames - f : block);
        }
        FILE *f = std::fopen(argv[4], "wb");
        if (!f) return 2;
        std::fwrite(a.data(), 2, (size_t)frames * 2, f);
        std::fclose(f);
        print_state(c, *st, pos);
        delete st;
        return 0;
    }
    if (mode == "plan" && argc == 10) {                                         // one planned call: what the device's stats must say
        const std::vector<int16_t> in = read_s16(argv[3]);
        const uint64_t frames = in.size() / 2;
        std::vector<CassState> st(1);
        std::memset(&st[0], 0, sizeof(CassState));
        st[0].taps = (uint32_t)c.taps;
        st[0].front.count = std::strtoull(argv[4], nullptr, 10);
        std::vector<double> tf;
        if (!tilt_table(c, argv[9], st[0].front.count, frames, tf)) return 2;
        std::vector<int32_t> hiss;
        if (c.hiss_level != 0) {
            RandSeq seq(rand_state_at(std::strtoull(argv[5], nullptr, 10)));
            hiss.resize((size_t)frames * 2);
            for (int32_t &h : hiss) h = audio_hiss_num(seq.next(), c.hiss_level);
        }
        std::vector<int16_t> out(in.size() + 1);
        CassPlanStats ps;
        std::vector<uint64_t> which_front, which_back;
        cass_run_planned(c, st[0], in.data(), out.data(), hiss.empty() ? nullptr : hiss.data(), tf.data(), frames, (uint32_t)std::strtoul(argv[6], nullptr, 10),
                         (uint32_t)std::strtoul(argv[7], nullptr, 10), (uint32_t)std::strtoul(argv[8], nullptr, 10), &ps, &which_front, &which_back);
        std::printf("plan: segments %" PRIu64 " front %" PRIu64 " back %" PRIu64 " which_front", ps.segments, ps.repaired_front, ps.repaired_back);
        for (uint64_t j : which_front) std::printf(" %" PRIu64, j);
        std::printf(" which_back");
        for (uint64_t j : which_back) std::printf(" %" PRIu64, j);
        std::printf("\n");
        return 0;
    }
    if ((mode == "planned" && argc == 8) || (mode == "converge" && argc == 7)) {
        const std::vector<int16_t> in = read_s16(argv[3]);
        const uint64_t frames = in.size() / 2;
        std::vector<CassState> states(3);
        CassState &st0 = states[0], &ws = states[1], &st = states[2];
        std::memset(&st0, 0, sizeof(st0));
        st0.taps = (uint32_t)c.taps;
        st0.front.count = std::strtoull(argv[4], nullptr, 10);
        const uint64_t pos0 = std::strtoull(argv[5], nullptr, 10);
        std::vector<double> tf;
        if (!tilt_table(c, argv[mode == "planned" ? 7 : 6], st0.front.count, frames, tf)) return 2;
        std::vector<int32_t> hiss;                                              // numerators of the whole input
        if (c.hiss_level != 0) {
            RandSeq seq(rand_state_at(pos0));
            hiss.resize((size_t)frames * 2);
            for (int32_t &h : hiss) h = audio_hiss_num(seq.next(), c.hiss_level);
        }
        const int32_t *hp = hiss.empty() ? nullptr : hiss.data();
        if (mode == "planned") {
            const bool nonsilent = std::atoi(argv[6]) != 0;
            std::vector<int16_t> want(in.size() + 1), got(in.size() + 1);
            ws = st0;                                                           // the serial run, every tap
            {
                RandSeq seq(rand_state_at(pos0));                               // the serial run draws for itself, from the same position
                cass_run_serial(c, ws, in.data(), want.data(), frames, tf.data(), [&]() { return seq.next(); });
            }
            long bad = 0, runs = 0;
            const uint32_t Ls[6] = {1, 2, 63, 64, 65, 1000};
            const uint32_t Wf[4] = {0, 1, 64, cass_default_front_warmup(c)}, Wb[4] = {0, 64, 1, CASS_DEFAULT_BACK_WARMUP};
            // calls of unequal length: none, one frame, 777 frames, 64 frames, the rest; with many taps the history spans them
            const uint64_t cuts[4] = {0, 1, 777, 64};
            for (uint32_t L : Ls)
                for (int w = 0; w < 4; w++) {
                    std::fill(got.begin(), got.end(), (int16_t)0x5555);
                    st = st0;
                    uint64_t at = 0;
                    for (int k = 0; k < 5; k++) {
                        const uint64_t n = k < 4 ? (cuts[k] < frames - at ? cuts[k] : frames - at) : frames - at;
                        CassPlanStats ps;
                        cass_run_planned(c, st, in.data() + at * 2, got.data() + at * 2, hp ? hp + at * 2 : nullptr, tf.data() + at, n, L, Wf[w], Wb[w], &ps);
                        if (ps.segments != audio_seg_count(n, L)) bad++;
                        // W = 0 on input that is not silent: only the segments that start from the carried state pass
                        if (Wf[w] == 0 && nonsilent && n > 0 && ps.repaired_front != ps.segments - 1) bad++;
                        // the back as well, but for the stream's first frames, which may still be silent behind the FIR's delay
                        if (Wb[w] == 0 && c.post && nonsilent && n > 0 && ps.repaired_back + (uint64_t)c.taps < ps.segments - 1) bad++;
                        if (!c.post && ps.repaired_back != 0) bad++;
                        at += n;
                    }
                    if (std::memcmp(got.data(), want.data(), in.size() * 2) != 0) bad++;
                    if (!state_same(c, st, ws)) bad++;
                    runs++;
                }
            std::printf("planned: %ld runs, %ld bad\n", runs, bad);
            print_state(c, ws, pos0 + hiss.size());
            return bad ? 1 : 0;
        }
        // converge: the true states in front of every frame, then zero-state runs from 24 start points
        std::vector<CassFront> tfront((size_t)frames + 1);
        std::vector<CassBack> tback((size_t)frames + 1);
        std::vector<double> xs, rs((size_t)frames * 2 + 2);
        cass_plane_begin(c, st0, xs, frames);
        {
            CassFront s = st0.front;
            for (uint64_t f = 0; f < frames; f++) {
                tfront[(size_t)f] = s;
                cass_front_span(c, s, in.data(), xs.data(), hp, f, 1);
            }
            tfront[(size_t)frames] = s;
            cass_conv_span<false>(c, xs.data(), tf.data(), rs.data(), 0, frames);
            CassBack b = st0.back;
            for (uint64_t f = 0; f < frames; f++) {
                tback[(size_t)f] = b;
                cass_back_span(c, b, rs.data(), nullptr, f, 1);
            }
            tback[(size_t)frames] = b;
        }
        const uint32_t W = cass_default_front_warmup(c);
        uint64_t worst = 0, worst_back = 0;
        long unmet = 0, started = 0, unmet_back = 0, started_back = 0;
        for (int k = 0; k < 24; k++) {
            const uint64_t p = 1 + (frames - 1) * (uint64_t)k / 24;
            if (p + W <= frames) {                                              // else: too little input behind it to tell
                CassFront s = cass_front_spec(c, st0.front, p);
                uint64_t f = p;
                while (f < frames && !cass_front_same(s, tfront[(size_t)f])) {
                    cass_front_span(c, s, in.data(), nullptr, hp, f, 1);
                    f++;
                }
                started++;
                if (!cass_front_same(s, tfront[(size_t)f])) unmet++;
                else if (f - p > worst) worst = f - p;
            }
            if (c.post && p + 4 * CASS_DEFAULT_BACK_WARMUP <= frames) {
                CassBack s;
                s.post[0] = s.post[1] = 0;
                uint64_t f = p;
                while (f < frames && !cass_back_same(s, tback[(size_t)f])) {
                    cass_back_span(c, s, rs.data(), nullptr, f, 1);
                    f++;
                }
                started_back++;
                if (!cass_back_same(s, tback[(size_t)f])) unmet_back++;
                else if (f - p > worst_back) worst_back = f - p;
            }
        }
        std::printf("converge: front %ld starts, %ld unmet, worst %" PRIu64 " default_warmup %u; back %ld starts, %ld unmet, worst %" PRIu64
                    " measured %u default_warmup %u\n",
                    started, unmet, worst, W, started_back, unmet_back, worst_back, CASS_BACK_MEASURED, CASS_DEFAULT_BACK_WARMUP);
        return (unmet || unmet_back || worst > W || worst_back > CASS_BACK_MEASURED || started == 0 || (c.post && started_back == 0)) ? 1 : 0;
    }
    return 2;
}
