// Host check of csrc/ntsc_rowstate_lookback.hpp (built and run by tests/test_rowstate_lookback_host.py with plain g++, and
// again with -fsanitize=address,undefined): the noise accumulators k_row_states derives at a row's first draw from the
// rand() window there, against the serial replay from the stream's first draw.
//
// For K in {1, 4, 16, 100}, every row stride 8 ... 720 (chroma: the even ones), rows 0 ... 3 of the stream, streams that
// begin at three positions of rand() (0, a small one, one beyond 2^32 / 2), luma and chroma:
//   * the window path (the default look-back, straight from the window's words, extended where it has not settled)
//     wherever the kernel may take it -- no draw or at least the look-back's length behind the row;
//   * the ring path (back and forward through the lane's ring) at the default look-back, at the test hook's 2 / 2 and at a
//     look-back longer than the window;
//   each must give the serial replay's accumulators and leave the ring holding the row's window again.
// Seeded windows come from csrc/glibc_rand.cpp.  The extensions that ran are counted and printed; the hook's lengths
// must have driven most rows with draws behind them through one.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "glibc_rand.hpp"
#include "ntsc_rowstate_lookback.hpp"

using namespace ntscsim;
using namespace ntscsim::rowstate;

static long bad = 0, checked = 0;

#define CHECK(cond, ...)                                                                         \
    do {                                                                                         \
        checked++;                                                                               \
        if (!(cond)) {                                                                           \
            if (bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); }      \
        }                                                                                        \
    } while (0)

static const int MAXSTART = 3 * 720;       // draws behind the last row swept

// words[p + j], j = 0 ... 30: the window at the stream's draw p; the draw itself is words[p + 31] >> 1
static std::vector<uint32_t> stream_words(uint64_t pos0)
{
    const RandState s = rand_state_at(pos0);
    std::vector<uint32_t> w(31 + MAXSTART + 1);
    for (int j = 0; j < 31; j++) w[j] = s.w[j];
    for (size_t i = 31; i < w.size(); i++) w[i] = w[i - 31] + w[i - 3];
    return w;
}

struct Counts { long rows = 0, extended = 0, rounds = 0; };

static void check_ring_restored(const uint32_t *col, const Ring &r, const uint32_t (&st)[31], const char *what, long long start)
{
    bool same = r.slot == 0;
    for (int j = 0; j < 31 && same; j++) same = col[j * 3] == st[j];
    CHECK(same, "%s: ring not restored at start %lld", what, start);
}

template <bool CHROMA>
static void sweep(const std::vector<uint32_t> &w, uint64_t pos0, int K, Counts &cwin, Counts &chook)
{
    const Magic31 M = magic31((uint32_t)(2 * K + 1));
    constexpr int M0 = CHROMA ? LOOK_CHROMA : LOOK_LUMA;
    // the serial replay: accumulator(s) after p draws of the stream
    std::vector<int> n0(MAXSTART + 1), n1(MAXSTART + 1);
    {
        int a = 0, b = 0;
        for (int p = 0; p <= MAXSTART; p++) {
            n0[p] = a; n1[p] = b;
            if (p == MAXSTART) break;
            const int d = (int)((w[p + 31] >> 1) % (uint32_t)(2 * K + 1)) - K;
            if (CHROMA && (p & 1)) b = (b + d) / 2; else a = (a + d) / 2;
        }
    }
    for (int stride = 8; stride <= 720; stride += CHROMA ? 2 : 1) {
        for (int row = 0; row < 4; row++) {
            const long long start = (long long)stride * row;
            uint32_t st[31];
            for (int j = 0; j < 31; j++) st[j] = w[(size_t)start + j];
            uint32_t col[31 * 3];                   // a column of stride 3, as a lane's column of the LDS ring has one of 64
            Ring r;
            r.col = col; r.stride = 3;
            Acc a;
            // ---- the window path
            if (start == 0 || start >= M0) {
                from_window<M0, CHROMA>(st, M, K, start <= M0, a);
                if (start == 0) a.init(true, CHROMA, K);
                int rounds = 0;
                if (!a.settled()) {
                    r.load(st);
                    rounds = extend(r, clip(start, M0), start, CHROMA, M, K, a);
                    check_ring_restored(col, r, st, "window", start);
                }
                cwin.rows++; cwin.extended += rounds != 0; cwin.rounds += rounds;
                CHECK(a.settled() && a.lo0 == n0[start] && a.lo1 == n1[start],
                      "window path: pos0 %llu K %d chroma %d stride %d row %d: %d %d, serial %d %d", (unsigned long long)pos0,
                      K, (int)CHROMA, stride, row, a.lo0, a.lo1, n0[start], n1[start]);
            }
            // ---- the ring path at three look-back lengths
            const int lens[3] = {M0, 2, 40};
            for (int li = 0; li < 3; li++) {
                const int m0 = lens[li];
                r.load(st);
                const long long m = clip(start, m0);
                replay(r, m, start, CHROMA, M, K, a);
                const int rounds = extend(r, m, start, CHROMA, M, K, a);
                check_ring_restored(col, r, st, "ring", start);
                if (m0 == 2 && start > 2) { chook.rows++; chook.extended += rounds != 0; chook.rounds += rounds; }
                CHECK(a.settled() && a.lo0 == n0[start] && a.lo1 == n1[start],
                      "ring path: pos0 %llu K %d chroma %d stride %d row %d look-back %d: %d %d, serial %d %d",
                      (unsigned long long)pos0, K, (int)CHROMA, stride, row, m0, a.lo0, a.lo1, n0[start], n1[start]);
            }
        }
    }
}

int main()
{
    const uint64_t pos[3] = {0ull, 12345ull, 3000000007ull};
    const int Ks[4] = {1, 4, 16, 100};
    Counts cwin, chook;
    for (uint64_t p0 : pos) {
        const std::vector<uint32_t> w = stream_words(p0);
        for (int K : Ks) {
            sweep<false>(w, p0, K, cwin, chook);
            sweep<true>(w, p0, K, cwin, chook);
        }
    }
    std::printf("default look-back: %ld rows, %ld extended (%ld extensions)\n", cwin.rows, cwin.extended, cwin.rounds);
    std::printf("look-back 2 / 2:   %ld rows, %ld extended (%ld extensions)\n", chook.rows, chook.extended, chook.rounds);
    CHECK(chook.extended * 2 > chook.rows, "the hook's lengths extended only %ld of %ld rows", chook.extended, chook.rows);
    std::printf("%ld checks, %ld bad\n", checked, bad);
    return bad ? 1 : 0;
}
