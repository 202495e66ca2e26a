// ntsc_rowstate_lookback.hpp -- the noise accumulator(s) at a scanline's first draw, from the rand() window that the
// jump to that draw delivers anyway (k_row_states, ntsc_kernels.hip: row_states_body).  Plain integer code, so the same
// text runs on the host: tests/rowstate_lookback_check.cpp sweeps it with g++ against the serial replay from the
// stream's first draw.
//
// The reference carries an accumulator down the whole field, n <- (n + draw % (2K + 1) - K) / 2 with C truncation: the
// map is monotone in n, keeps n inside [-K, K] and halves the distance of two values, so running it from both ends of
// that range over the last m draws before the row pins the exact value as soon as the two trajectories meet.  The window
// at the row's start holds the raw words of the last 31 draws (draw = word >> 1), so for m <= 31 nothing has to be
// generated.  Where the trajectories have not met, the look-back grows by EXTEND draws at a time: the generator is
// reversible (s[i-31] = s[i] - s[i-3]), the lane walks its window back in place and forward again, and the walk is
// clipped at the stream's first draw of the field, where the accumulator is 0 and the result exact by construction.
#pragma once
#include <stdint.h>
#include "glibc_rand.hpp"   // Magic31

#ifdef __HIPCC__
#define NTSC_LB_FN __host__ __device__ __forceinline__
#else
#define NTSC_LB_FN inline
#endif

namespace ntscsim {
namespace rowstate {

constexpr int LOOK_LUMA = 24;      // draws looked back at first: luma (one accumulator, every draw its own)
constexpr int LOOK_CHROMA = 31;    // chroma (U and V take the draws in turn): the whole window
constexpr int EXTEND = 32;         // draws added per extension

NTSC_LB_FN int half(int n) { return (n + (int)((unsigned)n >> 31)) >> 1; }   // C `/ 2` (truncating)
NTSC_LB_FN unsigned mulhi(unsigned a, unsigned b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __umulhi(a, b);
#else
    return (unsigned)(((unsigned long long)a * b) >> 32);
#endif
}
// what a draw adds to its accumulator before the halving: draw % (2K + 1) - K, from the window's raw word
NTSC_LB_FN int delta(uint32_t word, const Magic31 &M, int K)
{
    const unsigned draw = word >> 1;
    return (int)(draw - (mulhi(draw, M.mul) >> M.shift) * M.div) - K;
}

// the two trajectories of the stream's accumulators: luma uses the first pair, chroma both (0 = U, 1 = V)
struct Acc {
    int lo0, hi0, lo1, hi1;
    // exact: the look-back starts at the stream's first draw of the field (accumulators 0)
    NTSC_LB_FN void init(bool exact, bool chroma, int K)
    {
        lo0 = exact ? 0 : -K; hi0 = exact ? 0 : K;
        lo1 = chroma ? lo0 : 0; hi1 = chroma ? hi0 : 0;
    }
    NTSC_LB_FN void push0(int d) { lo0 = half(lo0 + d); hi0 = half(hi0 + d); }
    NTSC_LB_FN void push1(int d) { lo1 = half(lo1 + d); hi1 = half(hi1 + d); }
    NTSC_LB_FN bool settled() const { return lo0 == hi0 && lo1 == hi1; }
};

// The look-back over the last M0 draws straight from the window (st[30] = the newest word), for a lane with at least
// M0 draws behind it.  A chroma row starts on an even draw of its stream, so the draw i positions back is V's for odd i.
template <int M0, bool CHROMA>
NTSC_LB_FN void from_window(const uint32_t (&st)[31], const Magic31 &M, int K, bool exact, Acc &a)
{
    static_assert(M0 >= 1 && M0 <= 31, "the window holds 31 draws");
    a.init(exact, CHROMA, K);
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int i = M0; i >= 1; i--) {
        const int d = delta(st[31 - i], M, K);
        if (CHROMA && (i & 1)) a.push1(d); else a.push0(d);
    }
}

// A lane's window as a ring of 31 words, `stride` words apart (the kernel: a column of its LDS ring), walked in place.
// slot = the oldest word, s[p-31], p being the position of the next draw.
struct Ring {
    uint32_t *col;
    int stride;
    int slot;
    NTSC_LB_FN void load(const uint32_t (&st)[31])
    {
        for (int j = 0; j < 31; j++) col[j * stride] = st[j];
        slot = 0;
    }
    // p -> p - 1: the newest word s[p-1] turns into s[p-32] = s[p-1] - s[p-4]
    NTSC_LB_FN void back()
    {
        const int n = slot == 0 ? 30 : slot - 1;
        const int j = n >= 3 ? n - 3 : n + 28;
        col[n * stride] -= col[j * stride];
        slot = n;
    }
    // the raw word of the draw at p; p -> p + 1
    NTSC_LB_FN uint32_t fwd()
    {
        const int j = slot >= 3 ? slot - 3 : slot + 28;
        const uint32_t v = col[slot * stride] + col[j * stride];
        col[slot * stride] = v;
        slot = slot == 30 ? 0 : slot + 1;
        return v;
    }
};

// The look-back over the last m draws (m <= start, any length) through the ring: back m draws, then forward again with
// both trajectories.  Leaves the ring as it found it.
NTSC_LB_FN void replay(Ring &r, long long m, long long start, bool chroma, const Magic31 &M, int K, Acc &a)
{
    for (long long i = 0; i < m; i++) r.back();
    a.init(m == start, chroma, K);
    for (long long i = 0; i < m; i++) {
        const int d = delta(r.fwd(), M, K);
        if (chroma && ((m + i) & 1)) a.push1(d); else a.push0(d);     // (position start - m + i; start is even)
    }
}

// first look-back of a lane: the configured length, clipped at the stream's first draw
NTSC_LB_FN long long clip(long long start, int m0) { return start < (long long)m0 ? start : (long long)m0; }

// A lane whose look-back over m draws has not settled: EXTEND draws further back at a time, until it settles or reaches
// the stream's first draw.  Returns the number of extensions.
NTSC_LB_FN int extend(Ring &r, long long m, long long start, bool chroma, const Magic31 &M, int K, Acc &a)
{
    int rounds = 0;
    while (!a.settled() && m < start) {
        m = start - m < (long long)EXTEND ? start : m + EXTEND;
        replay(r, m, start, chroma, M, K, a);
        rounds++;
    }
    return rounds;
}

} // namespace rowstate
} // namespace ntscsim
