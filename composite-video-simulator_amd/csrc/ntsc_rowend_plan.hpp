// ntsc_rowend_plan.hpp -- the schedule of a decoder row as the hand-tuned kernel runs it (ntsc_decode_fast.hip): which
// stream positions t form the pipeline fill, the steady loop and the drain, how fill and drain are cut into groups of
// four positions on the steady loop's phase, and which stage and which load is live at every position.  Plain integer
// code, so the same text runs on the host: tests/rowend_plan_check.cpp sweeps it with g++ against the per-position
// predicates of the one-position-at-a-time form (edge_step / vcr_edge), which stays the path of the rows and forms the
// groups do not take.
//
// Stream positions of a row of W samples (t = 0 ... W + SKT - 1, wave-uniform):
//   x1 = t - 7        first separator (VHS forms: chroma noise, phase noise, VHS chroma low-pass; the only one otherwise)
//   x2 = x1 - d       VHS forms: the VCR's luma path, vertical blend, re-modulation (d = chroma delay: 9, 12, 14)
//   x3 = x2 - 7       second separator and output filter (S-Video form: x3 = x2; non-VHS form: x3 = x1)
//   xo = x3 - 1       the pixel that leaves (full output low-pass, FO: xo = x3 - 4)
#pragma once

#ifdef __HIPCC__
#define NTSC_PLAN_FN __host__ __device__ __forceinline__
#else
#define NTSC_PLAN_FN static inline
#endif

namespace ntscsim {
namespace rowend {

struct Plan {
    int W, d;
    bool vhs, sv, fo;
    int D2;               // t - x2 (VHS forms)
    int D3;               // t - x3
    int OD;               // x3 - xo
    int SKT;              // t - xo: the pipeline's depth, and the steady loop's first position
    int LOFF;             // t - xl: the luma path's composite sample (its box filter looks two ahead of x2)
    int total;            // positions of the row: W + SKT
    int t_end;            // the steady loop stays below it: every sample inside the row, no raw chroma tail yet
    int st0, st1;         // the steady loop runs [st0, st1), st1 - st0 a multiple of 4 (st1 == st0: it does not run)
    int g0;               // first position of the first group (<= 0, = SKT mod 4: the group may be partial)
    int glast;            // first position of the last group (it may be partial too)
};

NTSC_PLAN_FN Plan make_plan(int W, int d, bool vhs, bool sv, bool fo)
{
    Plan p;
    p.W = W; p.d = vhs ? d : 0;
    p.vhs = vhs; p.sv = sv; p.fo = fo;
    p.D2 = 7 + p.d;
    p.D3 = vhs ? (sv ? p.D2 : p.D2 + 7) : 7;
    p.OD = fo ? 4 : 1;
    p.SKT = p.D3 + p.OD;
    p.LOFF = 5 + p.d;
    p.total = W + p.SKT;
    p.t_end = W - (p.d > 7 ? p.d - 7 : 0);
    p.st0 = p.SKT;
    p.st1 = p.t_end - p.SKT >= 4 ? p.SKT + ((p.t_end - p.SKT) & ~3) : p.SKT;
    p.g0 = (p.SKT & 3) ? (p.SKT & 3) - 4 : 0;
    p.glast = p.SKT + ((W - 1) & ~3);
    return p;
}

// the rows that run in groups: the ones the steady loop enters (the others take the one-position form throughout)
NTSC_PLAN_FN bool grouped(const Plan &p) { return p.st1 > p.st0; }

// what is live at stream position t
struct Pos {
    bool load_c;          // the first separator's composite sample is inside the row (else it reads 0)
    bool sep1;            // the first separator pushes (its state is dead once x1 has left the row)
    bool in1;             // x1 inside the row: two rand() draws, chroma / phase noise, VHS chroma low-pass
    bool tail_wr;         // ... and its input is kept raw for the row's last d positions
    bool load_l;          // the luma path's composite sample is inside the row (else it reads 0)
    bool in2;             // x2 inside the row: VHS luma filters, vertical blend, re-modulation
    bool tail_rd;         // ... with the raw chroma tail in place of the low-pass
    bool in3;             // x3 inside the row: the output filter pushes
    bool tv;              // the output stage runs (FO: also for the four positions behind the row)
    bool out;             // a pixel leaves, at xo
    int xo;
    bool burst;           // ... and completes a 16-pixel burst
    bool rest;            // ... or is the row's last one short of a burst: the pixels staged since the last burst leave
};

NTSC_PLAN_FN Pos position(const Plan &p, int t)
{
    Pos q;
    const int W = p.W, x1 = t - 7, x2 = t - p.D2, x3 = t - p.D3, xl = t - p.LOFF;
    q.load_c = t >= 0 && t < W;
    q.in1 = p.vhs && x1 >= 0 && x1 < W;
    q.in3 = x3 >= 0 && x3 < W;
    q.sep1 = p.vhs ? (t >= 0 && x1 < W) : (t >= 0 && x3 < W);
    q.tail_wr = q.in1 && x1 >= W - p.d;
    q.load_l = p.vhs && xl >= 0 && xl < W;
    q.in2 = p.vhs && x2 >= 0 && x2 < W;
    q.tail_rd = q.in2 && x2 >= W - p.d;
    q.tv = x3 >= 0 && x3 < W + p.OD;
    q.xo = x3 - p.OD;
    q.out = q.tv && q.xo >= 0;
    q.burst = q.out && (q.xo & 15) == 15;
    q.rest = q.out && !q.burst && q.xo == W - 1;
    return q;
}

// The luma delay ring (round 10): the first separator's box value yb(t) is the very value the VCR's luma path wants LOFF
// positions later, so a grouped row keeps it in LDS -- 16 slots per lane, position t at slot (t - SKT) & 15, every
// group's first slot a multiple of 4 -- instead of loading and filtering the samples a second time.  The static slot
// offsets are written for LOFF = 14 (SP); LP and EP (LOFF = 17, 19 > 16 slots) and the one-position rows keep the
// re-read, and a launch without ring rows allocates no LDS for it (the launcher asks this same function).
constexpr int LUMA_RING_SLOTS = 16;
constexpr int LUMA_RING_BYTES = LUMA_RING_SLOTS * 64 * 4;
NTSC_PLAN_FN bool luma_ring(const Plan &p)
{
#ifdef NTSC_LUMA_REREAD           /* A/B: the round-9 form everywhere */
    (void)p;
    return false;
#else
    return p.vhs && !p.sv && !p.fo && p.LOFF == 14 && grouped(p);
#endif
}

// rand() ring (LaneRand32): slot of the first draw of the group that starts at t0, given the slot of the row's first
// draw (at t = 7, two draws per position).  The window is placed so that the steady loop's first draw is on a multiple
// of 8 (LaneRand32::init), and every group starts a multiple of 4 positions from it: a multiple of 8 as well.
NTSC_PLAN_FN int ring_offset(int SKT) { return (-(31 + 2 * (SKT - 7))) & 7; }
NTSC_PLAN_FN int group_slot(int first_slot, int t0) { return (first_slot + 2 * (t0 - 7)) & 31; }

} // namespace rowend
} // namespace ntscsim
