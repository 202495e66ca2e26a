// Host check of csrc/ntsc_rowend_plan.hpp (built and run by tests/test_rowend_plan_host.py with plain g++, and again with
// -fsanitize=address,undefined): the schedule the hand-tuned decoder runs its rows by, against the per-position
// predicates of the one-position form (edge_step / vcr_edge of csrc/ntsc_decode_fast.hip), written out again here.
//
// For every width 1 ... 800, 1920 and 3840, the composite -vhs form at chroma delay 9, 12 and 14, the non-VHS form, the
// S-Video form and the full-output-filter form:
//   * every flag of every stream position t in [0, W + SKT) equals the one-position form's predicate;
//   * fill groups, steady loop and drain groups cover every position exactly once, the groups sit on the loop's phase,
//     and the loop's range is the one the one-position form's caller computes;
//   * inside the loop every stage is strictly inside the row; in the fill no upper bound of a stage binds and no row-end
//     rule applies, in the drain no lower bound binds (what group_step<END> leaves out);
//   * walking the positions in order, staging each pixel at slot xo & 15 and letting bursts and the row's rest leave where
//     the plan says, stores every output pixel exactly once;
//   * every group's first rand() draw is on a ring slot that is a multiple of 8.
#include <cstdio>
#include <vector>

#include "ntsc_rowend_plan.hpp"

using namespace ntscsim::rowend;

static long bad = 0;
static long checked = 0;

#define CHECK(cond, ...)                                                                         \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            if (bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); }      \
        }                                                                                        \
    } while (0)

// the one-position form's predicates at stream position t (ntsc_decode_fast.hip: vcr_edge, edge_step and the store
// logic of decode_fast_body's drain loop)
struct Ref {
    bool load_c, in1, tail_wr, load_l, in2, tail_rd, in3, live, out, burst, rest;
    int x1, x2, x3, xl, xo;
};

static Ref reference(int W, int d, bool vhs, bool sv, bool fo, int t)
{
    Ref r{};
    r.load_c = t < W;
    r.x1 = t - 7;
    r.x2 = r.x1 - d;
    r.xl = t - (5 + d);
    if (vhs) {
        r.in1 = r.x1 >= 0 && r.x1 < W;
        r.tail_wr = r.in1 && r.x1 >= W - d;
        r.load_l = r.xl >= 0 && r.xl < W;
        r.in2 = r.x2 >= 0 && r.x2 < W;
        r.tail_rd = r.in2 && r.x2 >= W - d;
        r.x3 = sv ? r.x2 : r.x2 - 7;
    } else {
        r.x3 = t - 7;
    }
    if (fo) {
        r.live = !(r.x3 < 0 || r.x3 >= W + 4);
        r.in3 = r.live && r.x3 < W;
        r.xo = r.x3 - 4;
    } else {
        r.live = !(r.x3 < 0 || r.x3 > W);
        r.in3 = r.live && r.x3 < W;
        r.xo = r.x3 - 1;
    }
    r.out = r.live && r.xo >= 0;
    r.burst = r.out && (r.xo & 15) == 15;
    r.rest = r.out && !r.burst && r.xo == W - 1;
    return r;
}

static void check_form(int W, int d, bool vhs, bool sv, bool fo)
{
    const Plan p = make_plan(W, d, vhs, sv, fo);
    const int dd = vhs ? d : 0;
    const int SKT = (vhs ? (sv ? 8 : 15) + dd : 8) + (fo ? 3 : 0);       // decode_fast_body
    CHECK(p.SKT == SKT && p.total == W + SKT && p.LOFF == 5 + dd, "W=%d d=%d vhs=%d sv=%d fo=%d", W, d, vhs, sv, fo);

    // the loop's range as steady() computes it
    const int t_end = W - (dd > 7 ? dd - 7 : 0);
    int s1 = SKT;
    while (s1 + 4 <= t_end) s1 += 4;
    CHECK(p.st0 == SKT && p.st1 == s1 && p.t_end == t_end, "W=%d d=%d: steady [%d,%d) want [%d,%d)", W, d, p.st0, p.st1, SKT, s1);
    CHECK(grouped(p) == (s1 > SKT), "W=%d d=%d", W, d);
    CHECK(p.g0 <= 0 && p.g0 > -4 && ((p.st0 - p.g0) & 3) == 0, "W=%d d=%d g0=%d", W, d, p.g0);
    CHECK(((p.glast - p.g0) & 3) == 0 && p.glast < p.total && p.glast + 4 >= p.total, "W=%d d=%d glast=%d", W, d, p.glast);

    // flags, position by position
    const int last1 = W + 6;                          // last position whose first separator is observed (x1 = W - 1)
    for (int t = 0; t < p.total; t++) {
        const Ref r = reference(W, dd, vhs, sv, fo, t);
        const Pos q = position(p, t);
        CHECK(q.load_c == r.load_c, "W=%d d=%d t=%d load_c", W, d, t);
        CHECK(q.in1 == r.in1 && q.tail_wr == r.tail_wr, "W=%d d=%d t=%d in1", W, d, t);
        CHECK(q.load_l == r.load_l, "W=%d d=%d t=%d load_l", W, d, t);
        CHECK(q.in2 == r.in2 && q.tail_rd == r.tail_rd, "W=%d d=%d t=%d in2", W, d, t);
        CHECK(q.in3 == r.in3 && q.tv == r.live, "W=%d d=%d t=%d in3", W, d, t);
        CHECK(q.out == r.out && (!r.out || q.xo == r.xo), "W=%d d=%d t=%d out", W, d, t);
        CHECK(q.burst == r.burst && q.rest == r.rest, "W=%d d=%d t=%d burst", W, d, t);
        // stages that push at every position in the one-position form: live from the row's first sample until the stage
        // behind them has taken its last value
        CHECK(q.sep1 == (t <= last1), "W=%d d=%d t=%d sep1", W, d, t);
        if (!vhs) CHECK(!q.in1 && !q.in2 && !q.load_l && !q.tail_wr && !q.tail_rd, "W=%d t=%d non-VHS", W, t);
        checked++;
    }
    // nothing is live outside [0, total)
    for (int t = -4; t < p.total + 4; t++) {
        if (t >= 0 && t < p.total) continue;
        const Pos q = position(p, t);
        CHECK(!q.load_c && !q.sep1 && !q.in1 && !q.load_l && !q.in2 && !q.in3 && !q.tv && !q.out,
              "W=%d d=%d t=%d outside", W, d, t);
    }

    // coverage: the order the kernel walks the positions in
    std::vector<int> covered(p.total, 0), order;
    if (grouped(p)) {
        for (int t0 = p.g0; t0 < p.st0; t0 += 4)
            for (int j = 0; j < 4; j++)
                if (t0 + j >= 0 && t0 + j < p.total) { covered[t0 + j]++; order.push_back(t0 + j); }
        for (int t = p.st0; t < p.st1; t++) { covered[t]++; order.push_back(t); }
        for (int t0 = p.st1; t0 < p.glast + 4; t0 += 4)
            for (int j = 0; j < 4; j++)
                if (t0 + j >= 0 && t0 + j < p.total) { covered[t0 + j]++; order.push_back(t0 + j); }
        const int xe = (W & 1) ? W - 1 : W - 2;
        for (int t = 0; t < p.total; t++) {
            const Ref r = reference(W, dd, vhs, sv, fo, t);
            if (t < p.st0) {
                // fill: only lower bounds bind, no row-end rule applies
                CHECK(r.load_c, "W=%d d=%d t=%d fill load", W, d, t);
                CHECK(!r.tail_wr && !r.tail_rd, "W=%d d=%d t=%d fill tail", W, d, t);
                CHECK(r.x1 + 4 < W && r.x1 < xe && r.x3 + 4 < W && r.x3 < xe, "W=%d d=%d t=%d fill guards", W, d, t);
                if (vhs) CHECK(r.in1 == (r.x1 >= 0) && r.load_l == (r.xl >= 0) && r.in2 == (r.x2 >= 0), "W=%d d=%d t=%d fill", W, d, t);
                CHECK(r.in3 == (r.x3 >= 0) && !r.out, "W=%d d=%d t=%d fill out", W, d, t);
            } else if (t < p.st1) {
                // the loop: every stage strictly inside the row
                CHECK(r.load_c && r.in3 && r.out, "W=%d d=%d t=%d steady", W, d, t);
                if (vhs) CHECK(r.in1 && !r.tail_wr && r.load_l && r.in2 && !r.tail_rd, "W=%d d=%d t=%d steady vhs", W, d, t);
                CHECK(r.x1 + 4 < W && r.x3 + 4 < W && r.x1 < xe && r.x3 < xe, "W=%d d=%d t=%d steady guards", W, d, t);
                CHECK(r.xo < W - 1 - (fo ? 4 : 0), "W=%d d=%d t=%d steady last sample", W, d, t);
            } else {
                // drain: only upper bounds bind
                CHECK(r.x1 >= 0 && r.x3 >= 0 && r.xo >= 0, "W=%d d=%d t=%d drain", W, d, t);
                if (vhs) CHECK(r.xl >= 0 && r.x2 >= 0, "W=%d d=%d t=%d drain vhs", W, d, t);
                CHECK(r.out == r.live, "W=%d d=%d t=%d drain out", W, d, t);
            }
        }
        // the ring slots of the groups' first draws
        if (vhs) {
            const int first_slot = (ring_offset(SKT) + 31) & 31;      // LaneRand32::init: slot of the row's first draw
            for (int t0 = p.g0; t0 < p.glast + 4; t0 += 4) {
                const int s = group_slot(first_slot, t0);
                CHECK((s & 7) == 0 && s >= 0 && s < 32, "W=%d d=%d t0=%d slot %d", W, d, t0, s);
                CHECK(s == ((first_slot + 2 * (t0 - 7)) & 31), "W=%d d=%d t0=%d", W, d, t0);
            }
        }
    } else {
        for (int t = 0; t < p.total; t++) { covered[t]++; order.push_back(t); }
    }
    for (int t = 0; t < p.total; t++) CHECK(covered[t] == 1, "W=%d d=%d t=%d covered %d times", W, d, t, covered[t]);
    for (size_t i = 1; i < order.size(); i++) CHECK(order[i] == order[i - 1] + 1, "W=%d d=%d out of order at %d", W, d, order[i]);

    // stores: 16 staging slots, bursts and the row's rest where the plan says
    std::vector<int> stored(W, 0);
    int slot[16];
    for (int &s : slot) s = -1;
    for (int t : order) {
        const Pos q = position(p, t);
        if (!q.out) continue;
        CHECK(q.xo >= 0 && q.xo < W, "W=%d d=%d t=%d xo=%d", W, d, t, q.xo);
        if (q.xo < 0 || q.xo >= W) continue;
        slot[q.xo & 15] = q.xo;
        if (q.burst || q.rest) {
            const int xb = q.xo & ~15;
            for (int x = xb; x <= q.xo; x++) {
                CHECK(slot[x & 15] == x, "W=%d d=%d x=%d leaves unstaged", W, d, x);
                stored[x]++;
            }
        }
    }
    for (int x = 0; x < W; x++) CHECK(stored[x] == 1, "W=%d d=%d vhs=%d sv=%d fo=%d: pixel %d stored %d times", W, d, vhs, sv, fo, x, stored[x]);
}

int main()
{
    std::vector<int> widths;
    for (int w = 1; w <= 800; w++) widths.push_back(w);
    widths.push_back(1920);
    widths.push_back(3840);
    const int delays[] = {9, 12, 14};
    for (int w : widths) {
        check_form(w, 0, false, false, false);
        for (int d : delays) {
            check_form(w, d, true, false, false);
            check_form(w, d, true, true, false);
            check_form(w, d, true, false, true);
        }
    }
    std::printf("%ld positions checked, %ld bad\n", checked, bad);
    return bad ? 1 : 0;
}
