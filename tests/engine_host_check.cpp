// engine_host_check.cpp -- drives csrc/engine_host.hpp (what the host-frame engines decide without the GPU: the copy threads,
// the row maps, the copy lists of staged results, the ranges of pinned memory, the writer table of tight rows) without a GPU:
// plain C++ with its own main, compiled and run by tests/test_engine_host.py.  Prints one line per failed check and returns
// their count.
#include <cstdio>
#include <map>
#include <string>

#include "engine_host.hpp"

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

static const uint8_t FILL = 0xEE;

// ---- Delivery ---------------------------------------------------------------------------------------------------------
// The cancel check must open a gate only AFTER stop(true) has taken effect, and the class shows that to nobody; the test
// reads its private state (under its own mutex) through the explicit-instantiation idiom instead of sleeping.
template <class Tag, typename Tag::type M>
struct Rob { friend typename Tag::type get(Tag) { return M; } };
struct MutexTag { typedef std::mutex Delivery::*type; friend type get(MutexTag); };
struct CancelTag { typedef bool Delivery::*type; friend type get(CancelTag); };
struct ThreadsTag { typedef std::vector<std::thread> Delivery::*type; friend type get(ThreadsTag); };
template struct Rob<MutexTag, &Delivery::m_>;
template struct Rob<CancelTag, &Delivery::cancel_>;
template struct Rob<ThreadsTag, &Delivery::threads_>;

struct Gate {
    std::mutex m; std::condition_variable cv; bool is_open = false;
    void open() { { std::lock_guard<std::mutex> lk(m); is_open = true; } cv.notify_all(); }
    void pass() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return is_open; }); }
};

// one launch's worth of copies: N_OPS strided ops of ROWS rows (row bytes < source pitch < destination pitch) and one
// contiguous op, every op with a source and a destination region of its own
struct Job {
    static const int N_OPS = 50, ROWS = 40;
    static const size_t RB = 24, SSTEP = 40, DSTEP = 56;
    std::vector<uint8_t> src, dst;
    std::vector<CopyOp> ops;
    explicit Job(int tag) : src((size_t)(N_OPS + 1) * ROWS * SSTEP), dst((size_t)(N_OPS + 1) * ROWS * DSTEP, FILL)
    {
        for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)((i * 7 + (size_t)tag * 13) % 199);       // never FILL
        for (int k = 0; k < N_OPS; k++) ops.push_back({dst.data() + (size_t)k * ROWS * DSTEP, src.data() + (size_t)k * ROWS * SSTEP, DSTEP, SSTEP, RB, ROWS});
        ops.push_back({dst.data() + (size_t)N_OPS * ROWS * DSTEP, src.data() + (size_t)N_OPS * ROWS * SSTEP, RB, RB, RB, ROWS});
    }
    // every op applied (a second application would look the same: what can be seen is that nothing is missing and that
    // nothing else was written); bytes beyond `rb` of every destination row keep their fill
    bool in_place() const
    {
        std::vector<uint8_t> want(dst.size(), FILL);
        for (const CopyOp &o : ops)
            for (int r = 0; r < o.rows; r++)
                std::memcpy(want.data() + (o.dst - dst.data()) + o.dstep * (size_t)r, o.src + o.sstep * (size_t)r, o.rb);
        return want == dst;
    }
    bool untouched() const { return std::count(dst.begin(), dst.end(), FILL) == (long)dst.size(); }
    std::vector<CopyOp> take() const { return ops; }
};

static void delivery_checks(const char *threads_env, size_t threads_want)
{
    if (threads_env) setenv("NTSCSIM_COPY_THREADS", threads_env, 1);
    else unsetenv("NTSCSIM_COPY_THREADS");
    Delivery d;
    std::mutex om;
    std::vector<int> order;                     // the waiters, as the lead thread calls them
    int starts = 0;
    auto note = [&](int id) { std::lock_guard<std::mutex> lk(om); order.push_back(id); };
    auto on_start = [&] { std::lock_guard<std::mutex> lk(om); starts++; };

    // post order: job 1's waiter blocks on a gate, job 2's returns at once and must find job 1's bytes in place
    Job j1(1), j2(2);
    Gate g1;
    bool j1_first = false;
    d.post([&] { note(1); g1.pass(); return true; }, j1.take(), 1, on_start);
    d.post([&] { note(2); j1_first = j1.in_place(); return true; }, j2.take(), 2, on_start);
    CHECK((d.*get(ThreadsTag())).size() == threads_want);
    CHECK(j1.untouched() && j2.untouched());            // (nothing moves before its launch is done)
    g1.open();
    CHECK(d.wait(2));
    CHECK(d.wait(1));
    CHECK(j1_first && j1.in_place() && j2.in_place());
    CHECK((order == std::vector<int>{1, 2}));

    // a launch that failed: wait() says so (every time), its ops are not applied, later launches are delivered
    Job j3(3), j4(4);
    d.post([&] { note(3); return false; }, j3.take(), 3);
    d.post([&] { note(4); return true; }, j4.take(), 4);
    CHECK(d.wait(4));
    CHECK(!d.wait(3) && !d.wait(3));
    CHECK(d.wait(1) && d.wait(2));
    CHECK(j3.untouched() && j4.in_place());

    // drain() returns only after the last post is in place
    Job j5(5);
    d.post([&] { note(5); return true; }, j5.take(), 5);
    d.drain();
    CHECK(j5.in_place());

    // stop(true) drops what is undelivered: job 6's launch completes only after the cancel has taken effect, job 7 is queued
    // behind it
    Job j6(6), j7(7);
    d.post([&] {
               note(6);
               for (;;) {
                   { std::lock_guard<std::mutex> lk(d.*get(MutexTag())); if (d.*get(CancelTag())) break; }
                   std::this_thread::yield();
               }
               return true;
           },
           j6.take(), 6);
    d.post([&] { note(7); return true; }, j7.take(), 7);
    d.stop(true);
    CHECK(j6.untouched() && j7.untouched());
    CHECK((d.*get(ThreadsTag())).empty());
    CHECK(d.wait(7));                                   // (dropped is not failed)

    // a post after stop() restarts the threads (the start hook runs again) and is delivered
    Job j8(8);
    d.post([&] { note(8); return true; }, j8.take(), 8, on_start);
    CHECK((d.*get(ThreadsTag())).size() == threads_want);
    CHECK(d.wait(8) && j8.in_place());
    d.stop();
    CHECK(starts == 2);
    CHECK((order == std::vector<int>{1, 2, 3, 4, 5, 6, 7, 8}));
    CHECK(j1.in_place() && j2.in_place() && j3.untouched() && j4.in_place() && j5.in_place() && j6.untouched() && j7.untouched());
}

// ---- copy lists: run them, and check what they may touch -----------------------------------------------------------------
struct Plane { const uint8_t *p; size_t bytes; };

// every op reads inside `from`, writes inside one of `to`, and no byte is written twice; returns bytes written per plane of `to`
static std::vector<size_t> run_ops(const std::vector<CopyOp> &ops, Plane from, const std::vector<Plane> &to)
{
    std::map<const uint8_t *, int> written;
    std::vector<size_t> per(to.size(), 0);
    for (const CopyOp &o : ops) {
        CHECK(o.rows > 0 && o.rb > 0);
        for (int r = 0; r < o.rows; r++) {
            const uint8_t *s = o.src + o.sstep * (size_t)r;
            uint8_t *t = o.dst + o.dstep * (size_t)r;
            CHECK(s >= from.p && s + o.rb <= from.p + from.bytes);
            size_t k = 0;
            while (k < to.size() && !(t >= to[k].p && t + o.rb <= to[k].p + to[k].bytes)) k++;
            CHECK(k < to.size());
            if (k == to.size()) continue;
            per[k] += o.rb;
            for (size_t i = 0; i < o.rb; i++) CHECK(++written[t + i] == 1);
            std::memcpy(t, s, o.rb);
        }
    }
    return per;
}

// ---- the BGRA engine's row maps ------------------------------------------------------------------------------------------
static void row_map_checks()
{
    const int W = 16, PITCH = 80, LS = 96;                  // row bytes 64 < device pitch < caller linesize
    for (int H = 2; H <= 5; H++)
        for (unsigned field = 0; field < 2; field++)
            for (int bob = 0; bob < 2; bob++) {
                std::vector<uint8_t> dev((size_t)PITCH * H, 0);
                auto enc = [](int row, int x) { return (uint8_t)(row * 37 + x + 1); };        // < FILL, distinct rows at every x
                for (int y = 0; y < H; y++)
                    for (int x = 0; x < 4 * W; x++) dev[(size_t)y * PITCH + x] = enc(y, x);
                // the model, from the contract (include/ntscsim.h, ntscsim_submit) and the reference's loop: composite_layer()
                // writes rows field, field + 2, ...; then ffmpeg_ntsc.cpp:2233-2257 on the caller's frame
                std::vector<uint8_t> want((size_t)LS * H, FILL);
                auto row = [&](std::vector<uint8_t> &f, int y) { return f.data() + (size_t)LS * y; };
                for (int y = (int)field; y < H; y += 2) std::memcpy(row(want, y), dev.data() + (size_t)PITCH * y, 4 * W);
                if (bob && field) for (int y = 1; y < H; y += 2) std::memcpy(row(want, y - 1), row(want, y), 4 * W);
                if (bob && !field) for (int y = 1; y + 1 < H; y += 2) std::memcpy(row(want, y), row(want, y + 1), 4 * W);
                // the staged copy list
                std::vector<uint8_t> got((size_t)LS * H, FILL);
                std::vector<CopyOp> ops;
                sub_delivery_ops(got.data(), LS, dev.data(), PITCH, W, H, field, bob != 0, ops);
                run_ops(ops, {dev.data(), dev.size()}, {{got.data(), got.size()}});
                CHECK(got == want);
                // the rows as k_deliver takes them
                std::vector<uint8_t> ker((size_t)LS * H, FILL);
                int row0, step, n;
                sub_rows(H, field, bob != 0, row0, step, n);
                for (int k = 0; k < n; k++) {
                    const size_t y = (size_t)row0 + (size_t)k * step;
                    const size_t ys = bob ? bob_src_row(y, field != 0) : y;
                    CHECK(y < (size_t)H && ys < (size_t)H);
                    if (y < (size_t)H && ys < (size_t)H) std::memcpy(row(ker, (int)y), dev.data() + (size_t)PITCH * ys, 4 * W);
                }
                CHECK(ker == want);
                CHECK(sub_item_rows(bob ? NTSCSIM_DESC_BOB : 0u, field) == (bob ? 2u : field));
            }
}

static void dst_conflict_checks()
{
    const int W = 16, H = 4, LS = 96;
    const uint8_t *f = reinterpret_cast<const uint8_t *>((uintptr_t)0x100000);     // numbers: nothing reads a frame
    const size_t span = (size_t)LS * (H - 1) + 4 * W;
    CHECK(!sub_dst_conflict(f, LS, 0, f, LS, 1, W, H) && !sub_dst_conflict(f, LS, 1, f, LS, 0, W, H));     // the two fields of a frame
    CHECK(sub_dst_conflict(f, LS, 0, f, LS, 0, W, H) && sub_dst_conflict(f, LS, 1, f, LS, 1, W, H));       // same parity
    for (unsigned r = 0; r < 3; r++) CHECK(sub_dst_conflict(f, LS, 2, f, LS, r, W, H) && sub_dst_conflict(f, LS, r, f, LS, 2, W, H));      // bob
    CHECK(!sub_dst_conflict(f, LS, 2, f + span, LS, 2, W, H) && !sub_dst_conflict(f + span, LS, 2, f, LS, 2, W, H));       // frames that touch
    CHECK(sub_dst_conflict(f, LS, 2, f + span - 1, LS, 2, W, H));                                            // ... share one byte
    CHECK(sub_dst_conflict(f, LS, 0, f, LS + 16, 1, W, H));                      // views of other geometry: assume the worst
    CHECK(sub_dst_conflict(f, LS, 0, f + 4, LS, 1, W, H));
}

// ---- the 4:2:2 engine's copy list ----------------------------------------------------------------------------------------
static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

static void h422_ops_checks()
{
    const int W = 16, W2 = W / 2;
    for (int H : {2, 3, 5, 6, 64, 65})               // (64: the encoder frame's luma goes in two halves)
        for (uint32_t mode = NTSCSIM_OUT422_BOB422; mode <= NTSCSIM_OUT422_FRAME; mode++)
            for (int flt = 0; flt < 2; flt++)
                for (unsigned field = 0; field < 2; field++)
                    for (int how = 0; how < 27; how++) {
                        const int frm_how = how % 3, flt_how = how / 3 % 3, out_how = how / 9;
                        if (H >= 64 && (frm_how || flt_how)) continue;       // (the tall cases are about the encoder frame)
                        // the record as the engine lays it out: [field rows of the frame][encoder frame][field rows of the filter frame]
                        const int L = (H + 1) / 2;
                        H422Record R;
                        R.W = W; R.H = H;
                        R.dn_frm = 0;
                        R.dn_out = up256((size_t)L * W * 2);
                        R.dn_flt = R.dn_out + up256((size_t)H * W + 2 * (size_t)(H + 1) * W2);
                        R.dbytes = R.dn_flt + up256((size_t)L * W * 2);
                        std::vector<uint8_t> st(R.dbytes);
                        for (size_t i = 0; i < st.size(); i++) st[i] = (uint8_t)(i % 199);
                        // chroma rows of the encoder frame, from the header: 4:2:2 has `height`, 4:2:0 (height + 1) / 2
                        const int ch = (mode == NTSCSIM_OUT422_BOB422 || mode == NTSCSIM_OUT422_FRAME) ? H : (H + 1) / 2;
                        const int ls[3] = {W + 8, W2 + 4, W2 + 12};
                        std::vector<uint8_t> buf[3][3];              // frame, filter, out x planes
                        ntscsim_loop422 it;
                        std::memset(&it, 0, sizeof(it));
                        it.width = W; it.height = H; it.field = field; it.out_mode = mode;
                        ntscsim_frame422 *fr[3] = {&it.frame, &it.filter, &it.out};
                        std::vector<Plane> to;
                        for (int f = 0; f < 3; f++)
                            for (int k = 0; k < 3; k++) {
                                const int rows = (f == 2 && k) ? ch : H;
                                buf[f][k].assign((size_t)ls[k] * rows, FILL);
                                fr[f]->data[k] = buf[f][k].data(); fr[f]->linesize[k] = ls[k];
                                to.push_back({buf[f][k].data(), buf[f][k].size()});
                            }
                        std::vector<CopyOp> ops;
                        h422_delivery_ops(R, st.data(), it, flt != 0, frm_how, flt_how, out_how, ops);
                        const std::vector<size_t> per = run_ops(ops, {st.data(), st.size()}, to);
                        // what arrives: the field's rows of frame and filter frame, all of the encoder frame -- and only what is staged
                        const size_t n = (size_t)((H - (int)field + 1) / 2);
                        const size_t want[3][3] = {{n * W, n * W2, n * W2}, {n * W, n * W2, n * W2}, {(size_t)H * W, (size_t)ch * W2, (size_t)ch * W2}};
                        const bool on[3] = {frm_how == 0, flt && flt_how == 0, out_how == 0};
                        for (int f = 0; f < 3; f++)
                            for (int k = 0; k < 3; k++) CHECK(per[(size_t)(3 * f + k)] == (on[f] ? want[f][k] : 0));
                        // ... in the rows of the field, from the record's section of that result
                        for (int f = 0; f < 2; f++)
                            for (int k = 0; k < 3 && on[f]; k++)
                                for (int y = 0; y < H; y++) {
                                    const uint8_t *r = buf[f][k].data() + (size_t)ls[k] * y;
                                    const size_t rb = k ? W2 : W;
                                    const bool mine = (unsigned)(y & 1) == field;
                                    const size_t sec = (f ? R.dn_flt : R.dn_frm) + (k == 0 ? 0 : n * W + (k == 2 ? n * W2 : 0)) + rb * (size_t)(y / 2);
                                    CHECK(mine ? std::memcmp(r, st.data() + sec, rb) == 0 : std::count(r, r + ls[k], FILL) == ls[k]);
                                    CHECK(std::count(r + rb, r + ls[k], FILL) == (long)(ls[k] - rb));
                                }
                        // ... and the encoder frame whole; the record keeps one spare row per chroma plane (the repack's row past
                        // a 4:2:0 plane), which is not delivered
                        for (int k = 0; k < 3 && on[2]; k++)
                            for (int y = 0; y < (k ? ch : H); y++) {
                                const size_t rb = k ? W2 : W;
                                const size_t sec = R.dn_out + (k == 0 ? 0 : (size_t)H * W + (k == 2 ? (size_t)(ch + 1) * W2 : 0)) + rb * (size_t)y;
                                const uint8_t *r = buf[2][k].data() + (size_t)ls[k] * y;
                                CHECK(std::memcmp(r, st.data() + sec, rb) == 0 && std::count(r + rb, r + ls[k], FILL) == (long)(ls[k] - rb));
                            }
                        CHECK(h422_field_rows(H, field) == (int)n && h422_out_chroma_rows(H, mode) == ch);
                        CHECK(R.dn_out + h422_out_bytes(W, H, mode) <= R.dn_flt);
                    }
}

// ---- ranges of pinned memory -----------------------------------------------------------------------------------------------
static void pin_range_checks()
{
    uint8_t *const dev = reinterpret_cast<uint8_t *>((uintptr_t)0x7000000000);
    PinRanges pr;
    pr.regs.push_back({0x200000, 0x203000, dev, true});
    pr.regs.push_back({0x203000, 0x204000, dev + 0x10000, false});        // a page-rounded neighbour: touches, does not overlap
    CHECK(pr.find(0x200000, 0x203000) == dev);                            // containment at both ends
    CHECK(pr.find(0x200010, 0x202ff0) == dev + 0x10);
    CHECK(pr.find(0x202fff, 0x203000) == dev + 0x2fff);
    CHECK(pr.find(0x200000, 0x203001) == nullptr);                        // one byte past the registration (the neighbour is another one)
    CHECK(pr.find(0x1fffff, 0x200010) == nullptr);
    CHECK(pr.find(0x203000, 0x204000) == dev + 0x10000);
    CHECK(!pr.overlaps(0x1ff000, 0x200000) && !pr.overlaps(0x204000, 0x205000));
    CHECK(pr.overlaps(0x1ff000, 0x200001) && pr.overlaps(0x203fff, 0x205000) && pr.overlaps(0x201000, 0x202000));
    PinRanges::Reg r;
    CHECK(!pr.release(0x204000, &r) && !pr.release(0x1fffff, &r) && pr.regs.size() == 2);
    CHECK(pr.release(0x201234, &r) && r.p0 == 0x200000 && r.p1 == 0x203000 && r.dev == dev && r.owned);      // by an interior address
    CHECK(pr.regs.size() == 1 && !pr.overlaps(0x200000, 0x203000) && pr.overlaps(0x203000, 0x203001));
    CHECK(pr.release(0x203000, &r) && !r.owned && pr.regs.empty());

    const PageSpan a = page_span(reinterpret_cast<const void *>((uintptr_t)0x200010), 0x2000);      // unaligned: both edge pages whole
    CHECK(a.p0 == 0x200000 && a.p1 == 0x203000);
    const PageSpan b = page_span(reinterpret_cast<const void *>((uintptr_t)0x200000), 0x2000);
    CHECK(b.p0 == 0x200000 && b.p1 == 0x202000);
    const PageSpan c1 = page_span(reinterpret_cast<const void *>((uintptr_t)0x200fff), 2);
    CHECK(c1.p0 == 0x200000 && c1.p1 == 0x202000);
    // the program break lies above the program's own data and below the stack
    CHECK(in_brk_heap((uintptr_t)&g_failed) && !in_brk_heap((uintptr_t)&pr));
}

// ---- the writer table of the 4:2:2 engine's TIGHT rows -----------------------------------------------------------------
// A seeded random walk over what h422_submit / h422_release_rings do to the table -- batched writes with rising tickets into
// slot t % ring, one-at-a-time iterations, DIRTY, re-makes of the rings to larger and smaller sizes, more caller frames than
// the table holds -- beside a brute-force model that keeps the whole history and answers from it: "since the last re-make,
// DIRTY, one-at-a-time iteration or eviction of this frame, which iteration wrote the other field last, and have fewer than
// ring - 2 iterations passed since".  After every step every frame and field is asked.
struct WriterEvent { enum Kind { WRITE, BREAK, GONE, RESET } kind; int frame; unsigned field; uint64_t t; };

static H422Writers::Chain writers_model(const std::vector<WriterEvent> &log, int frame, unsigned field, uint64_t t, int ring)
{
    for (size_t i = log.size(); i-- > 0;) {
        const WriterEvent &ev = log[i];
        if (ev.kind == WriterEvent::RESET) break;
        if (ev.frame != frame) continue;
        if (ev.kind == WriterEvent::BREAK || ev.kind == WriterEvent::GONE) break;
        if (ev.field == field) continue;                    // (this field's own last writer is of no interest)
        const long long passed = (long long)(t - ev.t);
        if (passed < (long long)ring - 2) return {(int)(ev.t % (uint64_t)ring), ev.t};
        break;
    }
    return {-1, 0};
}

static void writers_checks()
{
    const int HOT = 4, FRAMES = 160, STEPS = 8000;
    static const int RINGS[] = {2, 3, 4, 6, 10, 18, 34, 66, 130};
    auto ptr = [](int id) { return reinterpret_cast<const uint8_t *>((uintptr_t)0x10000000 + (uintptr_t)id * 4096); };   // (never read)
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](unsigned n) {                            // splitmix64: the same walk everywhere
        uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (unsigned)((z ^ (z >> 31)) % n);
    };
    H422Writers w;
    std::vector<WriterEvent> log;
    std::vector<int> live;                                  // the model's frames since the last re-make, oldest first
    uint64_t next = 1, reset_t = 1;
    int ring = 10, cold = HOT;
    long chained = 0, evictions = 0, grew = 0, shrank = 0, shrank_below_live = 0;
    long mismatches = 0, bad_size = 0, bad_slot = 0, bad_ticket = 0;            // (counted: a broken table fails at every step)

    auto touch = [&](int f) {                               // what at() does to the table's population
        if (std::find(live.begin(), live.end(), f) != live.end()) return;
        if (live.size() >= 64) { log.push_back({WriterEvent::GONE, live.front(), 0, 0}); live.erase(live.begin()); evictions++; }
        live.push_back(f);
    };
    auto pick = [&] {
        if (rnd(100) < 50) return (int)rnd(HOT);
        if (rnd(100) < 20) return (int)rnd(FRAMES);         // any frame again, evicted or not
        cold = cold + 1 < FRAMES ? cold + 1 : HOT;          // ... or the next new one: this is what overflows the table
        return cold;
    };
    for (int step = 0; step < STEPS; step++) {
        const unsigned what = rnd(1000);
        if (what < 620) {                                   // a batched iteration; the fields mostly alternate, as in the loop
            const int f = pick();
            const unsigned field = rnd(100) < 85 ? (unsigned)(next & 1) : rnd(2);
            const uint64_t t = next++;
            touch(f);
            w.at(ptr(f)).batched(field, t, (int)(t % (uint64_t)ring));
            log.push_back({WriterEvent::WRITE, f, field, t});
        } else if (what < 760) {                            // one at a time, on the mirror
            const int f = pick();
            next++;
            touch(f);
            w.at(ptr(f)).serial();
            log.push_back({WriterEvent::BREAK, f, 0, 0});
        } else if (what < 860) {                            // the caller rewrote the frame
            const int f = pick();
            touch(f);
            w.at(ptr(f)).dirty();
            log.push_back({WriterEvent::BREAK, f, 0, 0});
        } else if (what < 865) {                            // a re-make of the rings
            const int nr = RINGS[rnd(sizeof(RINGS) / sizeof(RINGS[0]))];
            bool below = false;                             // does the old table hold a live slot the new rings do not have?
            for (int f = 0; f < FRAMES; f++)
                for (unsigned field = 0; field < 2; field++) below = below || writers_model(log, f, field, next, ring).fslot >= nr;
            if (nr > ring) grew++;
            if (nr < ring) shrank++;
            if (below) shrank_below_live++;
            w.reset();
            log.push_back({WriterEvent::RESET, -1, 0, 0});
            live.clear();
            ring = nr;
            reset_t = next;
        } else {                                            // time passes on other frames: iterations nobody records here
            next += 1 + rnd(3);
        }
        if (w.tab.size() > H422Writers::MAX_FRAMES || w.tab.size() != live.size()) bad_size++;
        for (int f = 0; f < FRAMES; f++)
            for (unsigned field = 0; field < 2; field++) {
                const H422Writers::Entry *x = w.find(ptr(f));
                const H422Writers::Chain got = x ? x->chain_for(field, next, ring) : H422Writers::Chain{-1, 0};
                const H422Writers::Chain want = writers_model(log, f, field, next, ring);
                if (got.fslot != want.fslot || got.ticket != want.ticket) mismatches++;
                if (got.fslot >= 0) {
                    chained++;
                    if (got.fslot >= ring) bad_slot++;                                  // a slot of THIS allocation
                    if (got.ticket < reset_t || got.ticket >= next) bad_ticket++;       // ... written since it was made
                }
            }
    }
    if (mismatches || bad_size || bad_slot || bad_ticket)
        std::printf("writer table: %ld answers differ from the model, %ld slots outside the ring, %ld tickets from before the re-make, "
                    "%ld steps with a wrong table size\n", mismatches, bad_slot, bad_ticket, bad_size);
    CHECK(mismatches == 0);
    CHECK(bad_slot == 0 && bad_ticket == 0);
    CHECK(bad_size == 0);
    // the walk went where the table can go wrong
    if (!(chained > 1000 && evictions > 64 && grew > 5 && shrank > 5))
        std::printf("writer table walk: %ld chained answers, %ld evictions, %ld larger / %ld smaller re-makes\n", chained, evictions, grew, shrank);
    CHECK(chained > 1000 && evictions > 64 && grew > 5 && shrank > 5);
    CHECK(shrank_below_live > 0);                           // a re-make to fewer slots than a live fslot
}

int main()
{
    delivery_checks("1", 1);
    delivery_checks("4", 4);
    delivery_checks("16", 16);
    delivery_checks(nullptr, 4);          // the default, and the clamp at both ends
    delivery_checks("0", 1);
    delivery_checks("99", 16);
    row_map_checks();
    dst_conflict_checks();
    h422_ops_checks();
    pin_range_checks();
    writers_checks();
    if (g_failed) std::printf("%d check(s) failed\n", g_failed);
    return g_failed;
}
