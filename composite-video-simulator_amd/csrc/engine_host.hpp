// engine_host.hpp -- what the two host-frame engines (ntscsim_submit.hip, ntscsim_host422.hip) and the pinning of caller
// memory (ntscsim_pins.hip) decide WITHOUT the GPU: which rows of a caller frame a field writes and from where, the copy
// lists of staged results, the copy threads that run them, and the bookkeeping of registered address ranges.  No HIP in
// this file: tests/engine_host_check.cpp drives it with plain g++ (as tests/layer_host_check.cpp drives ntsc_layer.hpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <vector>

#include "ntscsim.h"

#if defined(__HIPCC__)
#define NTSC_HOST_DEVICE __host__ __device__
#else
#define NTSC_HOST_DEVICE
#endif

// ---- delivery of STAGED results (frames that are not pinned): the rows travel device -> pinned staging ring by DMA and
// from there into the caller's frames by memcpy.  That memcpy used to run on the caller's thread inside ntscsim_wait()
// (1.1 MB per 720x480 4:2:2 iteration: the whole budget of a 30k fields/s loop); it now runs on threads of the engine as
// soon as the launch is done, i.e. usually long before the caller asks.  One lead thread takes the launches in order
// (the job's `launched` waits for the launch -- the engines synchronise on its event --, then the copies, split over
// itself and `helpers` more threads); ntscsim_wait() only waits for the launch's id.  Copies of one launch never overlap
// each other (the engines drop all but the last writer of a row at launch time), launches are delivered one after the
// other: the caller's frames end up as the in-order loop leaves them.
struct CopyOp { uint8_t *dst; const uint8_t *src; size_t dstep, sstep, rb; int rows; };

class Delivery {
public:
    ~Delivery() { stop(); }
    // everything posted before is delivered in post order.  `launched` blocks until the launch is done and says whether it
    // succeeded; `on_start` (optional) runs first on the lead thread when this post starts the threads.
    void post(std::function<bool()> launched, std::vector<CopyOp> &&ops, uint64_t id, std::function<void()> on_start = nullptr)
    {
        std::unique_lock<std::mutex> lk(m_);
        if (!started_) start(std::move(on_start));
        q_.push_back(Job{std::move(launched), std::move(ops), id});
        posted_ = id;
        cv_.notify_all();
    }
    // true once launch `id` is in the caller's frames; false: the launch failed (the rows are lost)
    bool wait(uint64_t id)
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_done_.wait(lk, [&] { return delivered_ >= id; });
        return failed_.empty() || std::find(failed_.begin(), failed_.end(), id) == failed_.end();
    }
    void drain() { std::unique_lock<std::mutex> lk(m_); cv_done_.wait(lk, [&] { return delivered_ >= posted_; }); }
    // cancel: what has not been delivered yet is dropped, not copied (ntscsim_destroy() with fields in flight: the caller
    // never waited for them, its frames may be gone)
    void stop(bool cancel = false)
    {
        {
            std::unique_lock<std::mutex> lk(m_);
            if (!started_) return;
            cancel_ = cancel;
            cv_done_.wait(lk, [&] { return delivered_ >= posted_; });
            quit_ = true;
            cv_.notify_all();
        }
        for (auto &t : threads_) t.join();
        threads_.clear();
        started_ = false; quit_ = false; cancel_ = false;
    }

private:
    struct Job { std::function<bool()> launched; std::vector<CopyOp> ops; uint64_t id; };
    std::mutex m_;
    std::condition_variable cv_, cv_done_;
    std::deque<Job> q_;
    std::vector<std::thread> threads_;
    std::vector<uint64_t> failed_;
    uint64_t posted_ = 0, delivered_ = 0;
    bool started_ = false, quit_ = false, cancel_ = false;
    // the launch being copied: helpers pull ops by index
    const std::vector<CopyOp> *cur_ = nullptr;
    std::atomic<size_t> next_{0};
    uint64_t gen_ = 0;
    int busy_ = 0;

    static void run_op(const CopyOp &o)
    {
        if (o.dstep == o.rb && o.sstep == o.rb) { std::memcpy(o.dst, o.src, o.rb * (size_t)o.rows); return; }
        for (int r = 0; r < o.rows; r++) std::memcpy(o.dst + o.dstep * (size_t)r, o.src + o.sstep * (size_t)r, o.rb);
    }
    void pull()
    {
        const std::vector<CopyOp> &ops = *cur_;
        for (size_t i = next_.fetch_add(1); i < ops.size(); i = next_.fetch_add(1)) run_op(ops[i]);
    }
    void helper()
    {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(m_);
        for (;;) {
            cv_.wait(lk, [&] { return quit_ || (cur_ && gen_ != seen); });
            if (quit_) return;
            seen = gen_;
            lk.unlock();
            pull();
            lk.lock();
            if (--busy_ == 0) cv_done_.notify_all();
        }
    }
    void lead(const std::function<void()> &on_start)
    {
        if (on_start) on_start();
        std::unique_lock<std::mutex> lk(m_);
        for (;;) {
            cv_.wait(lk, [&] { return quit_ || !q_.empty(); });
            if (q_.empty()) return;          // quit_ and nothing left
            Job j = std::move(q_.front());
            q_.pop_front();
            lk.unlock();
            const bool ok = j.launched();
            lk.lock();
            if (ok && !cancel_ && !j.ops.empty()) {
                cur_ = &j.ops; next_.store(0); gen_++;
                busy_ = (int)threads_.size() - 1;
                cv_.notify_all();
                lk.unlock();
                pull();
                lk.lock();
                cv_done_.wait(lk, [&] { return busy_ == 0; });
                cur_ = nullptr;
            }
            if (!ok) failed_.push_back(j.id);
            delivered_ = j.id;
            cv_done_.notify_all();
        }
    }
    void start(std::function<void()> on_start)          // m_ held
    {
        const char *ev = std::getenv("NTSCSIM_COPY_THREADS");
        int n = ev ? std::atoi(ev) : 4;
        if (n < 1) n = 1;
        if (n > 16) n = 16;
        threads_.emplace_back([this, on_start = std::move(on_start)] { lead(on_start); });
        for (int i = 1; i < n; i++) threads_.emplace_back([this] { helper(); });
        started_ = true;
    }
};

// ---- registered ranges of caller memory.  Registration (hipHostRegister) is page-wise, so the first and last page of a
// buffer get pinned whole.  That is only harmless when nothing else lives in them: a foreign heap block that starts in a
// pinned page and runs on into pageable memory can no longer be the source of a hipMemcpy, and unpinning one of two
// registrations that share a page pulls it from under the other.  And never memory of the brk heap (small malloc blocks):
// the allocator trims and recycles those pages under a registration, and the GPU then faults on them -- in this call or
// in an unrelated later one (seen: sporadic aborts of the process, rocr's VMFaultHandler).
struct PageSpan { uintptr_t p0, p1; };
inline PageSpan page_span(const void *p, size_t len)
{
    const uintptr_t PG = 4096, a0 = (uintptr_t)p;
    return {a0 & ~(PG - 1), (a0 + len + PG - 1) & ~(PG - 1)};
}
inline bool in_brk_heap(uintptr_t a) { return a < (uintptr_t)sbrk(0); }

struct PinRanges {
    struct Reg { uintptr_t p0, p1; uint8_t *dev; bool owned; };      // owned: ours to unregister
    std::vector<Reg> regs;
    // device-visible address of a0 when ONE registration holds all of [a0, a1), else NULL
    uint8_t *find(uintptr_t a0, uintptr_t a1) const
    {
        for (const Reg &r : regs)
            if (a0 >= r.p0 && a1 <= r.p1) return r.dev + (a0 - r.p0);
        return nullptr;
    }
    bool overlaps(uintptr_t p0, uintptr_t p1) const
    {
        for (const Reg &r : regs)
            if (p0 < r.p1 && r.p0 < p1) return true;
        return false;
    }
    // forget the registration that holds address `a`; *out is what it was
    bool release(uintptr_t a, Reg *out)
    {
        for (size_t i = 0; i < regs.size(); i++)
            if (a >= regs[i].p0 && a < regs[i].p1) {
                *out = regs[i];
                regs.erase(regs.begin() + (long)i);
                return true;
            }
        return false;
    }
};

// ---- row maps of the BGRA engine (ntscsim_submit) ---------------------------------------------------------------------
// The loop's line doubling (ffmpeg_ntsc.cpp:2233-2257): field 1 copies odd row y onto y - 1, field 0 copies row y + 1
// onto odd row y while y + 1 < H -- destination row y takes the field's row beside it (its own when it is the field's).
NTSC_HOST_DEVICE inline size_t bob_src_row(size_t y, bool field) { return field ? (y | 1) : ((y + 1) & ~(size_t)1); }

// rows the synchronous call + (optionally) the loop's line doubling write: first row, step, count
inline void sub_rows(int H, unsigned field, bool bob, int &row0, int &step, int &n)
{
    if (!bob) { row0 = (int)field; step = 2; n = (H - (int)field + 1) / 2; return; }
    // every row except the last one when it has no partner (its source row would lie behind the frame)
    row0 = 0; step = 1;
    n = bob_src_row((size_t)H - 1, field != 0) < (size_t)H ? H : H - 1;
}

// Do two fields in flight write the same bytes of a caller frame?  (rows: 0 / 1 = the rows of that parity, 2 = every
// row: line doubling.)  The two fields of one frame do not; anything else that overlaps is ordered by the engine:
// the header promises delivery in submit order.
inline bool sub_dst_conflict(const uint8_t *a, int a_ls, unsigned a_rows, const uint8_t *b, int b_ls, unsigned b_rows,
                             int W, int H)
{
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (size_t)a_ls * (size_t)(H - 1) + (size_t)W * 4;
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (size_t)b_ls * (size_t)(H - 1) + (size_t)W * 4;
    if (a1 <= b0 || b1 <= a0) return false;
    if (a_rows == 2u || b_rows == 2u) return true;
    if (a0 == b0 && a_ls == b_ls) return a_rows == b_rows;
    return true;          // overlapping views that are not the same frame: assume the worst
}
inline unsigned sub_item_rows(uint32_t flags, unsigned field) { return (flags & NTSCSIM_DESC_BOB) ? 2u : (field & 1u); }

// What the copy threads do for one staged field: device frame `s` (row pitch `pitch`, as downloaded into the staging
// ring) -> the caller's frame.  (Fields of one launch never write the same rows: ntscsim_submit() launches before it
// accepts a field that clashes with a pending one.)
inline void sub_delivery_ops(uint8_t *dst, int dst_ls, const uint8_t *s, size_t pitch, int W, int H, unsigned field, bool bob,
                             std::vector<CopyOp> &ops)
{
    const size_t rb = (size_t)W * 4, ls = (size_t)dst_ls;
    int row0, step, nr;
    sub_rows(H, field, bob, row0, step, nr);
    if (!bob) {
        // rows field, field + 2, ...: in two halves (the ops of a launch are what the threads share out)
        const int h0 = nr / 2;
        if (h0 > 0) ops.push_back({dst + (size_t)row0 * ls, s + (size_t)row0 * pitch, 2 * ls, 2 * pitch, rb, h0});
        if (nr - h0 > 0) ops.push_back({dst + (size_t)(row0 + 2 * h0) * ls, s + (size_t)(row0 + 2 * h0) * pitch, 2 * ls, 2 * pitch, rb, nr - h0});
    } else {
        // line doubling: two strided passes (even destination rows, odd destination rows), each reading every second
        // source row
        for (int par = 0; par < 2; par++) {
            const int cnt = (nr - par + 1) / 2;           // destination rows par, par + 2, ... < nr
            if (cnt <= 0) continue;
            ops.push_back({dst + (size_t)par * ls, s + bob_src_row((size_t)par, field != 0) * pitch, 2 * ls, 2 * pitch, rb, cnt});
        }
    }
}

// ---- row maps of the 4:2:2 engine (ntscsim_submit422) -----------------------------------------------------------------
inline int h422_field_rows(int H, unsigned field) { return H > (int)field ? (H - (int)field + 1) / 2 : 0; }

// chroma rows of the encoder frame that output_frame() writes inside the plane (:1177-1236)
inline int h422_out_chroma_rows(int H, uint32_t mode) { return (mode == NTSCSIM_OUT422_BOB422 || mode == NTSCSIM_OUT422_FRAME) ? H : (H + 1) / 2; }

// ... and the rows the record keeps per chroma plane (the interlaced repack writes one row past a 4:2:0 plane for a
// height of 2 mod 4, :1215-1223: it has room here and is not delivered)
inline int h422_out_chroma_alloc(int H, uint32_t mode) { return h422_out_chroma_rows(H, mode) + 1; }
inline size_t h422_out_bytes(int W, int H, uint32_t mode) { return (size_t)W * H + 2 * (size_t)(W / 2) * (size_t)h422_out_chroma_alloc(H, mode); }

// delivery record of one iteration (device and staging): `dbytes` bytes, the field's rows of the frame at dn_frm, the
// encoder frame at dn_out, the field's rows of the filter frame at dn_flt (h422_ensure_rings)
struct H422Record { int W, H; size_t dbytes, dn_frm, dn_out, dn_flt; };

// What the copy threads do for one iteration: its staged results, staging record `st` -> caller planes.  `*_how`: 0 =
// through the staging record (the only ones copied here), 1 = written by the delivery kernels into the pinned frame, 2 =
// not at all; `flt`: the iteration delivers filter rows (the feedback path).
inline void h422_delivery_ops(const H422Record &R, const uint8_t *st, const ntscsim_loop422 &L, bool flt, int frm_how, int flt_how,
                              int out_how, std::vector<CopyOp> &ops)
{
    const int W = R.W, H = R.H, W2 = W / 2;
    const int n = h422_field_rows(H, L.field);
    auto rows_out = [&](const ntscsim_frame422 &f, const uint8_t *s) {
        for (int k = 0; k < 3; k++) {
            const size_t rb = k ? (size_t)W2 : (size_t)W;
            if (n > 0) ops.push_back({f.data[k] + (size_t)f.linesize[k] * L.field, s, 2 * (size_t)f.linesize[k], rb, rb, n});
            s += rb * (size_t)n;
        }
    };
    if (frm_how == 0) rows_out(L.frame, st + R.dn_frm);
    if (flt && flt_how == 0) rows_out(L.filter, st + R.dn_flt);
    if (L.out.data[0] && out_how == 0) {
        const uint8_t *s = st + R.dn_out;
        const int ch = h422_out_chroma_rows(H, L.out_mode);
        for (int k = 0; k < 3; k++) {
            const size_t rb = k ? (size_t)W2 : (size_t)W;
            const int nr = k ? ch : H;
            // (luma in two halves: the ops of a launch are the unit the copy threads share out)
            if (k == 0 && nr >= 64) {
                const int h0 = nr / 2;
                ops.push_back({L.out.data[0], s, (size_t)L.out.linesize[0], rb, rb, h0});
                ops.push_back({L.out.data[0] + (size_t)L.out.linesize[0] * h0, s + rb * (size_t)h0, (size_t)L.out.linesize[0], rb, rb, nr - h0});
            } else
                ops.push_back({L.out.data[k], s, (size_t)L.out.linesize[k], rb, rb, nr});
            s += rb * (size_t)(k ? h422_out_chroma_alloc(H, L.out_mode) : H);
        }
    }
}

// ---- TIGHT rows of the 4:2:2 engine: who wrote each field of a caller frame last, and into which device frame -----------
// A batched iteration on tight rows (linesize[0] < width + 2) takes the two bytes behind each of its rows -- pixels 0, 1 of
// the OTHER field's rows -- from the device frame that holds them as the in-order loop has them now: the one the last
// iteration that wrote that field rendered into (ring slot `fslot`), while that slot has not been handed out again -- fewer
// than ring - 2 iterations later.  Otherwise (nothing recorded: the first iterations of a frame, after a one-at-a-time
// iteration, a DIRTY frame or a re-make of the rings) the bytes are the caller's own, snapshotted at submit.
// Slots are positions in ONE allocation of the rings: reset() goes with every re-make (h422_release_rings), whatever the
// new ring's size, geometry or caller frame -- a slot of the old allocation is nobody's in the new one, and lies behind its
// end when the ring shrank.
struct H422Writers {
    struct Chain { int fslot; uint64_t ticket; };       // fslot < 0: none, take the snapshot
    struct Entry {
        const uint8_t *frame;
        uint64_t ticket[2];         // per field: the iteration that wrote it last (0: not this engine, or not since a break)
        int fslot[2];               // ... and the device frame it wrote
        void dirty() { ticket[0] = ticket[1] = 0; }                 // the caller rewrote the frame
        void serial() { ticket[0] = ticket[1] = 0; }                // the frame moves on in the caller's memory (mirror path)
        void batched(unsigned field, uint64_t t, int slot) { ticket[field & 1u] = t; fslot[field & 1u] = slot; }
        // iteration `t` of `field`, rings of `ring` slots: where the other field's rows are
        Chain chain_for(unsigned field, uint64_t t, int ring) const
        {
            const unsigned other = (field & 1u) ^ 1u;
            if (ticket[other] != 0 && t - ticket[other] + 2 < (uint64_t)ring) return {fslot[other], ticket[other]};
            return {-1, 0};
        }
    };
    static constexpr size_t MAX_FRAMES = 64;               // (a tool has one frame; keep the table bounded: the oldest goes)
    std::vector<Entry> tab;

    const Entry *find(const uint8_t *frame) const
    {
        for (const Entry &x : tab) if (x.frame == frame) return &x;
        return nullptr;
    }
    // the frame's entry, made when there is none (valid until the next at() / reset())
    Entry &at(const uint8_t *frame)
    {
        if (const Entry *x = find(frame)) return tab[(size_t)(x - tab.data())];
        if (tab.size() >= MAX_FRAMES) tab.erase(tab.begin());
        tab.push_back({frame, {0, 0}, {-1, -1}});
        return tab.back();
    }
    void reset() { tab.clear(); }
};
