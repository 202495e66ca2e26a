// ntscsim_queue.hip -- the ticket FIFO both host-frame engines run on (ntscsim_submit.hip, ntscsim_host422.hip).  Included by
// ntscsim_hip.hip (one translation unit) in front of them.
//
// Submitted work gets tickets 1, 2, ... and collects in `pending`; a launch takes all of `pending` as one Batch, closed by
// the event `done`, into `inflight`; launches retire oldest first, which is what "waiting for a ticket also completes every
// earlier one" (include/ntscsim.h) means.  Ticket t owns ring slot t mod ring; source frames have a ring position of their
// own, because several tickets may read one source (NTSCSIM_SUBMIT_SAME_SRC).  Staged results go through the copy threads
// (Delivery, engine_host.hpp).  `Item` is what an engine keeps per ticket (it has a member `ticket`), `Extra` what it adds
// to a launch.
template <class Item, class Extra>
struct LaunchQueue {
    struct Batch : Extra {
        uint64_t first = 0, last = 0;
        hipEvent_t done = nullptr;
        std::vector<Item> items;
        int rc = NTSCSIM_OK;
        bool launched_ok = false;
        bool posted = false;              // staged results: handed to the copy threads (Delivery), id = `last`
    };
    std::vector<Item> pending;
    std::deque<Batch> inflight;
    Delivery dlv;                         // staging ring -> caller frames, off the caller's thread
    std::vector<hipEvent_t> ev_pool;
    uint64_t next_ticket = 1;             // next to issue
    uint64_t done_ticket = 0;             // everything <= this has been delivered
    // source ring
    int src_cur = -1;                     // slot holding the frame of the previous submit
    uint64_t src_ring_pos = 0;
    std::vector<uint64_t> src_last_ticket;    // last ticket that reads the slot

    // A launch begins: `b` takes the pending items and an event.  false: there is no event (close the batch with an error).
    bool open(Batch &b)
    {
        b.first = pending.front().ticket;
        b.last = pending.back().ticket;
        b.items.swap(pending);
        pending.clear();
        if (!ev_pool.empty()) { b.done = ev_pool.back(); ev_pool.pop_back(); return true; }
        return hipEventCreateWithFlags(&b.done, hipEventDisableTiming) == hipSuccess;
    }
    // ... and ends, launched or not: its tickets are waited for like any others and report `rc`
    int close(Batch &b, int rc)
    {
        b.rc = rc;
        inflight.push_back(std::move(b));
        return rc;
    }
    // staged results of a launch whose `done` has been recorded: the copy threads move them as soon as the event fires
    void post(Batch &b, int device, std::vector<CopyOp> &&ops)
    {
        const hipEvent_t done = b.done;
        dlv.post([done] {
                     const bool ok = hipEventSynchronize(done) == hipSuccess;
                     if (!ok) (void)hipGetLastError();
                     return ok;
                 },
                 std::move(ops), b.last, [device] { (void)hipSetDevice(device); });
        b.posted = true;
    }
    // Retire the oldest launch: wait for it (staged rows are in the caller's frames then), recycle its event.
    // `retired(batch)`: the engine's own bookkeeping, before the batch goes.
    template <class Retired>
    int retire_front(ntscsim_ctx *c, const char *who, Retired &&retired)
    {
        Batch &b = inflight.front();
        int rc = b.rc;
        if (b.launched_ok) {
            bool ok;
            if (b.posted) ok = dlv.wait(b.last);          // (the copy threads synchronised on the event and moved the rows)
            else ok = hipEventSynchronize(b.done) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); c->err = std::string(who) + ": a launch failed on the device (hipEventSynchronize)"; rc = NTSCSIM_E_HIP; }
        }
        retired(b);
        done_ticket = b.last;
        if (b.done) ev_pool.push_back(b.done);
        inflight.pop_front();
        return rc;
    }
    // ntscsim_wait(): `launch()` sends the pending items off when the ticket is among them
    template <class Launch, class Retired>
    int wait_ticket(ntscsim_ctx *c, const char *who, uint64_t ticket, Launch &&launch, Retired &&retired)
    {
        if (ticket == NTSCSIM_TICKET_ALL) ticket = next_ticket - 1;
        if (ticket == 0) return NTSCSIM_OK;
        if (ticket >= next_ticket) return NTSCSIM_E_ARG;
        int rc = NTSCSIM_OK;
        if (!pending.empty() && ticket >= pending.front().ticket) {
            const int r = launch();
            if (r != NTSCSIM_OK) rc = r;
        }
        while (!inflight.empty() && inflight.front().first <= ticket) {
            const int r = retire_front(c, who, retired);
            if (r != NTSCSIM_OK && rc == NTSCSIM_OK) rc = r;
        }
        return rc;
    }
    // ring space: the next ticket t takes the slot that ticket t - ring held.  Returns that ticket when it has not retired
    // yet (the caller waits for it), else 0.
    uint64_t slot_holder(uint64_t ring) const
    {
        const uint64_t t = next_ticket;
        return (t > ring && done_ticket < t - ring) ? t - ring : 0;
    }
    // the slot for the next source frame; *last_reader: the ticket to wait for before the slot is overwritten (0: none)
    int src_next(uint64_t ring, uint64_t *last_reader) const
    {
        const int slot = (int)(src_ring_pos % ring);
        const uint64_t last = src_last_ticket[(size_t)slot];
        *last_reader = last > done_ticket ? last : 0;
        return slot;
    }
    void src_filled(int slot) { src_ring_pos++; src_cur = slot; }
    void src_reset(size_t ring) { src_last_ticket.assign(ring, 0); src_ring_pos = 0; src_cur = -1; }
    // the engine goes away (the device is idle): undelivered rows are dropped, the events destroyed
    void shutdown()
    {
        dlv.stop(true);
        for (auto &b : inflight) if (b.done) (void)hipEventDestroy(b.done);
        for (auto ev : ev_pool) (void)hipEventDestroy(ev);
    }
};
