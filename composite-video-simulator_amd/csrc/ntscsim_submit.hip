// ntscsim_submit.hip -- the asynchronous host-frame form of the drop-in: ntscsim_submit() / ntscsim_wait()
// (include/ntscsim.h).  Included by ntscsim_hip.hip (one translation unit).
//
// What it replaces: the call `composite_layer(ring[idx], in.rgb, in, (current&1)^1, current)` at
// ffmpeg_ntsc.cpp:2229 when the caller keeps its loop (:2202-2282) and its AVFrames, but lets `depth`
// fields be in flight.  Structure:
//
//   submit   src frame --DMA (s_up)--> device source ring          (once per frame: NTSCSIM_SUBMIT_SAME_SRC)
//            field recorded in `pending`; at `depth` fields: launch
//   launch   one lane (child ctx: own stream + scratch) runs the ordinary batched kernel chain
//            (ntscsim_fields_device) on the pending fields, then k_deliver writes every field's rows from the
//            device destination ring straight into the caller's pinned frames (or one linear D2H into the
//            staging ring for frames that are not pinned); an event closes the launch
//   wait     retire launches up to the ticket's: synchronise on the event, or on the copy threads that move staged rows
//
// Tickets, launches in flight and the source ring are the LaunchQueue's (ntscsim_queue.hip), row maps and copy lists
// engine_host.hpp's, pinning ntscsim_pins.hip's.  Here: the rings, the lanes, the order of fields that share rows of a frame.
//
// Lanes exist because a launch of 32 fields is ~125 wavefronts on a chip with 2,048 slots and takes the same
// ~0.5 ms as one of 600: three launches side by side hide that latency.  Fields carry explicit rand()
// positions, so it does not matter which lane runs which launch.

namespace {

struct DeliverRec {
    const uint8_t *dev;       // device frame (row 0)
    uint8_t *host;            // device-visible address of the caller's frame (row 0)
    int32_t dev_pitch, host_pitch;
    int32_t row0, row_step, nrows;
    int32_t bob;              // 0: row y <- device row y;  1 + field: line doubling, row y <- the field's row beside it
};

// One workgroup per (row chunk, field): copies rows row0, row0+row_step, ... of a device frame into the
// caller's (pinned, device-mapped) frame.  Stores go over the host link; 16-byte stores when every address is
// 16-byte aligned.  With `bob` the loop's line doubling (ffmpeg_ntsc.cpp:2233-2257) happens on the way out: destination
// row y takes the field's row beside it (bob_src_row); the one row without a partner is not in [row0, row0 + nrows).
__global__ void k_deliver(const DeliverRec *__restrict__ recs, int row_bytes, int vec16)
{
    const DeliverRec r = recs[blockIdx.y];
    for (int k = blockIdx.x; k < r.nrows; k += gridDim.x) {
        const size_t y = (size_t)r.row0 + (size_t)k * r.row_step;
        const size_t ys = r.bob == 0 ? y : bob_src_row(y, r.bob == 2);
        const uint8_t *s = r.dev + ys * (size_t)r.dev_pitch;
        uint8_t *d = r.host + y * (size_t)r.host_pitch;
        if (vec16) {
            const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
            uint4 *d4 = reinterpret_cast<uint4 *>(d);
            for (int i = threadIdx.x; i < row_bytes / 16; i += blockDim.x) d4[i] = s4[i];
        } else {
            const uint32_t *s1 = reinterpret_cast<const uint32_t *>(s);
            uint32_t *d1 = reinterpret_cast<uint32_t *>(d);
            for (int i = threadIdx.x; i < row_bytes / 4; i += blockDim.x) d1[i] = s1[i];
        }
    }
}

} // namespace

struct SubmitItem {
    uint64_t ticket;
    int src_slot, dst_slot;
    uint8_t *host_dst;        // caller's frame
    uint8_t *host_dst_dev;    // its device-visible address when pinned, else NULL (staged)
    bool direct;              // the decoder writes its rows straight into the caller's pinned frame (no ring, no k_deliver)
    int dst_ls;
    unsigned field;
    uint32_t flags;
    uint64_t fieldno, rng_pos;
};
struct SubmitLaunch {         // what a launch of this engine has beside the queue's
    hipEvent_t up = nullptr;                  // the uploads of its sources (s_up)
    hipEvent_t t0 = nullptr, t1 = nullptr;    // NTSCSIM_SUBMIT_TIMING: GPU time stamps around the launch
    unsigned lane = 0;
};

struct SubmitEngine : LaunchQueue<SubmitItem, SubmitLaunch> {
    using Item = SubmitItem;
    ntscsim_submit_opts o;
    int W = 0, H = 0;
    size_t pitch = 0, fbytes = 0;
    int nslots = 0;
    DevBuf<uint8_t> dsrc, ddst;
    uint8_t *hsrc = nullptr, *hdst = nullptr;         // pinned staging rings (lazy, nslots frames each)
    DeliverRec *recs = nullptr;                       // pinned, device-visible: nslots records
    hipStream_t s_up = nullptr;
    std::vector<ntscsim_ctx *> lanes;
    unsigned lane_next = 0;

    std::vector<uint64_t> pending_deps;   // first tickets of launches in flight that the pending one must follow (shared dst rows)
    // NTSCSIM_SUBMIT_DIRECT=0: A/B switch back to the device destination ring + k_deliver for every field
    bool direct_ok = !(std::getenv("NTSCSIM_SUBMIT_DIRECT") && std::getenv("NTSCSIM_SUBMIT_DIRECT")[0] == '0');
    std::vector<hipEvent_t> up_pool;
    PinCache pins;                    // registrations of caller memory
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool timing = std::getenv("NTSCSIM_SUBMIT_TIMING") != nullptr;      // developer switch: print every launch's GPU span
    hipEvent_t tref = nullptr;
};

extern "C" void ntscsim_submit_opts_init(ntscsim_submit_opts *o)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t)sizeof(*o);
    o->depth = 32;
    o->slots = 256;
    o->lanes = 3;
    o->pin_caller_buffers = 1;
    o->min_pin_bytes = 256u << 10;
}

static int sub_wait_ticket(ntscsim_ctx *c, uint64_t ticket);
static int sub_launch(ntscsim_ctx *c);

static SubmitEngine *sub_get(ntscsim_ctx *c)
{
    if (!c->sub) {
        c->sub = new (std::nothrow) SubmitEngine();
        if (c->sub) { ntscsim_submit_opts_init(&c->sub->o); c->sub->pins.policy = c->pin_policy; }
    }
    return c->sub;
}

static void sub_release_geometry(SubmitEngine *e)
{
    e->dsrc.release(); e->ddst.release();
    if (e->hsrc) (void)hipHostFree(e->hsrc);
    if (e->hdst) (void)hipHostFree(e->hdst);
    if (e->recs) (void)hipHostFree(e->recs);
    e->hsrc = e->hdst = nullptr; e->recs = nullptr;
    e->W = e->H = 0; e->nslots = 0;
    e->src_cur = -1;
    e->src_last_ticket.clear();
}

static void submit_engine_destroy(ntscsim_ctx *c)
{
    SubmitEngine *e = c->sub;
    if (!e) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    e->shutdown();
    for (auto &b : e->inflight) if (b.up) (void)hipEventDestroy(b.up);
    for (auto ev : e->up_pool) (void)hipEventDestroy(ev);
    for (ntscsim_ctx *l : e->lanes) ntscsim_destroy(l);
    sub_release_geometry(e);
    pin_release(e->pins, nullptr);
    if (e->s_up) (void)hipStreamDestroy(e->s_up);
    delete e;
    c->sub = nullptr;
}

extern "C" int ntscsim_submit_configure(ntscsim_ctx *c, const ntscsim_submit_opts *o)
{
    if (!c || !o || o->struct_size != sizeof(ntscsim_submit_opts)) return NTSCSIM_E_ARG;
    if (o->depth < 1 || o->depth > 4096 || o->lanes < 1 || o->lanes > 8) return NTSCSIM_E_ARG;
    if (o->slots != 0 && o->slots < 2 * o->depth) return NTSCSIM_E_ARG;
    if (o->slots > 65536) return NTSCSIM_E_ARG;
    SubmitEngine *e = sub_get(c);
    if (!e) return NTSCSIM_E_NOMEM;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = sub_wait_ticket(c, NTSCSIM_TICKET_ALL);
    if (rc != NTSCSIM_OK) return rc;
    e->o = *o;
    e->pins.policy = o->pin_caller_buffers < 0 ? 0 : (o->pin_caller_buffers > 2 ? 2 : o->pin_caller_buffers);
    e->pins.min_bytes = o->min_pin_bytes;
    if (e->o.slots == 0) e->o.slots = 8 * e->o.depth;
    while ((int)e->lanes.size() > e->o.lanes) { ntscsim_destroy(e->lanes.back()); e->lanes.pop_back(); }
    sub_release_geometry(e);          // the rings are sized by `slots`
    return NTSCSIM_OK;
}

static int sub_ensure_geometry(ntscsim_ctx *c, SubmitEngine *e, int W, int H)
{
    if (e->W == W && e->H == H && e->nslots == e->o.slots) return NTSCSIM_OK;
    // another geometry: drain, then rebuild the rings
    int rc = sub_wait_ticket(c, NTSCSIM_TICKET_ALL);
    if (rc != NTSCSIM_OK) return rc;
    sub_release_geometry(e);
    const size_t pitch = (((size_t)W * 4 + 15) / 16) * 16;
    const size_t fbytes = ((pitch * (size_t)H + 255) / 256) * 256;
    const int ns = e->o.slots;
    HIPCHK(c, e->dsrc.ensure(fbytes * (size_t)ns));
    HIPCHK(c, e->ddst.ensure(fbytes * (size_t)ns));
    HIPCHK(c, hipHostMalloc((void **)&e->recs, sizeof(DeliverRec) * (size_t)ns, hipHostMallocDefault));
    if (!e->s_up) HIPCHK(c, hipStreamCreateWithFlags(&e->s_up, hipStreamNonBlocking));
    e->W = W; e->H = H; e->pitch = pitch; e->fbytes = fbytes; e->nslots = ns;
    e->src_reset((size_t)ns);
    return NTSCSIM_OK;
}

static int sub_ensure_staging(ntscsim_ctx *c, SubmitEngine *e, bool src)
{
    uint8_t **p = src ? &e->hsrc : &e->hdst;
    if (*p) return NTSCSIM_OK;
    HIPCHK(c, hipHostMalloc((void **)p, e->fbytes * (size_t)e->nslots, hipHostMallocDefault));
    return NTSCSIM_OK;
}

static uint8_t *sub_pinned(ntscsim_ctx *c, SubmitEngine *e, const void *p, size_t span)
{
    e->pins.declared = c->declared;
    return pin_lookup(e->pins, p, span);
}

// ntscsim_host_unpin() and its relatives (ntscsim_pins.hip)
static PinCache *sub_pins(ntscsim_ctx *c) { return c->sub ? &c->sub->pins : nullptr; }
static int sub_quiesce(ntscsim_ctx *c, int *wait_rc)
{
    SubmitEngine *e = c->sub;
    *wait_rc = sub_wait_ticket(c, NTSCSIM_TICKET_ALL);
    HIPCHK(c, hipStreamSynchronize(e->s_up ? e->s_up : c->stream));
    e->src_cur = -1;
    return NTSCSIM_OK;
}

extern "C" void ntscsim_submit_stats(const ntscsim_ctx *c, uint64_t out[8])
{
    if (!out) return;
    for (int i = 0; i < 8; i++) out[i] = (c && c->sub) ? c->sub->stats[i] : 0;
    if (c && c->sub) out[6] = c->sub->pins.regs.size();      // registrations of caller memory held right now
}

// a launch retires: its upload event is free again, NTSCSIM_SUBMIT_TIMING prints its GPU span
static void sub_retired(SubmitEngine *e, SubmitEngine::Batch &b)
{
    if (e->timing && b.t0 && b.t1) {
        float a = 0, z = 0;
        (void)hipEventSynchronize(b.t1);
        (void)hipEventElapsedTime(&a, e->tref, b.t0); (void)hipEventElapsedTime(&z, e->tref, b.t1);
        std::fprintf(stderr, "launch tickets %llu..%llu lane %u: GPU %.3f .. %.3f ms (%.3f)\n", (unsigned long long)b.first,
                     (unsigned long long)b.last, b.lane, a, z, z - a);
        (void)hipEventDestroy(b.t0); (void)hipEventDestroy(b.t1);
    }
    if (b.up) e->up_pool.push_back(b.up);
}

static int sub_wait_ticket(ntscsim_ctx *c, uint64_t ticket)
{
    SubmitEngine *e = c->sub;
    if (!e) return ticket == NTSCSIM_TICKET_ALL ? NTSCSIM_OK : NTSCSIM_E_ARG;
    return e->wait_ticket(c, "submit", ticket, [&] { return sub_launch(c); }, [&](SubmitEngine::Batch &b) { sub_retired(e, b); });
}

// Enqueue the pending fields as one launch on the next lane.
static int sub_launch(ntscsim_ctx *c)
{
    SubmitEngine *e = c->sub;
    if (!e || e->pending.empty()) return NTSCSIM_OK;
    SubmitEngine::Batch b;
    auto finish = [&](int rc) { return e->close(b, rc); };
    bool have_ev = e->open(b);
    const int n = (int)b.items.size();
    if (!e->up_pool.empty()) { b.up = e->up_pool.back(); e->up_pool.pop_back(); }
    else have_ev = hipEventCreateWithFlags(&b.up, hipEventDisableTiming) == hipSuccess && have_ev;
    if (!have_ev) {
        c->err = "hipEventCreate failed";
        return finish(NTSCSIM_E_HIP);
    }
    // the lane: a child ctx with the parent's parameters and switches
    const unsigned li = e->lane_next++ % (unsigned)e->o.lanes;
    while (e->lanes.size() <= li) {
        ntscsim_ctx *l = nullptr;
        const int rc = ntscsim_create(&c->prm, c->device, &l);
        if (rc != NTSCSIM_OK) return finish(rc);
        e->lanes.push_back(l);
    }
    ntscsim_ctx *lane = e->lanes[li];
    lane->mode = c->mode; lane->force_generic = c->force_generic; lane->no_fast_decode = c->no_fast_decode;
    lane->split_vhs = c->split_vhs;
    if (lane->warm_override[0] != c->warm_override[0] || lane->warm_override[1] != c->warm_override[1])
        ntscsim_debug_set_warmup(lane, c->warm_override[0], c->warm_override[1]);

    std::vector<ntscsim_field_desc> descs((size_t)n);
    bool any_staged = false, any_direct = false;     // any_direct: pinned frames served by k_deliver (line doubling, unaligned)
    int n_direct = 0;                                // pinned frames the decoder writes itself
    for (int i = 0; i < n; i++) {
        const SubmitEngine::Item &it = b.items[(size_t)i];
        ntscsim_field_desc &d = descs[(size_t)i];
        std::memset(&d, 0, sizeof(d));
        d.src_dev = e->dsrc.p + e->fbytes * (size_t)it.src_slot;
        d.src_linesize = (int)e->pitch;
        if (it.direct) { d.dst_dev = it.host_dst_dev; d.dst_linesize = it.dst_ls; }      // rows leave the decoder over the link
        else { d.dst_dev = e->ddst.p + e->fbytes * (size_t)it.dst_slot; d.dst_linesize = (int)e->pitch; }
        d.field = it.field;
        // (no NTSCSIM_DESC_BOB: the line doubling happens on the way out -- k_deliver's row map, or the host copy of a
        //  staged frame -- so the device frame only ever holds the field's own rows)
        d.flags = it.flags & (NTSCSIM_DESC_INTERLACED | NTSCSIM_DESC_TFF);
        d.fieldno = it.fieldno;
        d.rng_pos = it.rng_pos;
        if (it.direct) n_direct++;
        else if (it.host_dst_dev) any_direct = true;
        else any_staged = true;
    }
    hipError_t er = hipEventRecord(b.up, e->s_up);
    if (er == hipSuccess) er = hipStreamWaitEvent(lane->stream, b.up, 0);
    // launches in flight that write the same rows of the same caller frame come first (delivery in submit order)
    for (uint64_t dep : e->pending_deps)
        for (const auto &ob : e->inflight)
            if (ob.first == dep && ob.launched_ok && ob.lane != li && er == hipSuccess)
                er = hipStreamWaitEvent(lane->stream, ob.done, 0);
    e->pending_deps.clear();
    b.lane = li;
    if (e->timing) {
        if (!e->tref) { (void)hipEventCreate(&e->tref); (void)hipEventRecord(e->tref, lane->stream); }
        (void)hipEventCreate(&b.t0); (void)hipEventCreate(&b.t1);
        (void)hipEventRecord(b.t0, lane->stream);
    }
    if (er != hipSuccess) { c->err = std::string("submit launch: ") + hipGetErrorString(er); return finish(NTSCSIM_E_HIP); }
    lane->latency_form = true;         // (short launches take the three-role workgroup form: ntsc_pipe.hip)
    int rc = ntscsim_fields_device(lane, descs.data(), n, e->W, e->H, lane->stream);
    lane->latency_form = false;
    if (rc != NTSCSIM_OK) { c->err = lane->err; return finish(rc); }
    c->kernels = lane->kernels;
    // delivery
    if (any_direct) {
        // records live in the slot-indexed pinned array (a slot's record is rewritten only after its launch
        // retired); slots are handed out in ring order, so the pinned frames of a launch are a few runs of
        // consecutive records: one k_deliver per run
        bool vec16 = ((e->W * 4) & 15) == 0;
        for (const auto &it : b.items) {
            if (!it.host_dst_dev || it.direct) continue;
            DeliverRec &r = e->recs[it.dst_slot];
            r.dev = e->ddst.p + e->fbytes * (size_t)it.dst_slot;
            r.host = it.host_dst_dev;
            r.dev_pitch = (int32_t)e->pitch; r.host_pitch = it.dst_ls;
            sub_rows(e->H, it.field, (it.flags & NTSCSIM_DESC_BOB) != 0, r.row0, r.row_step, r.nrows);
            r.bob = (it.flags & NTSCSIM_DESC_BOB) ? 1 + (int32_t)it.field : 0;
            vec16 = vec16 && !(((uintptr_t)it.host_dst_dev | (uintptr_t)it.dst_ls) & 15);
        }
        size_t i = 0;
        int nd = 0;
        auto via_kernel = [](const SubmitEngine::Item &x) { return x.host_dst_dev && !x.direct; };
        while (i < b.items.size()) {
            if (!via_kernel(b.items[i])) { i++; continue; }
            size_t j = i + 1;
            while (j < b.items.size() && via_kernel(b.items[j]) && b.items[j].dst_slot == b.items[j - 1].dst_slot + 1) j++;
            hipLaunchKernelGGL(k_deliver, dim3(16, (unsigned)(j - i)), dim3(256), 0, lane->stream,
                               e->recs + b.items[i].dst_slot, e->W * 4, vec16 ? 1 : 0);
            nd += (int)(j - i);
            i = j;
        }
        er = hipGetLastError();
        if (er != hipSuccess) { c->err = std::string("k_deliver: ") + hipGetErrorString(er); return finish(NTSCSIM_E_HIP); }
        e->stats[4] += (uint64_t)nd;
    }
    e->stats[4] += (uint64_t)n_direct;
    if (any_staged) {
        rc = sub_ensure_staging(c, e, false);
        if (rc != NTSCSIM_OK) return finish(rc);
        // whole frames, runs of consecutive slots as one linear copy
        size_t i = 0;
        while (i < b.items.size()) {
            if (b.items[i].host_dst_dev) { i++; continue; }
            size_t j = i + 1;
            while (j < b.items.size() && !b.items[j].host_dst_dev && b.items[j].dst_slot == b.items[j - 1].dst_slot + 1) j++;
            const size_t off = e->fbytes * (size_t)b.items[i].dst_slot;
            er = hipMemcpyAsync(e->hdst + off, e->ddst.p + off, e->fbytes * (j - i), hipMemcpyDeviceToHost, lane->stream);
            if (er != hipSuccess) { c->err = std::string("submit D2H: ") + hipGetErrorString(er); return finish(NTSCSIM_E_HIP); }
            e->stats[5] += (uint64_t)(j - i);
            i = j;
        }
    }
    if (e->timing) (void)hipEventRecord(b.t1, lane->stream);
    er = hipEventRecord(b.done, lane->stream);
    if (er != hipSuccess) { c->err = std::string("hipEventRecord: ") + hipGetErrorString(er); return finish(NTSCSIM_E_HIP); }
    b.launched_ok = true;
    e->stats[1]++;
    if (any_staged) {
        std::vector<CopyOp> ops;
        for (const auto &it : b.items)
            if (!it.host_dst_dev)
                sub_delivery_ops(it.host_dst, it.dst_ls, e->hdst + e->fbytes * (size_t)it.dst_slot, e->pitch, e->W, e->H, it.field,
                                 (it.flags & NTSCSIM_DESC_BOB) != 0, ops);
        e->post(b, c->device, std::move(ops));
    }
    return finish(NTSCSIM_OK);
}

extern "C" int ntscsim_flush(ntscsim_ctx *c)
{
    if (!c) return NTSCSIM_E_ARG;
    if (!c->sub && !c->h422) return NTSCSIM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = c->sub ? sub_launch(c) : NTSCSIM_OK;
    if (c->h422) { const int r = h422_launch(c); if (rc == NTSCSIM_OK) rc = r; }
    return rc;
}

extern "C" int ntscsim_wait(ntscsim_ctx *c, uint64_t ticket)
{
    if (!c) return NTSCSIM_E_ARG;
    // a ctx serves one of the two tools: tickets of ntscsim_submit422() (ntscsim_host422.hip) are waited for here too
    if (c->h422) {
        HIPCHK(c, hipSetDevice(c->device));
        if (!c->sub) return h422_wait_ticket(c, ticket);
        if (ticket != NTSCSIM_TICKET_ALL) return NTSCSIM_E_ARG;      // two ticket sequences on one ctx: only "all" is unambiguous
        const int r = h422_wait_ticket(c, ticket);
        const int r2 = sub_wait_ticket(c, ticket);
        return r != NTSCSIM_OK ? r : r2;
    }
    if (!c->sub) return ticket == NTSCSIM_TICKET_ALL ? NTSCSIM_OK : NTSCSIM_E_ARG;
    if (ticket != NTSCSIM_TICKET_ALL && ticket <= c->sub->done_ticket && ticket != 0) return NTSCSIM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return sub_wait_ticket(c, ticket);
}

extern "C" int ntscsim_submit(ntscsim_ctx *c, const uint8_t *src, int src_ls, int src_interlaced, int src_tff,
                              uint8_t *dst, int dst_ls, int W, int H, unsigned field, uint64_t fieldno,
                              uint32_t flags, uint64_t *ticket)
{
    if (!c || !src || !dst) return NTSCSIM_E_ARG;                   // :1578-1579
    if (src_ls < 4 * W || dst_ls < 4 * W) return NTSCSIM_E_SIZE;     // :1580-1581
    if (field > 1) return NTSCSIM_E_ARG;
    if (W < 16 || H < 2 || W > 16384 || H > 16384) return NTSCSIM_E_SIZE;
    if (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)src_ls | (uintptr_t)dst_ls) & 3) return NTSCSIM_E_ARG;
    if (flags & ~(NTSCSIM_DESC_BOB | NTSCSIM_SUBMIT_SAME_SRC | NTSCSIM_SUBMIT_SRC_STABLE)) return NTSCSIM_E_ARG;
    SubmitEngine *e = sub_get(c);
    if (!e) return NTSCSIM_E_NOMEM;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = sub_ensure_geometry(c, e, W, H);
    if (rc != NTSCSIM_OK) return rc;

    // ring space: ticket t uses destination slot t mod nslots; the launch that held it must have retired
    const uint64_t t = e->next_ticket;
    if (const uint64_t holder = e->slot_holder((uint64_t)e->nslots)) {
        e->stats[7]++;
        rc = sub_wait_ticket(c, holder);
        if (rc != NTSCSIM_OK) return rc;
    }
    const size_t rb = (size_t)W * 4;
    // source frame
    int sslot = e->src_cur;
    if (!(flags & NTSCSIM_SUBMIT_SAME_SRC) || sslot < 0) {
        uint64_t last;
        sslot = e->src_next((uint64_t)e->nslots, &last);
        if (last) {
            // (cannot happen while sources <= fields in flight <= nslots, kept as a guard)
            rc = sub_wait_ticket(c, last);
            if (rc != NTSCSIM_OK) return rc;
        }
        uint8_t *dslot = e->dsrc.p + e->fbytes * (size_t)sslot;
        const size_t span = (size_t)src_ls * (size_t)(H - 1) + rb;
        const bool pinned = sub_pinned(c, e, src, span) != nullptr;
        const uint8_t *from = src;
        size_t from_ls = (size_t)src_ls;
        if (!pinned) {
            rc = sub_ensure_staging(c, e, true);
            if (rc != NTSCSIM_OK) return rc;
            uint8_t *hs = e->hsrc + e->fbytes * (size_t)sslot;
            if ((size_t)src_ls == e->pitch) std::memcpy(hs, src, span);
            else for (int y = 0; y < H; y++) std::memcpy(hs + e->pitch * (size_t)y, src + (size_t)src_ls * (size_t)y, rb);
            from = hs; from_ls = e->pitch;
            e->stats[3]++;
        }
        if (from_ls == e->pitch)
            HIPCHK(c, hipMemcpyAsync(dslot, from, e->pitch * (size_t)(H - 1) + rb, hipMemcpyHostToDevice, e->s_up));
        else
            HIPCHK(c, hipMemcpy2DAsync(dslot, e->pitch, from, from_ls, rb, (size_t)H, hipMemcpyHostToDevice, e->s_up));
        // the caller may rewrite src as soon as we return: the DMA must have read it
        if (pinned && !(flags & NTSCSIM_SUBMIT_SRC_STABLE)) HIPCHK(c, hipStreamSynchronize(e->s_up));
        e->src_filled(sslot);
        e->stats[2]++;
    }
    // destination
    const size_t dspan = (size_t)dst_ls * (size_t)(H - 1) + rb;
    SubmitEngine::Item it;
    it.ticket = t;
    it.src_slot = sslot;
    it.dst_slot = (int)(t % (uint64_t)e->nslots);
    it.host_dst = dst;
    it.host_dst_dev = sub_pinned(c, e, dst, dspan);
    it.dst_ls = dst_ls;
    // the decoder's 64-byte row bursts go straight into a pinned, 16-byte aligned frame; line doubling (every row written
    // twice) and unaligned frames keep the device ring + k_deliver
    it.direct = e->direct_ok && it.host_dst_dev && !(flags & NTSCSIM_DESC_BOB) &&
                !(((uintptr_t)it.host_dst_dev | (uintptr_t)dst_ls) & 15);
    {
        // delivery in submit order for fields that write the same rows of the same frame: the pending launch goes out
        // first, and the next one waits for every launch in flight that holds such a field
        const unsigned rows = sub_item_rows(flags, field);
        bool clash = false;
        for (const auto &pi : e->pending)
            if (sub_dst_conflict(dst, dst_ls, rows, pi.host_dst, pi.dst_ls, sub_item_rows(pi.flags, pi.field), W, H)) { clash = true; break; }
        if (clash) {
            rc = sub_launch(c);
            if (rc != NTSCSIM_OK) return rc;
        }
        for (const auto &ob : e->inflight) {
            bool hit = false;
            for (const auto &oi : ob.items)
                if (sub_dst_conflict(dst, dst_ls, rows, oi.host_dst, oi.dst_ls, sub_item_rows(oi.flags, oi.field), W, H)) { hit = true; break; }
            if (hit && std::find(e->pending_deps.begin(), e->pending_deps.end(), ob.first) == e->pending_deps.end())
                e->pending_deps.push_back(ob.first);
        }
    }
    it.field = field;
    it.flags = (flags & NTSCSIM_DESC_BOB) | (src_interlaced ? NTSCSIM_DESC_INTERLACED : 0u) | (src_tff ? NTSCSIM_DESC_TFF : 0u);
    it.fieldno = fieldno;
    it.rng_pos = c->rng_pos;
    c->rng_pos += ntscsim_rng_calls_per_field(&c->prm, W, H, field);
    e->src_last_ticket[(size_t)sslot] = t;
    e->pending.push_back(it);
    e->next_ticket++;
    e->stats[0]++;
    if (ticket) *ticket = t;
    if ((int)e->pending.size() >= e->o.depth) return sub_launch(c);
    return NTSCSIM_OK;
}
