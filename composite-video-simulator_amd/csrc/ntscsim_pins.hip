// ntscsim_pins.hip -- caller memory the GPU addresses in place: ntscsim_host_pin() and its relatives (include/ntscsim.h), the
// caches of registrations behind them, and the per-call pinning of ntscsim_frames_host().  Included by ntscsim_hip.hip (one
// translation unit), in front of the two host-frame engines, which keep a PinCache each.
//
// Which pages may be registered at all -- whole pages, never the brk heap, never a page another registration holds -- is
// written once, in engine_host.hpp (page_span, in_brk_heap, PinRanges); here are the HIP calls and each client's thresholds.

// registrations of caller memory (hipHostRegister in place), cached: a tool recycles a handful of frame buffers
// policy: 0 = never (everything is staged); 1 (default) = memory that IS pinned already -- declared with
// ntscsim_host_pin(), allocated with ntscsim_host_alloc() / hipHostMalloc, registered by the caller -- plus buffers
// that start on a page boundary; 2 = additionally blocks that carry glibc's header of a chunk with a mapping of its
// own (a peek at the allocator's internals: opt-in, glibc only)
struct PinCache : PinRanges {
    int policy = 1;
    size_t min_bytes = 256u << 10;
    const PinCache *declared = nullptr;      // the ctx's explicit registrations (ntscsim_host_pin)
};
// forget the registration that holds `base`, or all of them (NULL); everything that uses them must have completed
static void pin_release(PinCache &pc, const void *base)
{
    PinRanges::Reg r;
    if (base) {
        if (pc.release((uintptr_t)base, &r) && r.owned) (void)hipHostUnregister((void *)r.p0);
        return;
    }
    for (auto &x : pc.regs)
        if (x.owned) (void)hipHostUnregister((void *)x.p0);
    pc.regs.clear();
    (void)hipGetLastError();
}

static void declared_pins_destroy(ntscsim_ctx *c)
{
    if (!c->declared) return;
    pin_release(*c->declared, nullptr);
    delete c->declared;
    c->declared = nullptr;
}

// Pinned already -- ntscsim_host_alloc() / hipHostMalloc / the caller's own hipHostRegister: the runtime knows, no guess
// about who owns the pages is needed.  First and last byte must belong to one registration (same offset).  Returns the
// device-visible address of p; NULL with *partly set when the first byte is pinned but the span is not one registration.
static uint8_t *runtime_pinned_ptr(const void *p, size_t span, bool *partly = nullptr)
{
    hipPointerAttribute_t at0, at1;
    if (partly) *partly = false;
    if (hipPointerGetAttributes(&at0, p) != hipSuccess || at0.type != hipMemoryTypeHost || !at0.devicePointer) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (hipPointerGetAttributes(&at1, (const uint8_t *)p + (span - 1)) != hipSuccess || at1.type != hipMemoryTypeHost ||
        at1.devicePointer != (void *)((uint8_t *)at0.devicePointer + (span - 1))) {
        (void)hipGetLastError();
        if (partly) *partly = true;
        return nullptr;
    }
    return (uint8_t *)at0.devicePointer;
}

// Device-visible address of caller memory [p, p+span), pinning it in place on first sight.  NULL = not pinned
// (policy, too small, shares a page with another registration, registration refused): the staging ring is used.
static uint8_t *pin_lookup(PinCache &pc, const void *p, size_t span)
{
    if (pc.policy <= 0 || span == 0) return nullptr;
    const uintptr_t a0 = (uintptr_t)p, a1 = a0 + span;
    // (1) declared by the caller, or seen before
    if (pc.declared)
        if (uint8_t *d = pc.declared->find(a0, a1)) return d;
    if (uint8_t *d = pc.find(a0, a1)) return d;
    if (pc.regs.size() >= 1024) return nullptr;
    // (2) pinned already
    bool partly;
    if (uint8_t *d = runtime_pinned_ptr(p, span, &partly)) {
        pc.regs.push_back({a0, a1, d, false});
        return d;
    }
    if (partly) return nullptr;      // pinned in part: leave it alone, stage
    if (span < pc.min_bytes) return nullptr;
    // (3) pin in place: whole pages that are the buffer's own (engine_host.hpp), never small blocks
    if (span < (64u << 10) || in_brk_heap(a0)) return nullptr;
    if (a0 & 4095u) {
        // not on a page boundary: policy 1 stages it.  Policy 2 accepts a block that starts within the allocator's
        // header + alignment padding of a page AND carries glibc's IS_MMAPPED bit (bit 1 of the size word in front
        // of the pointer malloc / posix_memalign returned) with a chunk size that covers the span -- an allocation
        // with a mapping of its own, whose edge pages are its own.
#if defined(__GLIBC__)
        if (pc.policy < 2 || (a0 & 4095u) > 128u) return nullptr;
        size_t hdr;
        std::memcpy(&hdr, (const void *)(a0 - sizeof(size_t)), sizeof(hdr));
        if (!(hdr & 2u) || (hdr & ~(size_t)7) < span) return nullptr;
#else
        return nullptr;
#endif
    }
    const PageSpan pg = page_span(p, span);
    // partial overlap with a live registration
    if (pc.overlaps(pg.p0, pg.p1) || (pc.declared && pc.declared->overlaps(pg.p0, pg.p1))) return nullptr;
    hipError_t er = hipHostRegister((void *)pg.p0, pg.p1 - pg.p0, hipHostRegisterDefault);
    (void)hipGetLastError();
    if (er != hipSuccess) return nullptr;
    void *dev = nullptr;
    if (hipHostGetDevicePointer(&dev, (void *)pg.p0, 0) != hipSuccess || !dev) {
        (void)hipGetLastError();
        (void)hipHostUnregister((void *)pg.p0);
        return nullptr;
    }
    pc.regs.push_back({pg.p0, pg.p1, (uint8_t *)dev, true});
    return (uint8_t *)dev + (a0 - pg.p0);
}

// ntscsim_field(): the device-visible address of a caller frame that is the GPU's to address ALREADY -- declared through
// ntscsim_host_pin(), or pinned memory the runtime knows -- else NULL.  Registers nothing and remembers nothing: the
// synchronous call must not outlive the caller's allocation with a cache entry.
static uint8_t *pinned_device_ptr(ntscsim_ctx *c, const void *p, size_t span)
{
    if (!span) return nullptr;
    if (c->declared)
        if (uint8_t *d = c->declared->find((uintptr_t)p, (uintptr_t)p + span)) return d;
    return runtime_pinned_ptr(p, span);
}

// Pin two caller buffers in place for the duration of a call (ntscsim_frames_host).  Small buffers are not worth a
// registration; buffers whose page ranges touch become one registration, or none when one of them is small.
struct HostPins {
    uintptr_t s0 = 0, d0 = 0;
    bool pin_src = false, pin_dst = false;
    void pin(const void *src, size_t src_span, void *dst, size_t dst_span, unsigned flags)
    {
        const size_t MIN_PIN = 1u << 20;
        PageSpan s = page_span(src, src_span);
        const PageSpan d = page_span(dst, dst_span);
        bool want_src = src_span >= MIN_PIN && !in_brk_heap((uintptr_t)src);
        bool want_dst = dst_span >= MIN_PIN && !in_brk_heap((uintptr_t)dst);
        const bool touch = s.p0 < d.p1 && d.p0 < s.p1;
        if (want_src && want_dst && touch) {                        // page ranges touch: one registration
            s = {std::min(s.p0, d.p0), std::max(s.p1, d.p1)};
            want_dst = false;
        } else if (touch) {
            want_src = want_dst = false;                            // a small buffer inside the other's pages
        }
        s0 = s.p0; d0 = d.p0;
        pin_src = want_src && hipHostRegister((void *)s.p0, s.p1 - s.p0, flags) == hipSuccess;
        pin_dst = want_dst && hipHostRegister((void *)d.p0, d.p1 - d.p0, flags) == hipSuccess;
        (void)hipGetLastError();
    }
    void unpin()
    {
        if (pin_src) (void)hipHostUnregister((void *)s0);
        if (pin_dst) (void)hipHostUnregister((void *)d0);
        pin_src = pin_dst = false;
    }
};

// ---- the ctx's caches.  The engines are defined behind this file: each hands out its cache (NULL: no such engine yet) and
// brings itself to rest -- everything in flight waited for (*wait_rc), its own streams synchronised, the source frame of
// the previous submit forgotten.
static PinCache *h422_pins(ntscsim_ctx *c);
static PinCache *sub_pins(ntscsim_ctx *c);
static int h422_quiesce(ntscsim_ctx *c, int *wait_rc);
static int sub_quiesce(ntscsim_ctx *c, int *wait_rc);

// the 4:2:2 engine's, the BGRA engine's, the caller's declarations: those that exist, in this order
static int ctx_pin_caches(ntscsim_ctx *c, PinCache *out[3])
{
    int n = 0;
    for (PinCache *pc : {h422_pins(c), sub_pins(c), c->declared})
        if (pc) out[n++] = pc;
    return n;
}

extern "C" int ntscsim_host_unpin(ntscsim_ctx *c, const void *base)
{
    if (!c) return NTSCSIM_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = NTSCSIM_OK, r = NTSCSIM_OK;
    // (an engine that cannot be brought to rest keeps its registrations)
    if (PinCache *pc = h422_pins(c)) {
        const int q = h422_quiesce(c, &rc);
        if (q == NTSCSIM_OK) pin_release(*pc, base);
        else rc = q;
    }
    if (PinCache *pc = sub_pins(c)) {
        const int q = sub_quiesce(c, &r);
        if (rc == NTSCSIM_OK) rc = r;
        if (q != NTSCSIM_OK) return q;
        pin_release(*pc, base);
    }
    if (c->declared) {           // ... and the caller's own declaration (ntscsim_host_pin) last: nothing uses it any more
        HIPCHK(c, hipStreamSynchronize(c->stream));
        pin_release(*c->declared, base);
    }
    return rc;
}

// ---- explicit contract: the caller says which memory is its own to pin ----------
extern "C" int ntscsim_host_pin(ntscsim_ctx *c, const void *base, size_t len)
{
    if (!c || !base || len == 0) return NTSCSIM_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->declared) c->declared = new (std::nothrow) PinCache();
    if (!c->declared) return NTSCSIM_E_NOMEM;
    const uintptr_t a0 = (uintptr_t)base, a1 = a0 + len;
    const PageSpan pg = page_span(base, len);
    // What can be declared is an allocation of its own: a mapping, a block above the mmap threshold, a pool.  (The engines'
    // own pinning has always refused the brk heap: pin_lookup.)
    if (in_brk_heap(pg.p0)) {
        c->err = "ntscsim_host_pin: the range lies in the brk heap (a small malloc block); declare an allocation of its own";
        return NTSCSIM_E_ARG;
    }
    if (c->declared->find(pg.p0, pg.p1)) return NTSCSIM_OK;                 // declared before
    // registrations the engines made on their own for these pages go first (everything in flight is delivered)
    PinCache *caches[3];
    const int nc = ctx_pin_caches(c, caches);
    auto registered = [&](uintptr_t p0, uintptr_t p1) {
        for (int k = 0; k < nc; k++) if (caches[k]->overlaps(p0, p1)) return true;
        return false;
    };
    for (uintptr_t a = pg.p0; a < pg.p1 && registered(pg.p0, pg.p1); a += 4096)
        if (registered(a, a + 1)) {
            const int rc = ntscsim_host_unpin(c, (const void *)a);
            if (rc != NTSCSIM_OK) return rc;
        }
    hipError_t er = hipHostRegister((void *)pg.p0, pg.p1 - pg.p0, hipHostRegisterDefault);
    bool owned = true;
    if (er == hipErrorHostMemoryAlreadyRegistered) { owned = false; er = hipSuccess; }      // e.g. ntscsim_host_alloc() memory
    (void)hipGetLastError();
    if (er != hipSuccess) { c->err = std::string("hipHostRegister: ") + hipGetErrorString(er); return NTSCSIM_E_HIP; }
    void *dev = nullptr, *dev_last = nullptr;
    if (hipHostGetDevicePointer(&dev, (void *)a0, 0) != hipSuccess || !dev ||
        hipHostGetDevicePointer(&dev_last, (void *)(a1 - 1), 0) != hipSuccess || dev_last != (uint8_t *)dev + (len - 1)) {
        (void)hipGetLastError();
        if (owned) (void)hipHostUnregister((void *)pg.p0);
        c->err = "ntscsim_host_pin: the range is not one registration";
        return NTSCSIM_E_HIP;
    }
    if (owned) c->declared->regs.push_back({pg.p0, pg.p1, (uint8_t *)dev - (a0 - pg.p0), true});
    else c->declared->regs.push_back({a0, a1, (uint8_t *)dev, false});
    return NTSCSIM_OK;
}

extern "C" void *ntscsim_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (bytes == 0) return nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

extern "C" void ntscsim_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

// Planes like av_frame_get_buffer(frame, align) lays them out -- linesize = row bytes rounded up to `align`, every
// plane start aligned, 32 spare rows' worth of padding dropped in favour of `align` + 64 spare bytes per plane -- in
// ONE pinned allocation.
extern "C" int ntscsim_host_frame_alloc(int n_planes, const int *row_bytes, const int *rows, int align,
                                        uint8_t **data, int *linesize, void **base, size_t *bytes)
{
    if (n_planes < 1 || n_planes > 8 || !row_bytes || !rows || !data || !linesize || !base) return NTSCSIM_E_ARG;
    if (align < 1) align = 1;
    if (align & (align - 1)) return NTSCSIM_E_ARG;
    const size_t A = (size_t)(align < 64 ? 64 : align);
    size_t off[8], total = 0;
    for (int k = 0; k < n_planes; k++) {
        if (row_bytes[k] < 1 || rows[k] < 1) return NTSCSIM_E_ARG;
        linesize[k] = (int)(((size_t)row_bytes[k] + (size_t)align - 1) / (size_t)align * (size_t)align);
        off[k] = total;
        total += ((size_t)linesize[k] * (size_t)rows[k] + 64 + A - 1) / A * A;
    }
    uint8_t *p = (uint8_t *)ntscsim_host_alloc(total);
    if (!p) return NTSCSIM_E_NOMEM;
    for (int k = 0; k < n_planes; k++) data[k] = p + off[k];
    *base = p;
    if (bytes) *bytes = total;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_set_pin_policy(ntscsim_ctx *c, int policy)
{
    if (!c || policy < 0 || policy > 2) return NTSCSIM_E_ARG;
    c->pin_policy = policy;
    PinCache *caches[3];
    const int nc = ctx_pin_caches(c, caches);
    for (int k = 0; k < nc; k++) caches[k]->policy = policy;
    return NTSCSIM_OK;
}
