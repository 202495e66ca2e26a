// ntsc_scan.hip -- device half of the scanimate stage (include/ntscsim.h: ntscsim_scan_*): phosphor_dot(),
// scanimate_modify_raster() and composite_layer() of ffmpeg_scanimate.cpp:817-974.  Line numbers refer to that file.
//
// The stage is a scatter: every source sample becomes a dot whose cone is added to a 32-bit accumulator plane at an
// address that depends on the sample's position and on the field's effect.  The accumulator is an integer sum, so the
// adds may happen in any order and in any memory.  k_scan_splat gives a workgroup a tile of the source -- SCAN_LANES
// consecutive samples of a strip of consecutive source rows, lanes along x -- finds the box of destination pixels the
// tile's dots touch in a first pass over the dot centres, sums the dots in an on-chip window over that box with LDS
// adds and flushes the window's non-zero words to the plane with global adds, a row of the window at a time.  Rows of a
// dot that lie below the window (a strip the window cannot hold, the debug cap) are added to the plane directly,
// pixel by pixel: the result never depends on the window fitting.  k_scan_resolve turns the plane into BGRA and
// clears it for the next launch.
//
// Exactness: every fp64 expression keeps the tool's order and association (-ffp-contract=off),
// sqrt / division / floor / ceil are the correctly rounded ones, and no sin / cos runs here: the host computes them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ntscsim.h"
#include "ntsc_frames.hpp"
#include "ntsc_px4.hpp"
#include "ntsc_stage.hpp"

namespace ntscsim {

#define SDEV __device__ __forceinline__

constexpr int SCAN_LANES = 256;          // samples of a source row per workgroup: one per lane
constexpr int SCAN_STRIP_MAX = 16;       // source rows per workgroup at the most
constexpr int SCAN_PLANES = 8;           // accumulator planes of a ctx: output fields in flight
// The window: 48 KiB of the CU's 160 KiB, so that three workgroups are resident whatever the frame width.  A tile of
// 256 samples x 16 rows of the tool's 600 x 800 source lands in about 160 x 15 pixels of a 720 x 480 field (10 KiB).
constexpr int SCAN_WIN_WORDS = 12288;
constexpr int SCAN_RESOLVE_THREADS = 256;
constexpr size_t SCAN_TABLE_SIZES = 4;   // source sizes whose sine-effect tables a ctx keeps

struct ScanRec {                         // one output field
    uint8_t *dst;
    const uint8_t *src;
    uint32_t *acc;                       // the field's accumulator plane, width * height words, zero between launches
    const double *tsin, *tcos;           // effect 3: sin / cos(frame_t * pi * 2 * 6) per source sample, [y][2 * src_w]
    int32_t dst_ls, src_ls, src_w, src_h;
    int32_t effect, field, ystep, y0;    // rows y0, y0 + ystep, ... of the source are drawn :915-924
    int32_t nrows, strip, tiles_x, strips;
    int32_t zero_row0, vec, _pad[2];
    double sigscalxy, radius;            // :928; :936-941 behind the clamp :953
    double ef_t;                         // effect 3: sin(ef_field * pi * 2 / 59.94); effects 0 .. 2: ef_field / 180
    double rot, rot_abs, stretch, trap;  // 1 - 2 ef_t, |1 - 2 ef_t|, 1 + 12 ef_t, 1 - ef_t
};

SDEV double gldd(const double *p) { return *(const PX4_GLOBAL double *)p; }

struct ScanDot { double x, y, sig; };    // phosphor_dot()'s x, y on the screen and signal / dot_radius; sig 0: draws nothing

// what a lane keeps for all rows of its sample x: :931 and the slant :944
struct ScanLane { double sx, slant; };
SDEV ScanLane scan_lane(const ScanRec &r, int x)
{
    const int w2 = r.src_w << 1;
    ScanLane l;
    l.sx = (((double)x * 2) / w2) - 1.0;
    l.slant = (((double)x * r.ystep) / w2) / r.src_h;
    return l;
}

// :931-957 and :822-833 for sample x of source row y.  WITH_SIGNAL false: the position only (sig is 1).
template <bool WITH_SIGNAL>
SDEV ScanDot scan_dot(const ScanRec &r, const ScanLane &l, int x, int y, int W, int H)
{
    double sx = l.sx;
    double sy = (((double)y * 2) / r.src_h) - 1.0;
    sy += l.slant;
    double signal = 1.0;
    if (WITH_SIGNAL) {
        const uint32_t px = gld(r.src + (size_t)y * (size_t)r.src_ls + (size_t)(x >> 1) * 4u);
        signal = ((double)((px >> 8) & 0xFF)) / 255;                             // the green part :947
    }
    switch (r.effect) {
    case 3: {
        const size_t i = (size_t)y * (size_t)(r.src_w << 1) + (size_t)x;
        sx += gldd(r.tsin + i) * r.ef_t * 0.1;
        sy += gldd(r.tcos + i) * r.ef_t * 0.1;
        break;
    }
    case 1:
        sy *= r.rot;
        signal *= r.rot_abs;
        break;
    case 2:
        sy *= r.stretch;
        break;
    default: {
        const double f = (((sy + 1.0) / 2.0) * r.trap) + r.ef_t;
        sx *= f;
        signal *= f;
        break;
    }
    }
    signal *= r.sigscalxy;
    if (signal < 0) signal = 0;
    else if (signal > 32) signal = 32;
    ScanDot d;
    d.x = ((sx + 1.0) * W) / 2;
    d.y = ((sy + 1.0) * H) / 2;
    d.sig = signal / r.radius;           // 0 stays 0: `if (signal == 0) return` :824
    return d;
}

// the dot's box :836-839 cut to the frame; the doubles are cut to +-2^30 first, far outside any frame, so that the
// conversion to int is defined
struct ScanBox { int x0, x1, y0, y1; };
SDEV int scan_int(double v) { return (int)fmin(fmax(v, -1073741824.0), 1073741824.0); }
SDEV ScanBox scan_box(const ScanDot &d, double radius, int W, int H)
{
    ScanBox b;
    b.y0 = max(scan_int(floor(d.y - radius)), 0);
    b.y1 = min(scan_int(floor(d.y + radius)), H - 1);
    b.x0 = max(scan_int(floor(d.x - radius)), 0);
    b.x1 = min(scan_int(ceil(d.x + radius)), W - 1);
    return b;
}

SDEV void scan_add_global(uint32_t *p, uint32_t v)
{
    (void)__hip_atomic_fetch_add((PX4_GLOBAL uint32_t *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // no value comes back
}

// counters[0]: workgroups that drew a dot, counters[1]: those of them that added to the plane directly
__global__ __launch_bounds__(SCAN_LANES) void k_scan_splat(const ScanRec *__restrict__ recs, int W, int H, int win_words,
                                                           int rows_cap, unsigned int *__restrict__ counters)
{
    extern __shared__ uint32_t win[];
    __shared__ int box[4];               // x0, y0 (minima), x1, y1 (maxima) of the tile's dots on the screen
    const ScanRec &r = recs[blockIdx.z];
    if ((int)blockIdx.x >= r.tiles_x || (int)blockIdx.y >= r.strips) return;
    const int tid = threadIdx.x;
    const int x = (int)blockIdx.x * SCAN_LANES + tid;
    const bool on = x < (r.src_w << 1);
    const int k0 = (int)blockIdx.y * r.strip, k1 = min(k0 + r.strip, r.nrows);
    const double radius = r.radius;
    const ScanLane lane = scan_lane(r, on ? x : 0);

    if (tid == 0) { box[0] = W; box[1] = H; box[2] = -1; box[3] = -1; }
    __syncthreads();
    if (on) {
        ScanBox m = {W, -1, H, -1};
        for (int k = k0; k < k1; k++) {
            const ScanBox b = scan_box(scan_dot<false>(r, lane, x, r.y0 + k * r.ystep, W, H), radius, W, H);
            if (b.x0 <= b.x1 && b.y0 <= b.y1) {
                m.x0 = min(m.x0, b.x0); m.x1 = max(m.x1, b.x1);
                m.y0 = min(m.y0, b.y0); m.y1 = max(m.y1, b.y1);
            }
        }
        if (m.x0 <= m.x1) {
            atomicMin(&box[0], m.x0); atomicMin(&box[1], m.y0);
            atomicMax(&box[2], m.x1); atomicMax(&box[3], m.y1);
        }
    }
    __syncthreads();
    const int bx0 = box[0], by0 = box[1], bx1 = box[2], by1 = box[3];
    if (bx0 > bx1 || by0 > by1) return;                                         // the whole tile is off the screen
    const int wc = bx1 - bx0 + 1;                                               // the window: every column of the box ...
    const int wr = min(min(by1 - by0 + 1, rows_cap), win_words / wc);           // ... and as many of its rows as fit
    for (int i = tid; i < wr * wc; i += SCAN_LANES) win[i] = 0;
    __syncthreads();

    bool spilled = false;
    if (on) {
        uint32_t *plane = r.acc;
        for (int k = k0; k < k1; k++) {
            const ScanDot d = scan_dot<true>(r, lane, x, r.y0 + k * r.ystep, W, H);
            if (d.sig == 0) continue;
            const ScanBox b = scan_box(d, radius, W, H);
            // the first pass saw this very box, so its columns are the window's; the test keeps the LDS adds inside
            // the window whatever the first pass found
            const bool cols_in = b.x0 >= bx0 && b.x1 <= bx1;
            for (int iy = b.y0; iy <= b.y1; iy++) {
                const double dy = iy - d.y;
                const double dy2 = dy * dy;
                const bool inwin = cols_in && iy >= by0 && iy - by0 < wr;
                uint32_t *wrow = inwin ? win + (iy - by0) * wc - bx0 : win;     // in the window: below win_words
                uint32_t *prow = plane + (size_t)iy * (size_t)W;
                for (int ix = b.x0; ix <= b.x1; ix++) {
                    const double dx = ix - d.x;
                    const double fv = d.sig * ((radius - sqrt((dx * dx) + dy2)) / radius);    // :845
                    if (fv <= 0) continue;
                    const uint32_t v = (uint32_t)(fv * 255);
                    if (inwin) atomicAdd(wrow + ix, v);
                    else { scan_add_global(prow + ix, v); spilled = true; }
                }
            }
        }
    }
    const int any_spill = __syncthreads_or(spilled ? 1 : 0);
    if (tid == 0) {
        atomicAdd(&counters[0], 1u);
        if (any_spill) atomicAdd(&counters[1], 1u);
    }
    // the flush: a wave takes a row of the window, lanes along the row
    const int wave = tid >> 6, wl = tid & 63;
    for (int row = wave; row < wr; row += SCAN_LANES / 64) {
        uint32_t *prow = r.acc + (size_t)(by0 + row) * (size_t)W + bx0;
        for (int c = wl; c < wc; c += 64) {
            const uint32_t v = win[row * wc + c];
            if (v) scan_add_global(prow + c, v);
        }
    }
}

// :965-971, and the plane cleared behind the read.  One lane = 4 pixels of a row.
__global__ __launch_bounds__(SCAN_RESOLVE_THREADS) void k_scan_resolve(const ScanRec *__restrict__ recs, int W, int H)
{
    const ScanRec &r = recs[blockIdx.y];
    const int Q = (W + 3) >> 2, total = Q * H;
    const bool accvec = (W & 3) == 0;
    for (int item = blockIdx.x * SCAN_RESOLVE_THREADS + threadIdx.x; item < total; item += gridDim.x * SCAN_RESOLVE_THREADS) {
        const int y = item / Q, x = (item - y * Q) << 2;
        const int npx = W - x < 4 ? W - x : 4;
        uint8_t *ap = reinterpret_cast<uint8_t *>(r.acc + (size_t)y * (size_t)W + (size_t)x);
        uint32_t a[4];
        const uint32_t zero[4] = {0, 0, 0, 0};
        if (accvec) { px4_load<true>(a, ap, 4); px4_store<true>(ap, zero, 4); }
        else { px4_load<false>(a, ap, npx); px4_store<false>(ap, zero, npx); }
        if (y < r.field && !r.zero_row0) continue;                              // row 0 of a field == 1 frame is the caller's
        uint32_t o[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const uint32_t g = min(a[p] >> 1, 255u);
            o[p] = y < r.field ? 0u : 0xFF000000u + g * 0x010101u;
        }
        uint8_t *dp = r.dst + (size_t)y * (size_t)r.dst_ls + (size_t)x * 4u;
        if (r.vec && npx == 4) px4_store<true>(dp, o, 4);
        else px4_store<false>(dp, o, npx);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------

struct ScanTables {                      // effect 3, per source size
    int sw = 0, sh = 0;
    uint64_t group = 0;                  // the launch that used it last (ScanState::group)
    double *tsin = nullptr, *tcos = nullptr;
};

struct ScanState {
    ntscsim_scan_params prm;
    RecordSlots<> slots;
    FrameArena frames;                   // ntscsim_scan_frames_host()
    uint32_t *plane[SCAN_PLANES] = {};
    size_t plane_words = 0;
    uint32_t *kept = nullptr;            // ntscsim_scan_debug_raster()
    bool keep = false, have_kept = false;
    int kept_w = 0, kept_h = 0;
    int rows_cap = INT32_MAX;            // ntscsim_scan_debug_set_window_rows()
    unsigned int *counters = nullptr;
    std::vector<ScanTables> tables;
    uint64_t group = 0;                  // counts the launches: scan_launch()
    hipEvent_t tail = nullptr;           // behind the last launch: the planes are shared by every stream the caller uses
    hipStream_t tail_stream = nullptr;
    bool tail_used = false;
};

static void scan_free_planes(ScanState *k)
{
    for (uint32_t *&p : k->plane) { if (p) (void)hipFree(p); p = nullptr; }
    if (k->kept) { (void)hipFree(k->kept); k->kept = nullptr; }
    k->have_kept = false;
    k->plane_words = 0;
}

void scan_state_destroy(ScanState *k)
{
    if (!k) return;
    scan_free_planes(k);
    if (k->counters) (void)hipFree(k->counters);
    for (ScanTables &t : k->tables) { (void)hipFree(t.tsin); (void)hipFree(t.tcos); }
    if (k->tail) (void)hipEventDestroy(k->tail);
    k->slots.release();
    k->frames.release();
    delete k;
}

// ntscsim_debug_last_kernels(): the splat kernel's counter decides between k_scan_splat and k_scan_splat+spill
void scan_kernels_tap(ScanState *k, int device, std::string &kernels)
{
    const std::string name = "k_scan_splat";
    if (!k || !k->counters || kernels.find(name) == std::string::npos) return;
    unsigned int c[2] = {0, 0};
    if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return;
    if (hipMemcpy(c, k->counters, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess || c[1] == 0) return;
    for (size_t at = kernels.find(name); at != std::string::npos; at = kernels.find(name, at + name.size() + 6))
        kernels.insert(at + name.size(), "+spill");
}

} // namespace ntscsim

using namespace ntscsim;

namespace {

bool scan_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= (1 << 16) && h <= (1 << 16); }
bool scan_src_ok(int w, int h) { return scan_size_ok(w, h) && 2ull * (uint64_t)w * (uint64_t)h < (1ull << 31); }

// aligned: a device call; a host frame may lie anywhere and have any linesize that holds a row
int scan_check_desc(const ScanState *k, const ntscsim_scan_desc &d, bool aligned)
{
    const int W = k->prm.output_width, H = k->prm.output_height;
    if (!d.dst_dev || !d.src_dev) return NTSCSIM_E_ARG;
    if (!scan_src_ok(d.src_width, d.src_height)) return NTSCSIM_E_SIZE;
    if (plane_check(d.dst_dev, d.dst_linesize, W, aligned)) return NTSCSIM_E_SIZE;
    if (plane_check(d.src_dev, d.src_linesize, d.src_width, aligned)) return NTSCSIM_E_SIZE;
    if (overlaps(span_of(d.dst_dev, d.dst_linesize, H), span_of(d.src_dev, d.src_linesize, d.src_height))) return NTSCSIM_E_ARG;
    return NTSCSIM_OK;
}

// effect 3: the two tables of a source size, computed with the host's libm when first asked for.  The cache keeps
// SCAN_TABLE_SIZES sizes and drops the one not used for longest -- but never one that a record of the launch being built
// (k->group) points at: with more sizes than that in one launch the cache grows for the launch and shrinks at a later miss.
int scan_tables(const CtxStageView &v, ScanState *k, int sw, int sh, const double *&tsin, const double *&tcos)
{
    for (ScanTables &t : k->tables)
        if (t.sw == sw && t.sh == sh) { t.group = k->group; tsin = t.tsin; tcos = t.tcos; return NTSCSIM_OK; }
    while (k->tables.size() >= SCAN_TABLE_SIZES) {
        size_t old = k->tables.size();
        for (size_t i = 0; i < k->tables.size(); i++)
            if (k->tables[i].group != k->group && (old == k->tables.size() || k->tables[i].group < k->tables[old].group)) old = i;
        if (old == k->tables.size()) break;                                     // every one is this launch's
        const int rc = k->slots.wait_all(v);                                    // launches in flight may read it
        if (rc != NTSCSIM_OK) return rc;
        (void)hipFree(k->tables[old].tsin);
        (void)hipFree(k->tables[old].tcos);
        k->tables.erase(k->tables.begin() + (std::ptrdiff_t)old);
    }
    const size_t n = 2 * (size_t)sw * (size_t)sh;
    std::vector<double> hs, hc;
    try { hs.resize(n); hc.resize(n); } catch (const std::bad_alloc &) { return NTSCSIM_E_NOMEM; }
    const int den = sw * sh * 2;                                                // :949, an int in the tool
    for (size_t i = 0; i < n; i++) {
        const double frame_t = ((double)(unsigned int)i) / den;
        hs[i] = std::sin(frame_t * M_PI * 2 * 6);                               // :872-873
        hc[i] = std::cos(frame_t * M_PI * 2 * 6);
    }
    ScanTables t;
    t.sw = sw; t.sh = sh; t.group = k->group;
    hipError_t e = hipMalloc((void **)&t.tsin, n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&t.tcos, n * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(t.tsin, hs.data(), n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t.tcos, hc.data(), n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {                                                      // nothing half-made stays in the cache
        if (t.tsin) (void)hipFree(t.tsin);
        if (t.tcos) (void)hipFree(t.tcos);
        *v.err = std::string("scan tables: ") + hipGetErrorString(e);
        return NTSCSIM_E_HIP;
    }
    k->tables.push_back(t);
    tsin = t.tsin; tcos = t.tcos;
    return NTSCSIM_OK;
}

// the record of one field: the per-field scalars :865-887 and the tile grid
int scan_fill(const CtxStageView &v, ScanState *k, const ntscsim_scan_desc &d, uint32_t *plane, bool zero_row0, ScanRec &r)
{
    const int W = k->prm.output_width, H = k->prm.output_height;
    const bool ntsc = k->prm.input_ntsc != 0;
    std::memset(&r, 0, sizeof(r));
    r.dst = static_cast<uint8_t *>(d.dst_dev);
    r.src = static_cast<const uint8_t *>(d.src_dev);
    r.acc = plane;
    r.dst_ls = d.dst_linesize; r.src_ls = d.src_linesize; r.src_w = d.src_width; r.src_h = d.src_height;
    uint32_t effect, ef_field;
    ntscsim_scan_effect(d.fieldno, &effect, &ef_field);
    r.effect = (int32_t)effect;
    r.field = (int32_t)ntscsim_scan_field_of(d.fieldno);
    r.ystep = ntsc ? 2 : 1;
    r.y0 = ntsc ? r.field : 0;
    r.nrows = ntsc ? (r.src_h > r.y0 ? (r.src_h - r.y0 + 1) / 2 : 0) : r.src_h;
    r.zero_row0 = zero_row0 ? 1 : 0;
    r.vec = (((uintptr_t)d.dst_dev | (uintptr_t)d.dst_linesize) & 15) == 0;
    r.sigscalxy = ((double)W / r.src_w) * ((double)H / r.src_h) * 0.9;         // :928
    r.radius = ((double)H * (ntsc ? 2.05 : 1.05)) / r.src_h;                    // :936-941
    if (r.radius < 1.2) r.radius = 1.2;                                         // :953
    double vscale = 1.0, xshift = 0.0;                                          // of the picture on the screen, for the strip below
    if (effect == 3) {
        r.ef_t = std::sin(((double)ef_field * M_PI * 2) / (59.94 * 1));         // :871
        const int rc = scan_tables(v, k, r.src_w, r.src_h, r.tsin, r.tcos);
        if (rc != NTSCSIM_OK) return rc;
        xshift = 0.1 * std::fabs(r.ef_t);
    } else {
        r.ef_t = (double)ef_field / (60 * 3);
        r.rot = 1.0 - (r.ef_t * 2.0);                                           // :877
        r.rot_abs = std::fabs(1.0 - (r.ef_t * 2.0));                            // :878
        r.stretch = 1.0 + (r.ef_t * 12);                                        // :882
        r.trap = 1.0 - r.ef_t;                                                  // :886
        if (effect == 1) vscale = r.rot_abs;
        if (effect == 2) vscale = r.stretch;
    }
    // the strip: as many source rows as the window holds of the tile's destination rows, estimated; the kernel
    // measures the box itself and is right whatever this says
    const double cols = (double)SCAN_LANES * W / (2.0 * r.src_w) + 2 * r.radius + 3 + xshift * W;
    const double rows_fit = (double)SCAN_WIN_WORDS / std::min(cols, (double)W + 1);
    const double pitch = (double)r.ystep * H / r.src_h * vscale;                 // destination rows per source row drawn
    const double halo = 2 * r.radius + 3 + xshift * H;
    double s = pitch > 0 ? (rows_fit - halo) / pitch : (double)SCAN_STRIP_MAX;
    if (!(s >= 1)) s = 1;
    r.strip = (int32_t)std::min(s, (double)SCAN_STRIP_MAX);
    r.tiles_x = (2 * r.src_w + SCAN_LANES - 1) / SCAN_LANES;
    r.strips = (r.nrows + r.strip - 1) / r.strip;
    return NTSCSIM_OK;
}

int scan_planes(const CtxStageView &v, ScanState *k, int m)
{
    const size_t words = (size_t)k->prm.output_width * (size_t)k->prm.output_height;
    for (int i = 0; i < m; i++) {
        if (k->plane[i]) continue;
        STAGECHK(v, hipMalloc((void **)&k->plane[i], words * sizeof(uint32_t)));
        STAGECHK(v, hipMemset(k->plane[i], 0, words * sizeof(uint32_t)));
    }
    k->plane_words = words;
    if (k->keep && !k->kept) STAGECHK(v, hipMalloc((void **)&k->kept, words * sizeof(uint32_t)));
    if (!k->counters) {
        STAGECHK(v, hipMalloc((void **)&k->counters, 2 * sizeof(unsigned int)));
        STAGECHK(v, hipMemset(k->counters, 0, 2 * sizeof(unsigned int)));
    }
    return NTSCSIM_OK;
}

// one launch pair over up to SCAN_PLANES descriptors that do not depend on each other
int scan_launch(ntscsim_ctx *c, const ntscsim_scan_desc *descs, int m, bool zero_row0, bool last_of_call, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    ScanState *k = *v.scan;
    const int W = k->prm.output_width, H = k->prm.output_height;
    int rc = scan_planes(v, k, m);
    if (rc != NTSCSIM_OK) return rc;
    RecordSlot *slot = nullptr;
    rc = k->slots.acquire(v, (size_t)m * sizeof(ScanRec), slot);
    if (rc != NTSCSIM_OK) return rc;
    RecordSlot &s = *slot;
    ScanRec *recs = reinterpret_cast<ScanRec *>(s.host);
    k->group++;                                                                 // the tables its records point at stay (scan_tables())
    int tiles = 1, strips = 1;
    for (int i = 0; i < m; i++) {
        rc = scan_fill(v, k, descs[i], k->plane[i], zero_row0, recs[i]);
        if (rc != NTSCSIM_OK) return rc;
        tiles = std::max(tiles, recs[i].tiles_x);
        strips = std::max(strips, recs[i].strips);
    }
    STAGECHK(v, hipMemcpyAsync(s.dev, s.host, (size_t)m * sizeof(ScanRec), hipMemcpyHostToDevice, st));
    const ScanRec *recs_dev = reinterpret_cast<const ScanRec *>(s.dev);
    hipLaunchKernelGGL(k_scan_splat, dim3((unsigned)tiles, (unsigned)strips, (unsigned)m), dim3(SCAN_LANES),
                       SCAN_WIN_WORDS * sizeof(uint32_t), st, recs_dev, W, H, SCAN_WIN_WORDS, k->rows_cap, k->counters);
    STAGECHK(v, hipGetLastError());
    if (k->keep && last_of_call) {
        STAGECHK(v, hipMemcpyAsync(k->kept, k->plane[m - 1], k->plane_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        k->have_kept = true; k->kept_w = W; k->kept_h = H;
    }
    const long long quads = (long long)((W + 3) / 4) * H;
    const long long per = std::max(1LL, std::min((quads + SCAN_RESOLVE_THREADS - 1) / SCAN_RESOLVE_THREADS, (2048LL + m - 1) / m));
    hipLaunchKernelGGL(k_scan_resolve, dim3((unsigned)per, (unsigned)m), dim3(SCAN_RESOLVE_THREADS), 0, st, recs_dev, W, H);
    STAGECHK(v, hipGetLastError());
    STAGECHK(v, hipEventRecord(k->tail, st));                                   // in front of the slot's: a failure of either leaves no name
    k->tail_used = true;
    k->tail_stream = st;
    return stage_launched(v, &s, st, "k_scan_splat;k_scan_resolve");
}

// every descriptor checked, then launches of at most SCAN_PLANES descriptors, cut where descriptors depend on each
// other: they take effect in order (frames_in_order())
int scan_frames(ntscsim_ctx *c, const ntscsim_scan_desc *descs, int n, bool zero_row0, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    ScanState *k = *v.scan;
    const int H = k->prm.output_height;
    for (int i = 0; i < n; i++) {
        const int rc = scan_check_desc(k, descs[i], true);
        if (rc != NTSCSIM_OK) return rc;
    }
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    if (n == 0) return NTSCSIM_OK;
    if (!k->tail) STAGECHK(v, hipEventCreateWithFlags(&k->tail, hipEventDisableTiming));
    if (k->tail_used && k->tail_stream != st) STAGECHK(v, hipStreamWaitEvent(st, k->tail, 0));
    int rc = scan_planes(v, k, 1);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemsetAsync(k->counters, 0, 2 * sizeof(unsigned int), st));
    return frames_in_order(n, SCAN_PLANES, [&](int i, std::vector<Span> &rd) {
        rd.push_back(span_of(descs[i].src_dev, descs[i].src_linesize, descs[i].src_height));
        return span_of(descs[i].dst_dev, descs[i].dst_linesize, H);
    }, [&](int first, int m) { return scan_launch(c, descs + first, m, zero_row0, first + m == n, st); });
}

ScanState *scan_state(ntscsim_ctx *c) { return c ? *ctx_stage_view(c).scan : nullptr; }

} // namespace

extern "C" int ntscsim_scan_bind(ntscsim_ctx *c, const ntscsim_scan_params *p)
{
    if (!c || !p || p->struct_size != sizeof(*p)) return NTSCSIM_E_ARG;
    if (!scan_size_ok(p->output_width, p->output_height) ||
        (uint64_t)p->output_width * (uint64_t)p->output_height >= (1ull << 31)) return NTSCSIM_E_SIZE;
    if (!scan_src_ok(p->src_width, p->src_height)) return NTSCSIM_E_SIZE;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    ScanState *k = *v.scan;
    if (!k) {
        k = new (std::nothrow) ScanState();
        if (!k) return NTSCSIM_E_NOMEM;
        *v.scan = k;
    }
    const int rc = k->slots.wait_all(v);                                        // launches in flight use the planes
    if (rc != NTSCSIM_OK) return rc;
    if ((size_t)p->output_width * (size_t)p->output_height != k->plane_words) scan_free_planes(k);
    k->prm = *p;
    k->prm.last_input_path = nullptr;
    k->prm.output_path = nullptr;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_scan_frames_device(ntscsim_ctx *c, const ntscsim_scan_desc *descs, int n, void *hip_stream)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    if (!*v.scan) return NTSCSIM_E_ARG;                                         // ntscsim_scan_bind() first
    return scan_frames(c, descs, n, false, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
}

extern "C" int ntscsim_scan_clip_device(ntscsim_ctx *c, const void *const *src_dev, int src_linesize, int src_w, int src_h,
                                        void *const *out_dev, int out_linesize, int T, uint64_t *fieldno, void *hip_stream)
{
    if (!c || !fieldno || T < 0 || (T > 0 && (!src_dev || !out_dev))) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    ScanState *k = *v.scan;
    if (!k) return NTSCSIM_E_ARG;
    if (T > (1 << 24)) return NTSCSIM_E_SIZE;
    const int H = k->prm.output_height;
    std::vector<ntscsim_scan_desc> descs((size_t)T);
    CallWrites wr;
    for (int t = 0; t < T; t++) {
        ntscsim_scan_desc &d = descs[(size_t)t];
        d.dst_dev = out_dev[t]; d.dst_linesize = out_linesize;
        d.src_dev = src_dev[t]; d.src_linesize = src_linesize; d.src_width = src_w; d.src_height = src_h;
        d.fieldno = *fieldno + (uint64_t)t;
        const int rc = scan_check_desc(k, d, true);
        if (rc != NTSCSIM_OK) return rc;
        wr.add(span_of(d.dst_dev, d.dst_linesize, H));
    }
    // the outputs must be disjoint from each other and from every source
    if (wr.sort() != NTSCSIM_OK) return NTSCSIM_E_ARG;
    for (int t = 0; t < T; t++)
        if (wr.hits(span_of(src_dev[t], src_linesize, src_h))) return NTSCSIM_E_ARG;
    const int rc = scan_frames(c, descs.data(), T, true, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
    if (rc != NTSCSIM_OK) return rc;
    *fieldno += (uint64_t)T;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_scan_frames_host(ntscsim_ctx *c, const ntscsim_scan_desc *descs, int n)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    ScanState *k = *v.scan;
    if (!k) return NTSCSIM_E_ARG;
    const int W = k->prm.output_width, H = k->prm.output_height;
    for (int i = 0; i < n; i++) {
        const int rc = scan_check_desc(k, descs[i], false);
        if (rc != NTSCSIM_OK) return rc;
    }
    STAGECHK(v, hipSetDevice(v.device));
    // one descriptor at a time through the arena: destination | source, rows packed to a 16-byte pitch, the
    // destination up as well as down because the device call leaves row 0 of a field == 1 frame alone
    hipStream_t st = v.stream;
    const size_t drow = (size_t)W * 4, dpitch = (drow + 15) & ~(size_t)15, dbytes = dpitch * (size_t)H;
    for (int i = 0; i < n; i++) {
        const ntscsim_scan_desc &d = descs[i];
        const size_t srow = (size_t)d.src_width * 4, spitch = (srow + 15) & ~(size_t)15, sbytes = spitch * (size_t)d.src_height;
        const int rc = k->frames.reserve(v, dbytes + sbytes, dbytes + sbytes);
        if (rc != NTSCSIM_OK) return rc;
        unsigned char *stage = k->frames.staging, *arena = k->frames.arena;
        copy_rows(stage, dpitch, d.dst_dev, (size_t)d.dst_linesize, drow, H);
        copy_rows(stage + dbytes, spitch, d.src_dev, (size_t)d.src_linesize, srow, d.src_height);
        STAGECHK(v, hipMemcpyAsync(arena, stage, dbytes + sbytes, hipMemcpyHostToDevice, st));
        ntscsim_scan_desc dd = d;
        dd.dst_dev = arena; dd.dst_linesize = (int)dpitch;
        dd.src_dev = arena + dbytes; dd.src_linesize = (int)spitch;
        const int rc2 = scan_frames(c, &dd, 1, false, st);
        if (rc2 != NTSCSIM_OK) return rc2;
        STAGECHK(v, hipMemcpyAsync(stage, arena, dbytes, hipMemcpyDeviceToHost, st));
        STAGECHK(v, hipStreamSynchronize(st));
        copy_rows(d.dst_dev, (size_t)d.dst_linesize, stage, dpitch, drow, H);
    }
    return NTSCSIM_OK;
}

extern "C" int ntscsim_scan_debug_keep_raster(ntscsim_ctx *c, int on)
{
    ScanState *k = scan_state(c);
    if (!k) return NTSCSIM_E_ARG;
    k->keep = on != 0;
    if (!k->keep) k->have_kept = false;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_scan_debug_raster(ntscsim_ctx *c, uint32_t *out_host)
{
    ScanState *k = scan_state(c);
    if (!k || !out_host || !k->have_kept || !k->kept) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    STAGECHK(v, hipDeviceSynchronize());
    STAGECHK(v, hipMemcpy(out_host, k->kept, (size_t)k->kept_w * (size_t)k->kept_h * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NTSCSIM_OK;
}

extern "C" int ntscsim_scan_debug_set_window_rows(ntscsim_ctx *c, int rows)
{
    ScanState *k = scan_state(c);
    if (!k) return NTSCSIM_E_ARG;
    k->rows_cap = rows < 0 ? INT32_MAX : rows;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_scan_debug_spill(ntscsim_ctx *c, uint64_t *workgroups, uint64_t *spilled)
{
    ScanState *k = scan_state(c);
    if (!k || !workgroups || !spilled) return NTSCSIM_E_ARG;
    *workgroups = *spilled = 0;
    if (!k->counters) return NTSCSIM_OK;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    STAGECHK(v, hipDeviceSynchronize());
    unsigned int cnt[2] = {0, 0};
    STAGECHK(v, hipMemcpy(cnt, k->counters, sizeof(cnt), hipMemcpyDeviceToHost));
    *workgroups = cnt[0];
    *spilled = cnt[1];
    return NTSCSIM_OK;
}
