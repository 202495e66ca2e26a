// layer_host_check.cpp -- drives csrc/ntsc_layer.hpp (the host logic the colorkey and average_delay stages share) without
// a GPU: plain C++ with its own main, compiled and run by tests/test_layer_host.py.  Frame "pointers" are numbers: nothing
// here reads a frame.  Prints one line per failed check and returns their count.
#include <cstdio>
#include <vector>

#include "ntsc_layer.hpp"

using namespace ntscsim;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

static const int W = 10, H = 6, LS = 4 * W, FRAME = LS * H;       // 240-byte frames
static void *frame(int k) { return reinterpret_cast<void *>((uintptr_t)0x100000 + (uintptr_t)k * 0x1000); }
static void *at(void *p, long off) { return reinterpret_cast<void *>((uintptr_t)p + off); }

template <class Desc>
struct Call {                            // descriptors of one call, each with nl layers
    int nl;
    std::vector<Desc> d;
    std::vector<std::vector<LayerSrcOf<Desc>>> l;
    explicit Call(int nl_) : nl(nl_) {}
    void add(void *dst, std::vector<const void *> srcs, int dst_ls = LS, int src_ls = LS)
    {
        std::vector<LayerSrcOf<Desc>> s;
        for (const void *p : srcs) { LayerSrcOf<Desc> e = LayerSrcOf<Desc>(); e.src_dev = p; e.src_linesize = src_ls; s.push_back(e); }
        l.push_back(s);
        Desc x = Desc();
        x.dst_dev = dst; x.dst_linesize = dst_ls; x.width = W; x.height = H; x.n_layers = (int)srcs.size();
        d.push_back(x);
    }
    const Desc *descs() { for (size_t i = 0; i < d.size(); i++) d[i].layers = l[i].data(); return d.data(); }
    int n() const { return (int)d.size(); }
};

typedef std::vector<std::pair<int, int>> Runs;                     // (index of first descriptor, count) per launch

template <class Desc>
static int plan(Call<Desc> &c, int cap, Runs &runs, int fail_at = -1)
{
    runs.clear();
    const Desc *base = c.descs();
    return layer_frames_in_order(LayerGeom{W, H, c.nl}, base, c.n(), cap, [&](const Desc *d, int m) {
        runs.push_back({(int)(d - base), m});
        return (int)runs.size() - 1 == fail_at ? NTSCSIM_E_HIP : NTSCSIM_OK;
    });
}

template <class Desc>
static void planner_checks()
{
    Runs r;
    { Call<Desc> c(1); CHECK(plan(c, 65535, r) == NTSCSIM_OK && r.empty()); }                    // n = 0
    {   // independent descriptors: one launch; the cap of 1: one launch each
        Call<Desc> c(1);
        for (int i = 0; i < 3; i++) c.add(frame(2 * i), {frame(2 * i + 1)});
        CHECK(plan(c, 65535, r) == NTSCSIM_OK && r == Runs({{0, 3}}));
        CHECK(plan(c, 2, r) == NTSCSIM_OK && r == Runs({{0, 2}, {2, 1}}));
        CHECK(plan(c, 1, r) == NTSCSIM_OK && r == Runs({{0, 1}, {1, 1}, {2, 1}}));
        CHECK(plan(c, 1, r, 1) == NTSCSIM_E_HIP && r.size() == 2);                                 // a failed launch ends the call
    }
    {   // a destination that a later descriptor reads
        Call<Desc> c(1);
        c.add(frame(0), {frame(1)}); c.add(frame(2), {frame(3)}); c.add(frame(4), {frame(0)}); c.add(frame(5), {frame(1)});
        CHECK(plan(c, 65535, r) == NTSCSIM_OK && r == Runs({{0, 2}, {2, 2}}));
    }
    {   // a destination written twice; a source written later; overlap by the last row only
        Call<Desc> c(1);
        c.add(frame(0), {frame(1)}); c.add(frame(0), {frame(1)});
        CHECK(plan(c, 65535, r) == NTSCSIM_OK && r == Runs({{0, 1}, {1, 1}}));
        Call<Desc> e(1);
        e.add(frame(0), {frame(1)}); e.add(frame(1), {frame(2)});
        CHECK(plan(e, 65535, r) == NTSCSIM_OK && r == Runs({{0, 1}, {1, 1}}));
        Call<Desc> f(1);
        f.add(frame(0), {frame(1)}); f.add(at(frame(0), FRAME - 4), {frame(2)}); f.add(at(frame(0), 2 * FRAME - 8), {nullptr});
        CHECK(plan(f, 65535, r) == NTSCSIM_OK && r == Runs({{0, 1}, {1, 1}, {2, 1}}));
        Call<Desc> g(1);                                                                             // touching is not overlapping
        g.add(frame(0), {frame(1)}); g.add(at(frame(0), FRAME), {nullptr});
        CHECK(plan(g, 65535, r) == NTSCSIM_OK && r == Runs({{0, 2}}));
    }
    {   // check_desc: nothing is launched when any descriptor is refused
        Call<Desc> a(1); a.add(frame(0), {frame(1)}); a.add(nullptr, {frame(1)});
        CHECK(plan(a, 65535, r) == NTSCSIM_E_ARG && r.empty());
        Call<Desc> b(1); b.add(frame(0), {at(frame(0), FRAME - 4)});                                 // a source over its own destination
        CHECK(plan(b, 65535, r) == NTSCSIM_E_ARG && r.empty());
        Call<Desc> c(1); c.add(frame(0), {frame(1)}, LS - 4);
        CHECK(plan(c, 65535, r) == NTSCSIM_E_SIZE);
        Call<Desc> d(1); d.add(frame(0), {frame(1)}, LS, LS + 2);
        CHECK(plan(d, 65535, r) == NTSCSIM_E_SIZE);
        Call<Desc> e(1); e.add(at(frame(0), 2), {frame(1)});
        CHECK(plan(e, 65535, r) == NTSCSIM_E_SIZE);
        Call<Desc> f(1); f.add(frame(0), {at(frame(1), 1)});
        CHECK(plan(f, 65535, r) == NTSCSIM_E_SIZE);
        Call<Desc> g(2); g.add(frame(0), {frame(1)});                                                // not the bound layer count
        CHECK(plan(g, 65535, r) == NTSCSIM_E_SIZE);
        Call<Desc> h(1); h.add(frame(0), {nullptr}, LS, 0);                                          // an absent layer's linesize is not looked at
        CHECK(plan(h, 65535, r) == NTSCSIM_OK && r == Runs({{0, 1}}));
    }
}

template <class Desc>
static void clip_checks()
{
    const LayerGeom g{W, H, 2};
    const int delay = 2, T = 3;
    void *ring[2] = {frame(0), frame(1)};
    void *out[3] = {frame(2), frame(3), frame(4)};
    const void *src[6] = {frame(10), nullptr, frame(12), nullptr, nullptr, nullptr};                 // [layer * T + t]; layer 1 never present
    int32_t ls[2] = {LS, LS};
    std::vector<Desc> descs;
    std::vector<LayerSrcOf<Desc>> lays;
    auto run = [&](bool every) { return layer_clip_descs(g, delay, ring, LS, src, ls, out, LS, T, every, descs, lays); };
    CHECK(run(false) == NTSCSIM_OK && descs.size() == 3 && lays.size() == 6);
    for (int t = 0; t < T && descs.size() == 3; t++) {
        CHECK(descs[t].dst_dev == out[t] && descs[t].dst_linesize == LS && descs[t].width == W && descs[t].height == H);
        CHECK(descs[t].n_layers == 2 && descs[t].layers == lays.data() + 2 * t);
        CHECK(lays[2 * t].src_dev == src[t] && lays[2 * t + 1].src_dev == nullptr && lays[2 * t].src_linesize == LS);
    }
    CHECK(layer_clip_descs(g, delay, ring, LS, src, ls, out, LS, 0, true, descs, lays) == NTSCSIM_OK && descs.empty());   // T = 0
    // the linesize of a layer that is absent in every frame: refused only where every linesize is checked up front
    ls[1] = LS - 4;
    CHECK(run(false) == NTSCSIM_OK);
    CHECK(run(true) == NTSCSIM_E_SIZE);
    ls[1] = LS;
    ls[0] = LS + 2;
    CHECK(run(false) == NTSCSIM_E_SIZE && run(true) == NTSCSIM_E_SIZE);
    ls[0] = LS;
    // a source over an output by its last dword (pointers are 4-aligned, so no overlap is smaller), and one that only touches
    src[2] = at(out[1], -(long)FRAME + 4);
    CHECK(run(false) == NTSCSIM_E_ARG && run(true) == NTSCSIM_E_ARG);
    src[2] = at(out[1], -(long)FRAME);
    CHECK(run(false) == NTSCSIM_OK);
    src[2] = at(ring[1], FRAME - 4);                                                                 // over the ring's last dword
    CHECK(run(false) == NTSCSIM_E_ARG);
    src[2] = at(frame(12), 1);
    CHECK(run(false) == NTSCSIM_E_SIZE);
    src[2] = frame(12);
    // what the call writes overlaps itself
    out[2] = out[0];
    CHECK(run(false) == NTSCSIM_E_ARG);
    out[2] = at(ring[0], FRAME - 4);
    CHECK(run(false) == NTSCSIM_E_ARG);
    out[2] = nullptr;
    CHECK(run(false) == NTSCSIM_E_ARG);
    out[2] = at(frame(4), 2);
    CHECK(run(false) == NTSCSIM_E_SIZE);
    out[2] = frame(4);
    ring[1] = nullptr;
    CHECK(run(false) == NTSCSIM_E_ARG);
    ring[1] = frame(1);
    CHECK(layer_clip_descs(g, delay, ring, LS - 4, src, ls, out, LS, T, false, descs, lays) == NTSCSIM_E_SIZE);
    CHECK(layer_clip_descs(g, delay, ring, LS, src, ls, out, LS + 1, T, false, descs, lays) == NTSCSIM_E_SIZE);
    CHECK(run(true) == NTSCSIM_OK);
}

template <class Desc>
static void host_checks()
{
    const LayerGeom g{W, H, 2};
    const size_t pitch = 48, fb = pitch * H;                                                         // 40 bytes of pixels -> 16-byte pitch
    { HostFrames p; Call<Desc> c(2); CHECK(host_frames_plan(g, c.descs(), 0, p) == NTSCSIM_OK && p.order.empty() && p.dsts.empty()); }   // n = 0
    {   // one frame under two roles is one frame; any linesize goes, aligned or not
        Call<Desc> c(2);
        c.add(frame(0), {frame(1), nullptr});
        c.add(frame(2), {frame(0), frame(1)});
        c.add(frame(0), {nullptr, at(frame(3), 1)}, LS, LS + 3);
        HostFrames p;
        CHECK(host_frames_plan(g, c.descs(), c.n(), p) == NTSCSIM_OK);
        CHECK(p.pitch == pitch && p.fb == fb && p.order.size() == 4 && p.dsts.size() == 2);
        CHECK(p.dsts == std::vector<HostFrame>({{frame(0), LS}, {frame(2), LS}}));
        for (size_t i = 0; i < p.order.size(); i++) CHECK(p.where.at(p.order[i]) == i * fb);
        unsigned char *arena = reinterpret_cast<unsigned char *>((uintptr_t)0x40000000);
        std::vector<Desc> dd;
        std::vector<LayerSrcOf<Desc>> ll;
        host_frames_rebase(p, arena, c.descs(), c.n(), dd, ll);
        CHECK(dd.size() == 3 && ll.size() == 6);
        if (dd.size() == 3 && ll.size() == 6) {
            CHECK(dd[0].dst_dev == arena && dd[2].dst_dev == arena && dd[1].dst_dev == arena + 2 * fb);
            CHECK(dd[1].layers == ll.data() + 2 && dd[1].layers[0].src_dev == arena && dd[1].layers[1].src_dev == arena + fb);
            CHECK(dd[0].layers[1].src_dev == nullptr && dd[2].layers[1].src_dev == arena + 3 * fb);
            CHECK(dd[2].dst_linesize == (int)pitch && dd[2].layers[1].src_linesize == (int)pitch && dd[2].n_layers == 2);
        }
    }
    {   // two host frames that share memory without being the same (pointer, linesize): refused when one is written
        HostFrames p, q, r, s, t;
        Call<Desc> a(2); a.add(frame(0), {at(frame(0), FRAME - 1), nullptr});                        // by one byte
        CHECK(host_frames_plan(g, a.descs(), a.n(), p) == NTSCSIM_E_ARG);
        Call<Desc> b(2); b.add(frame(0), {at(frame(0), FRAME), nullptr});                            // touching
        CHECK(host_frames_plan(g, b.descs(), b.n(), q) == NTSCSIM_OK);
        Call<Desc> c(2); c.add(frame(0), {frame(1), nullptr}); c.add(frame(2), {frame(0), nullptr}, LS, LS + 4);   // same pointer, other linesize
        CHECK(host_frames_plan(g, c.descs(), c.n(), r) == NTSCSIM_E_ARG);
        Call<Desc> d(2); d.add(frame(0), {frame(1), at(frame(1), 8)});                               // two sources may overlap
        CHECK(host_frames_plan(g, d.descs(), d.n(), s) == NTSCSIM_OK && s.order.size() == 3);
        Call<Desc> e(2); e.add(frame(0), {frame(1), nullptr}); e.add(at(frame(0), FRAME - 1), {frame(1), nullptr});   // two destinations
        CHECK(host_frames_plan(g, e.descs(), e.n(), t) == NTSCSIM_E_ARG);
    }
    {
        HostFrames p, q, r;
        Call<Desc> a(2); a.add(nullptr, {frame(1), nullptr});
        CHECK(host_frames_plan(g, a.descs(), a.n(), p) == NTSCSIM_E_ARG);
        Call<Desc> b(2); b.add(frame(0), {frame(1), nullptr}, LS - 1);
        CHECK(host_frames_plan(g, b.descs(), b.n(), q) == NTSCSIM_E_SIZE);
        Call<Desc> c(2); c.add(frame(0), {frame(1), nullptr}, LS, LS - 1);
        CHECK(host_frames_plan(g, c.descs(), c.n(), r) == NTSCSIM_E_SIZE);
    }
}

int main()
{
    CHECK(overlaps(Span{0, 4}, Span{3, 8}) && !overlaps(Span{0, 4}, Span{4, 8}) && !overlaps(Span{4, 8}, Span{0, 4}));
    CHECK(span_of(frame(0), LS, H).b - span_of(frame(0), LS, H).a == (uintptr_t)FRAME);
    planner_checks<ntscsim_key_desc>();
    planner_checks<ntscsim_avg_desc>();
    clip_checks<ntscsim_key_desc>();
    clip_checks<ntscsim_avg_desc>();
    host_checks<ntscsim_key_desc>();
    host_checks<ntscsim_avg_desc>();
    std::printf("%s: %d failed\n", "layer_host_check", g_failed);
    return g_failed;
}
