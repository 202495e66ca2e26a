"""Launches of the device stages that the stages' own test files never make: thousands of descriptors in one call (the
grid-stride loops of k_key_*, k_avg_* and k_scan_resolve then make several passes), records of one launch that differ
in memory layout, size, tap count and weight range, one misaligned frame in an otherwise aligned clip, and a blend
call of more than 65535 descriptors.  Everything is integer arithmetic against the checkers (_key_ref, _avg_ref,
_blend_ref, _scan_ref), so the tolerance is zero; whole destination buffers are compared -- row padding and guard bytes
included -- the sources are checked to be untouched and the kernel names are asserted.

Many destinations cycle through a few distinct inputs so that the expected bytes need few checker runs: K = 7 patterns
of sources and initial destination content (7 is coprime to the pass and workgroup counts in play), every destination
in memory of its own, two memory layouts alternating from one descriptor to the next.  Every test asserts the
property it is after (per < slices, the number of distinct position gaps, two launches ...) from the host's own rule,
so a later change of a constant makes the test say so instead of silently stop covering its case."""
import ctypes as C
import functools

import numpy as np
import pytest

import _avg_ref as RA
import _blend_ref as RB
import _key_ref as RK
import _libs as L  # noqa: F401
import _scan_ref as RS
import ntscsim

pytestmark = pytest.mark.gpu

K = 7
W, H = 99, 33                            # ceil(W / 4) * H = 825 items: 4 slices of 256
# layout of a 99 x 33 frame inside its slot: (offset of the first pixel, linesize).  0: every pointer and linesize a
# multiple of 16 (the 16-byte path, the last quad of a row partial); 1: both only multiples of 4 (the dword path)
GEO = {0: (16, 416), 1: (20, 420)}
SLOT = (20 + H * 420 + 16 + 15) // 16 * 16
KEY = 0x8020C040


def strided(buf, off, ls, w, h):
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w, 4), strides=(ls, 4, 1))


def ceil_div(a, b):
    return (a + b - 1) // b


def frames_grid(w, h, n, target=8192, threads=256):
    """(slices, per) by the rule of key_launch() / avg_launch() / blend_launch() / scan_launch()"""
    slices = ceil_div(ceil_div(w, 4) * h, threads)
    return slices, max(1, min(slices, ceil_div(target, n)))


def random_bytes(seed, n):
    return np.random.RandomState(seed).randint(0, 256, size=n, dtype=np.uint8)


# ---- many descriptors per call: key and avg frames forms at 99 x 33 -------------------------------------------

class Batch:
    """V variants of one descriptor: variant j reads the sources of pattern j % K, carries tag[j] and starts from
    destination content of its own; the checker's result is computed once per variant.  Descriptor i of a call is
    variant i % V in layout i % 2, in its own slot of one device buffer."""

    def __init__(self, torch, nl, absent, tags, make_src, seed):
        self.torch = torch
        self.V = len(tags)
        assert self.V % 2 == 1 and self.V % K == 0                   # every (variant, layout) pair occurs; patterns cycle
        self.tags = tags
        self.src_host, self.src_dev = [], []
        for p in range(K):
            hs, ds = [], []
            for l in range(nl):
                if l in absent.get(p, ()):
                    hs.append(None)
                    ds.append(None)
                    continue
                lay = (p + l) % 2 if l == nl - 1 else 0              # odd patterns: the last layer's source on the dword layout
                off, ls = GEO[lay]
                buf = random_bytes(seed + 100 * p + l, SLOT)
                strided(buf, off, ls, W, H)[...] = make_src(seed + 100 * p + l)
                t = torch.from_numpy(buf).cuda()
                hs.append((buf, strided(buf, off, ls, W, H)))
                ds.append((t, torch.as_strided(t, (H, W, 4), (ls, 4, 1), off)))
            self.src_host.append(hs)
            self.src_dev.append(ds)
        self.init = np.empty((2 * self.V, SLOT), np.uint8)
        self.content = []
        for j in range(self.V):
            c = random_bytes(seed + 7000 + j, H * W * 4).reshape(H, W, 4)
            self.content.append(c)
            for lay in (0, 1):
                row = self.init[2 * j + lay]
                row[...] = random_bytes(seed + 9000 + 2 * j + lay, SLOT)
                strided(row, GEO[lay][0], GEO[lay][1], W, H)[...] = c
        self.want = None

    def sources(self, j):
        return [(s[1] if s else None) for s in self.src_host[j % K]]

    def present(self, j):
        return [s is not None for s in self.src_host[j % K]]

    def expect(self, frames):
        """frames[j]: the checker's destination of variant j"""
        self.want = self.init.copy()
        for j in range(self.V):
            for lay in (0, 1):
                strided(self.want[2 * j + lay], GEO[lay][0], GEO[lay][1], W, H)[...] = frames[j]

    def call(self, stage, frames_call, n, kernels, what):
        torch = self.torch
        i = np.arange(n)
        combo = (i % self.V) * 2 + (i % 2)
        if n >= 2 * self.V:
            assert len(set(combo.tolist())) == 2 * self.V
        big = torch.from_numpy(self.init[combo]).cuda()
        flat = big.view(-1)
        jobs = []
        for d in range(n):
            off, ls = GEO[d % 2]
            dst = torch.as_strided(flat, (H, W, 4), (ls, 4, 1), d * SLOT + off)
            jobs.append((dst, [(s[1] if s else None) for s in self.src_dev[(d % self.V) % K]], self.tags[d % self.V]))
        vec = [d % 2 == 0 and all(s is None or s[1].data_ptr() % 16 == 0 and s[1].stride(0) % 16 == 0
                                  for s in self.src_dev[(d % self.V) % K]) for d in range(min(n, 2 * K))]
        if n >= 2 * K:
            assert any(vec) and not all(vec)                             # records of both paths in one launch
        frames_call(jobs)
        stage.sync()
        assert stage.last_kernels() == kernels, what
        bad = (big.cpu().numpy() != self.want[combo]).any(axis=1)
        assert not bad.any(), "%s: %d of %d destinations differ, the first is %d" % (what, int(bad.sum()), n, int(np.argmax(bad)))

    def sources_untouched(self):
        for hs, ds in zip(self.src_host, self.src_dev):
            for h, d in zip(hs, ds):
                if h is not None:
                    assert int((d[0].cpu().numpy() != h[0]).sum()) == 0, "a source changed"

    def calls(self, stage, frames_call, n, kernels, what):
        """n == 8200: four 3-descriptor calls in front and behind.  The stage keeps four record slots and takes them in
        turn, so the long call gets the slot of the first short one and RecordSlots::acquire() has to grow it (free and
        allocate again); the short calls behind it run once through every slot, the grown one included."""
        short = 4 if n == 8200 else 0
        for k in range(short):
            self.call(stage, frames_call, 3, kernels, "%s, short call %d in front" % (what, k))
        self.call(stage, frames_call, n, kernels, "%s, %d descriptors" % (what, n))
        for k in range(short):
            self.call(stage, frames_call, 3, kernels, "%s, short call %d behind" % (what, k))
        self.sources_untouched()


def assert_passes(n):
    slices, per = frames_grid(W, H, n)
    assert slices == 4
    # 4100: workgroup 0 makes two full passes, workgroup 1 one full and one partial | 8200: four passes, the last partial
    assert per == {4100: 2, 8200: 1}[n] and per < slices and ceil_div(W, 4) * H % 256 != 0


KEY_LAYERS = {
    ("fast", False): [RK.layer(color=KEY, threshhold=96, fade=8, xdivr=3), RK.layer(color=0x102030, threshhold=200, invert=1)],
    ("fast", True): [RK.layer(color=KEY, threshhold=96, fade=8, xdivr=3, noisekey=500), RK.layer(color=0x102030, threshhold=200, invert=1)],
    ("general", False): [RK.layer(color=KEY, threshhold=70 + 30 * k, fade=k, xdivr=1 + k) for k in range(5)],
    ("general", True): [RK.layer(color=KEY, threshhold=70 + 30 * k, fade=k, xdivr=1 + k, noisekey=(300 if k in (1, 4) else 0))
                        for k in range(5)],
}
# pattern -> absent layers; layer 0 (fast) and layer 1 (general) draw noise and are always there: every descriptor has a job
ABSENT = {"fast": {3: (1,)}, "general": {3: (2,), 5: (0, 4)}}


def key_positions():
    """77 rand() positions for the noisy calls: pattern j % 7 at position j of the cycle.  Consecutive ones are
    2 * 3 * W * H + 17 * (j + 1) apart -- a different distance at every step, which stays a forward distance behind a
    descriptor with two noisy layers -- except that entry 40 jumps back to 3, and the cycle wraps back to its start."""
    pos = [5]
    for j in range(1, 11 * K):
        pos.append(3 if j == 40 else pos[-1] + 6 * W * H + 17 * j)
    assert max(pos) + 6 * W * H < 10 ** 7
    return pos


def flags_key(layers):
    f = ["-d", "1"]
    for lay in layers:
        f += RK.layer_flags(lay)
    return f


@pytest.mark.parametrize("n", [4100, 8200])
@pytest.mark.parametrize("noisy", [False, True], ids=["quiet", "noise"])
@pytest.mark.parametrize("form", ["fast", "general"])
def test_key_many_descriptors(form, noisy, n):
    """k_key_fast / k_key_general over 4100 and 8200 descriptors of 99 x 33: per = 2 and 1 workgroups for 4 slices, so
    the grid-stride loop makes two and four passes, the last partial.  Layouts alternate inside the call (16-byte and
    dword records in one launch), a few layers are absent.  The noisy 8200-descriptor call walks more than 64 distinct
    forward distances between consecutive draw jobs -- key_state_at() clears its map of jump polynomials at 64 -- and
    goes backwards at least twice; it is framed by short calls that make a record slot grow."""
    import torch
    assert_passes(n)
    layers = KEY_LAYERS[(form, noisy)]
    nl = len(layers)
    tags = key_positions() if noisy else [11 * j for j in range(K)]
    b = Batch(torch, nl, ABSENT[form], tags, lambda s: RK.make_frame(W, H, s, key=KEY), 31000 + 1000 * nl)
    ck = ntscsim.ColorKeyer(flags_key(layers), width=W, height=H)
    try:
        frames = []
        for j in range(b.V):
            f = b.content[j].copy()
            end = RK.key_frame(f, b.sources(j), layers, tags[j])
            assert ck.rand_advance(tags[j], b.present(j)) == end
            frames.append(f)
        b.expect(frames)
        if noisy:
            jobs = []
            for d in range(n):
                pos = tags[d % b.V]
                for l, lay in enumerate(layers):
                    if b.present(d % b.V)[l] and lay["noisekey"] > 0:
                        jobs.append(pos)
                        pos += 3 * W * H
            assert len(jobs) >= n                                         # a k_key_draw job for every descriptor
            gaps = np.diff(np.array(jobs, dtype=np.int64))
            if n == 8200:
                assert len(set(gaps[gaps > 0].tolist())) > 64 and int((gaps < 0).sum()) >= 2
            # the checker's draws at those positions all differ: a window carried to the wrong place shows in the hits
            firsts = set(tuple(RK.RAND.draws(p, 4).tolist()) for p in tags)
            assert len(firsts) == len(tags)
            # and the library's own window at every position (lane 0 of a job there, computed afresh on the host) is the
            # checker's: what is left to the byte compare is key_state_at()'s walk from one position to the next, which
            # no entry point shows
            out31 = (C.c_uint32 * 31)()
            for p in tags:
                assert ck._lib.ntscsim_key_debug_lane_state(W, H, p, 0, out31) == 0
                assert list(out31) == RK.RAND.window(p), p
        name = "k_key_%s<%s>" % (form, "true" if noisy else "false")
        b.calls(ck, ck.key_frames, n, (["k_key_draw"] if noisy else []) + [name], "key %s %s" % (form, "noise" if noisy else "quiet"))
    finally:
        ck.close()


AVG_LEVELS = {"fast": [200, 300], "general": [128, 64, 65536, 0, 200]}
AVG_FIELDS = [5, 6, 7, 8, (1 << 32) + 9, 10, 23]          # delay 3: field / delay takes every dither phase


@pytest.mark.parametrize("n", [4100, 8200])
@pytest.mark.parametrize("form", ["fast", "general"])
def test_avg_many_descriptors(form, n):
    """k_avg_fast / k_avg_general over 4100 and 8200 descriptors of 99 x 33, as test_key_many_descriptors."""
    import torch
    assert_passes(n)
    levels = AVG_LEVELS[form]
    nl = len(levels)
    delay = 3
    assert set(int(RA.dither(1, 1, f, delay)[0, 0]) for f in AVG_FIELDS) == {0, 85, 170, 255}
    b = Batch(torch, nl, ABSENT[form], AVG_FIELDS, lambda s: RA.make_frame(W, H, s), 52000 + 1000 * nl)
    flags = ["-d", str(delay)]
    for lv in levels:
        flags += RA.layer_flags(lv)
    av = ntscsim.FrameAverager(flags, width=W, height=H)
    try:
        frames = []
        for j in range(b.V):
            f = b.content[j].copy()
            RA.avg_frame(f, b.sources(j), levels, AVG_FIELDS[j], delay)
            frames.append(f)
        b.expect(frames)
        b.calls(av, av.average_frames, n, ["k_avg_" + form], "avg " + form)
    finally:
        av.close()


# ---- scan: eight fields of just over 262144 pixels in one call --------------------------------------------------

SCAN_SRC = (24, 40)                      # mono; the bind accepts any ratio, so this is the stage's cheapest source
SCAN_FIELDNOS = [0, 45, 181, 271, 361, 500, 541, 700]
SCAN_LAYOUTS = {"aligned": (16, 0), "unaligned": (4, 4)}
SCAN_KERNELS = ["k_scan_splat+spill", "k_scan_resolve"]


@functools.lru_cache(maxsize=None)
def scan_source(seed):
    f = RS.make_source(SCAN_SRC[0], SCAN_SRC[1], 8100 + seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def scan_reference(dw, dh, k):
    """the checker's BGRA field of descriptor k: computed once, shared by the layouts, never written"""
    out = RS.scan_field(scan_source(k), dw, dh, 0, SCAN_FIELDNOS[k])[1]
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("layout", sorted(SCAN_LAYOUTS))
@pytest.mark.parametrize("dw, dh", [(544, 484), (546, 482)])
def test_scan_eight_large_fields_in_one_call(dw, dh, layout):
    """One scan_frames call of 8 independent descriptors (one launch pair: the ctx has 8 accumulator planes) whose
    outputs have just over 262144 pixels: k_scan_resolve gets ceil(2048 / 8) = 256 workgroups per descriptor for 258
    slices, so two of them make a second pass.  All four effects and both parities; 546 wide: the accumulator rows are
    not 16-byte aligned (accvec false).  At this ratio (dot radius 12.7) the splat windows spill."""
    import torch
    m = len(SCAN_FIELDNOS)
    assert m == 8
    slices = ceil_div(ceil_div(dw, 4) * dh, 256)
    per = max(1, min(slices, ceil_div(2048, m)))
    assert per < slices < 2 * per and dw * dh > 262144
    assert (dw % 4 == 0) == (dw == 544)                                  # accvec in k_scan_resolve
    assert set(RS.effect_of(f)[0] for f in SCAN_FIELDNOS) == {0, 1, 2, 3} and set(RS.field_of(f) for f in SCAN_FIELDNOS) == {0, 1}
    pad, off = SCAN_LAYOUTS[layout]
    sw, sh = SCAN_SRC
    sc = ntscsim.Scanimator([], width=dw, height=dh)
    try:
        srcs, dsts, jobs = [], [], []
        for k, fieldno in enumerate(SCAN_FIELDNOS):
            sls, dls = 4 * sw + pad, 4 * dw + pad
            sbuf = random_bytes(600 + k, off + sh * sls + 16)
            strided(sbuf, off, sls, sw, sh)[...] = scan_source(k)
            dbuf = random_bytes(700 + k, off + dh * dls + 16)
            st, dt = torch.from_numpy(sbuf).cuda(), torch.from_numpy(dbuf).cuda()
            srcs.append((sbuf, st))
            dsts.append((dbuf, dt))
            jobs.append((torch.as_strided(dt, (dh, dw, 4), (dls, 4, 1), off), torch.as_strided(st, (sh, sw, 4), (sls, 4, 1), off), fieldno))
        sc.scan_frames(jobs)
        sc.sync()
        assert sc.last_kernels() == SCAN_KERNELS
        for k, fieldno in enumerate(SCAN_FIELDNOS):
            field = RS.field_of(fieldno)
            want = dsts[k][0].copy()
            strided(want, off, 4 * dw + pad, dw, dh)[field:] = scan_reference(dw, dh, k)[field:]
            bad = int((dsts[k][1].cpu().numpy() != want).sum())
            assert bad == 0, "descriptor %d (field %d): %d bytes differ" % (k, fieldno, bad)
            assert int((srcs[k][1].cpu().numpy() != srcs[k][0]).sum()) == 0, "source %d changed" % k
    finally:
        sc.close()


# ---- blend: unlike records in one launch, and more than 65535 descriptors -------------------------------------------

BLEND_LAYOUTS = {"A": (16, 0), "U": (4, 4)}          # (row padding, offset of the first pixel)
# (width, height, taps, layout of the destination and its sources); "M": an aligned destination, one source not.
# 263 x 24 is the largest (1584 quads against 825, 768 and 16) and comes neither first nor last in any of the calls
BLEND_DESCS = [
    (16, 4, 0, "A"), (96, 32, 1, "U"), (99, 33, 2, "A"), (263, 24, 4, "A"), (96, 32, 40, "A"), (99, 33, 3, "U"),
    (16, 4, 4, "U"), (263, 24, 40, "U"), (99, 33, "wide", "A"), (96, 32, 5, "M"), (16, 4, 40, "A"), (99, 33, 1, "A"),
]


@pytest.mark.parametrize("gamma", [2.2, None], ids=["gamma", "plain"])
def test_blend_unlike_descriptors_in_one_launch(gamma):
    """blend_launch() decides `general` and `wide` once per launch over all descriptors and sizes the grid by the
    largest one.  One call mixes four sizes, 0 .. 5 and 40 taps, both layouts and one descriptor whose weights break the
    u32 bound: a single k_blend_general<g,true>.  The same call without the wide descriptor, without the many-tap
    ones, and without either shows each of the two decisions from both sides."""
    import torch
    nsrc = 8
    g = "true" if gamma else "false"
    sizes = sorted(set((w, h) for w, h, _, _ in BLEND_DESCS))
    assert sizes == [(16, 4), (96, 32), (99, 33), (263, 24)]
    assert set(t for _, _, t, _ in BLEND_DESCS) == {0, 1, 2, 3, 4, 5, 40, "wide"}

    def make(w, h, lay, seed):
        pad, off = BLEND_LAYOUTS[lay]
        ls = 4 * w + 16 + pad if lay == "U" else (4 * w + 15) // 16 * 16 + pad
        buf = random_bytes(seed, off + h * ls + 16)
        t = torch.from_numpy(buf).cuda()
        return buf, strided(buf, off, ls, w, h), t, torch.as_strided(t, (h, w, 4), (ls, 4, 1), off)

    src = {(w, h, lay): [make(w, h, lay, 3000 + 97 * si + 10 * li + k) for k in range(nsrc)]
           for si, (w, h) in enumerate(sizes) for li, lay in enumerate("AU")}

    def taps(n, seed):
        if n == "wide":
            return [(0, 9000000), (4, 9000001)]
        rs = np.random.RandomState(seed)
        cut = np.sort(rs.randint(0, 65537, size=n - 1)) if n > 1 else np.array([], dtype=np.int64)
        wts = np.diff(np.concatenate([[0], cut, [65536]])).tolist() if n else []
        return [((seed + 3 * k) % nsrc, int(x)) for k, x in enumerate(wts)]

    fb = ntscsim.FrameBlender(("-gamma", repr(gamma)) if gamma else ())
    try:
        calls = {
            "k_blend_general<%s,true>" % g: BLEND_DESCS,
            "k_blend_general<%s,false>" % g: [d for d in BLEND_DESCS if d[2] != "wide"],
            "k_blend_fast<%s,true>" % g: [d for d in BLEND_DESCS if d[2] == "wide" or d[2] <= 4],
            "k_blend_fast<%s,false>" % g: [d for d in BLEND_DESCS if d[2] != "wide" and d[2] <= 4],
        }
        for kernel, descs in calls.items():
            items = [ceil_div(w, 4) * h for w, h, _, _ in descs]
            assert max(items) not in (items[0], items[-1]) and len(set(items)) == 4
            assert (max(1 if t == "wide" else t for _, _, t, _ in descs) > 4) == ("general" in kernel)
            assert any(t == "wide" for _, _, t, _ in descs) == kernel.endswith("true>")
            mul = 8192 if gamma else 255
            assert mul * (9000000 + 9000001) >= 1 << 32 and mul * 65536 < 1 << 32
            dst, jobs, want = [], [], []
            for i, (w, h, nt, lay) in enumerate(descs):
                dl = "A" if lay == "M" else lay
                d = make(w, h, dl, 4000 + i)
                tl = taps(nt, 40 + i)
                pick = [src[(w, h, dl)][s] for s, _ in tl]
                if lay == "M":
                    pick[-1] = src[(w, h, "U")][tl[-1][0]]
                jobs.append((d[3], [(p[3], wt) for p, (_, wt) in zip(pick, tl)]))
                wb = d[0].copy()
                pad, off = BLEND_LAYOUTS[dl]
                strided(wb, off, d[3].stride(0), w, h)[...] = RB.blend_frame((h, w), [p[1] for p in pick], [wt for _, wt in tl], gamma)
                dst.append(d)
                want.append(wb)
            vec = [all(t.data_ptr() % 16 == 0 and t.stride(0) % 16 == 0 for t in [dj] + [s for s, _ in tj]) for dj, tj in jobs]
            assert any(vec) and not all(vec)
            fb.blend_frames(jobs)
            fb.sync()
            assert fb.last_kernels() == [kernel]
            for i, d in enumerate(dst):
                bad = int((d[2].cpu().numpy() != want[i]).sum())
                assert bad == 0, "%s descriptor %d %r: %d bytes differ" % (kernel, i, descs[i], bad)
        for frames in src.values():
            for f in frames:
                assert int((f[2].cpu().numpy() != f[0]).sum()) == 0, "a source changed"
    finally:
        fb.close()


def test_blend_more_than_65535_descriptors():
    """65540 descriptors of 1 x 1 (the smallest frame a descriptor may have): ntscsim_blend_frames_device cuts the call
    into launches of 65535 and 5.  Sources are shared, every destination is a 16-byte slot of one tensor (4 guard bytes,
    the pixel, 8 guard bytes), content cycles over 7 patterns.  Only pattern 6 has more than four taps and the second
    launch holds patterns 1 .. 5, so the two launches also decide their form each on their own."""
    import torch
    n, slot = 65540, 16
    nsrc = 8
    hsrc = [random_bytes(5000 + k, 4).reshape(1, 1, 4) for k in range(nsrc)]
    dsrc = [torch.from_numpy(s).cuda() for s in hsrc]
    pats = [[], [(0, 65536)], [(1, 30000), (2, 35536)], [(3, 10000), (4, 20000), (5, 35536)],
            [(6, 16384), (7, 16384), (0, 16384), (2, 16384)], [(5, 65536), (1, 0)],
            [(0, 10000), (1, 10000), (2, 10000), (3, 10000), (4, 25536)]]
    assert len(pats) == K and [len(p) > 4 for p in pats] == [False] * 6 + [True]
    assert [(i % K) for i in range(65535, n)] == [1, 2, 3, 4, 5]
    init = np.stack([random_bytes(5100 + p, slot) for p in range(K)])
    want = init.copy()
    for p in range(K):
        want[p, 4:8] = RB.blend_frame((1, 1), [hsrc[s] for s, _ in pats[p]], [wt for _, wt in pats[p]], None).reshape(4)
        assert (want[p, 4:8] != init[p, 4:8]).any()
    idx = np.arange(n) % K
    big = torch.from_numpy(init[idx]).cuda()
    flat = big.view(-1)
    fb = ntscsim.FrameBlender(())
    try:
        jobs = [(torch.as_strided(flat, (1, 1, 4), (8, 4, 1), i * slot + 4), [(dsrc[s], wt) for s, wt in pats[i % K]]) for i in range(n)]
        fb.blend_frames(jobs)
        fb.sync()
        assert fb.last_kernels() == ["k_blend_general<false,false>", "k_blend_fast<false,false>"]
        got = big.cpu().numpy()
        for i in range(n - 5, n):
            assert got[i].tolist() == want[i % K].tolist(), "destination %d" % i
        bad = (got != want[idx]).any(axis=1)
        assert not bad.any(), "%d destinations differ, the first is %d" % (int(bad.sum()), int(np.argmax(bad)))
        for k in range(nsrc):
            assert (dsrc[k].cpu().numpy() == hsrc[k]).all()
    finally:
        fb.close()


# ---- clips: one misaligned frame in an aligned clip ---------------------------------------------------------------

CLIP_T, CLIP_DELAY, CLIP_LS = 7, 3, 400          # 400 bytes: rows of 96 and of 99 pixels, a multiple of 16


class ClipRig:
    """Frames of a clip in padded buffers, rows of 400 bytes; `odd` names the one frame that lies 4 bytes further in."""

    def __init__(self, torch, w, h, odd):
        self.torch, self.w, self.h, self.odd, self.seed = torch, w, h, odd, 77000

    def frame(self, name, content):
        self.seed += 1
        off = 4 if name == self.odd else 0
        buf = random_bytes(self.seed, 4 + self.h * CLIP_LS + 16)
        view = strided(buf, off, CLIP_LS, self.w, self.h)
        view[...] = content
        t = self.torch.from_numpy(buf).cuda()
        dv = self.torch.as_strided(t, (self.h, self.w, 4), (CLIP_LS, 4, 1), off)
        assert (dv.data_ptr() % 16 == 0) == (name != self.odd) and dv.data_ptr() % 4 == 0
        return buf, view, t, dv, off

    def setup(self, make_src):
        h, w = self.h, self.w
        self.ring = [self.frame(("ring", i), np.zeros((h, w, 4), np.uint8)) for i in range(CLIP_DELAY)]
        self.src = [[self.frame(("src", t, l), make_src(self.seed)) for t in range(CLIP_T)] for l in range(2)]
        self.out = [self.frame(("out", t), np.full((h, w, 4), 0x5A, np.uint8)) for t in range(CLIP_T)]
        assert sum(f[4] == 4 for f in self.ring + self.src[0] + self.src[1] + self.out) == 1      # exactly one misaligned frame

    def check(self, want, cring):
        for name, frames, contents in (("out", self.out, want), ("ring", self.ring, cring)):
            for i, f in enumerate(frames):
                wb = f[0].copy()
                strided(wb, f[4], CLIP_LS, self.w, self.h)[...] = contents[i]
                bad = int((f[2].cpu().numpy() != wb).sum())
                assert bad == 0, "%s[%d]: %d bytes differ" % (name, i, bad)
        for lay in self.src:
            for f in lay:
                assert int((f[2].cpu().numpy() != f[0]).sum()) == 0, "a source changed"


ODD_FRAMES = {"source": ("src", 4, 1), "ring": ("ring", 1), "output": ("out", 4)}


@pytest.mark.parametrize("w, h", [(96, 32), (99, 33)])
@pytest.mark.parametrize("noisy", [False, True], ids=["quiet", "noise"])
@pytest.mark.parametrize("odd", sorted(ODD_FRAMES))
def test_key_clip_with_one_misaligned_frame(odd, noisy, w, h):
    """T = 7, delay 3, 2 layers, every frame 16-byte aligned but one: source frame t = 4 of layer 1, ring frame 1 or
    output frame 4.  key_launch() has to move the whole clip as dwords (allbits); the kernel's name does not change."""
    import torch
    layers = KEY_LAYERS[("fast", noisy)]
    r = ClipRig(torch, w, h, ODD_FRAMES[odd])
    r.setup(lambda s: RK.make_frame(w, h, s, key=KEY))
    ck = ntscsim.ColorKeyer(["-d", str(CLIP_DELAY)] + flags_key(layers)[2:], width=w, height=h)
    try:
        assert ck.delay == CLIP_DELAY
        pos0 = 41
        cring = [np.zeros((h, w, 4), np.uint8) for _ in range(CLIP_DELAY)]
        want, wri, wpos = RK.key_clip(cring, [[r.src[l][t][1] for l in range(2)] for t in range(CLIP_T)], layers, 0, pos0)
        ri, pos = ck.key_clip([f[3] for f in r.ring], [[f[3] for f in lay] for lay in r.src], [f[3] for f in r.out], 0, pos0)
        ck.sync()
        assert ck.last_kernels() == (["k_key_draw"] if noisy else []) + ["k_key_clip_fast<%s,2>" % ("true" if noisy else "false")]
        assert (ri, pos) == (wri, wpos)
        r.check(want, cring)
    finally:
        ck.close()


@pytest.mark.parametrize("w, h", [(96, 32), (99, 33)])
@pytest.mark.parametrize("odd", sorted(ODD_FRAMES))
def test_avg_clip_with_one_misaligned_frame(odd, w, h):
    """As test_key_clip_with_one_misaligned_frame: avg_launch() clears cd.vec for the whole clip."""
    import torch
    levels = AVG_LEVELS["fast"]
    r = ClipRig(torch, w, h, ODD_FRAMES[odd])
    r.setup(lambda s: RA.make_frame(w, h, s))
    flags = ["-d", str(CLIP_DELAY)]
    for lv in levels:
        flags += RA.layer_flags(lv)
    av = ntscsim.FrameAverager(flags, width=w, height=h)
    try:
        field0 = 5
        cring = [np.zeros((h, w, 4), np.uint8) for _ in range(CLIP_DELAY)]
        want, wri, wfield = RA.avg_clip(cring, [[r.src[l][t][1] for l in range(2)] for t in range(CLIP_T)], levels, 0, field0)
        ri, field = av.average_clip([f[3] for f in r.ring], [[f[3] for f in lay] for lay in r.src], [f[3] for f in r.out], 0, field0)
        av.sync()
        assert av.last_kernels() == ["k_avg_clip_fast<2>"]
        assert (ri, field) == (wri, wfield)
        r.check(want, cring)
    finally:
        av.close()
