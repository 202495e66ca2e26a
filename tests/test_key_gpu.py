"""The device half of the colorkey stage (ntscsim_key_frames_device / _clip_device / _frames_host and the hand-off from
the field simulator) against the checker tests/_key_ref.py, byte for byte: the stage is integer arithmetic on glibc's
rand() stream, so the tolerance is zero.  Every byte of every destination buffer is compared -- row padding and the
guard bytes around the frame included -- and the sources are checked to be untouched."""
import ctypes as C

import numpy as np
import pytest

import _key_ref as R
import _libs as L
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

KEY = 0x8020C040            # non-black, high byte set
SIZES = [(96, 32), (100, 35), (99, 33)]
# rows 16-byte aligned (the vector path) | linesize and base pointer only 4-byte aligned (the dword path)
LAYOUTS = {"aligned": (0, 0), "unaligned": (4, 4)}


def geometry(w, layout):
    extra, off = LAYOUTS[layout]
    return 4 * w + extra + (16 if layout == "aligned" else 0), off          # padded rows in both layouts


def host_frame(w, h, ls, off, frame=None, seed=0):
    """A frame inside a padded byte buffer: rows of `ls` bytes starting `off` bytes in; padding random."""
    buf = np.random.RandomState(seed).randint(0, 256, size=off + h * ls + 16, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w, 4), strides=(ls, 4, 1))
    if frame is not None:
        view[...] = frame
    return buf, view


def dev_view(torch, buf, w, h, ls, off):
    t = torch.from_numpy(buf).cuda()
    return t, torch.as_strided(t, (h, w, 4), (ls, 4, 1), off)


def flags_of(layers, delay=1):
    f = ["-d", str(delay)]
    for lay in layers:
        f += R.layer_flags(lay)
    return f


class Rig:
    """One context, rebound for every layer list; frames in padded buffers of one layout."""

    def __init__(self, w, h, layout):
        import torch
        self.torch = torch
        self.w, self.h = w, h
        self.ls, self.off = geometry(w, layout)
        self.sim = ntscsim.FieldSimulator(device=0)
        self.seed = 1000

    def close(self):
        self.sim.close()

    def keyer(self, layers, delay=1):
        return ntscsim.ColorKeyer(flags_of(layers, delay), width=self.w, height=self.h, sim=self.sim)

    def frame(self, content=None):
        """(host buffer, host view, device buffer, device view); content None: a test frame near KEY"""
        self.seed += 1
        if content is None:
            content = R.make_frame(self.w, self.h, self.seed, key=KEY)
        buf, view = host_frame(self.w, self.h, self.ls, self.off, content, self.seed)
        dbuf, dview = dev_view(self.torch, buf, self.w, self.h, self.ls, self.off)
        return buf, view, dbuf, dview

    def same(self, dbuf, want_buf, what):
        bad = int((dbuf.cpu().numpy() != want_buf).sum())
        assert bad == 0, "%s: %d bytes differ" % (what, bad)

    def check_frames(self, layers, present=None, pos=0, kernels=None, what=""):
        """One descriptor through ntscsim_key_frames_device against the checker; returns the position behind."""
        nl = len(layers)
        present = [1] * nl if present is None else present
        ck = self.keyer(layers)
        srcs = [self.frame() if present[l] else None for l in range(nl)]
        dst = self.frame(np.random.RandomState(self.seed + 7).randint(0, 256, size=(self.h, self.w, 4), dtype=np.uint8))
        ck.key_frames([(dst[3], [s[3] if s else None for s in srcs], pos)])
        ck.sync()
        if kernels is not None:
            assert ck.last_kernels() == kernels, what
        want = dst[0].copy()
        wview = np.lib.stride_tricks.as_strided(want[self.off:], shape=(self.h, self.w, 4), strides=(self.ls, 4, 1))
        frame = np.ascontiguousarray(dst[1])
        end = R.key_frame(frame, [s[1] if s else None for s in srcs], layers, pos)
        wview[...] = frame
        self.same(dst[2], want, what)
        for s in srcs:
            if s:
                self.same(s[2], s[0], what + " (source)")
        assert ck.rand_advance(pos, present) == end
        return end


def names(noise, general=False, clip=False, nl=2):
    """clip=True: the fast clip form carries its layer count, k_key_clip_fast<NOISE,layers>"""
    k = "k_key_%s%s<%s%s>" % ("clip_" if clip else "", "general" if general else "fast", "true" if noise else "false",
                              ",%d" % nl if clip and not general else "")
    return (["k_key_draw"] if noise else []) + [k]


@pytest.fixture(params=[(w, h, lay) for (w, h) in SIZES for lay in sorted(LAYOUTS)], ids=lambda p: "%dx%d-%s" % p)
def rig(request):
    r = Rig(*request.param)
    yield r
    r.close()


def test_xdivr_without_and_with_noise(rig):
    """xdivr 0, 1, 2, 3, 7, 64, width + 5.  With noise the checker itself must show a hit in the middle of a hold group
    (which keys the rest of that group) followed by a later group of the same row without any hit."""
    w, h = rig.w, rig.h
    pos = 5
    for xd in (0, 1, 2, 3, 7, 64, w + 5):
        rig.check_frames([R.layer(color=KEY, threshhold=96, xdivr=xd)], kernels=names(False), what="xd %d" % xd)
        lay = R.layer(color=KEY, threshhold=96, xdivr=xd, noisekey=700 if xd < 64 else 150)
        if 1 < xd < w:
            hit = R.noise_hits(lay, h, w, pos)
            seen = False
            for y in range(h):
                groups = [hit[y, g:g + xd] for g in range(0, w, xd)]
                for gi, g in enumerate(groups[:-1]):
                    if len(g) > 1 and g[1:].any() and not g[0] and any(not later.any() for later in groups[gi + 1:]):
                        seen = True
            assert seen, "no mid-group hit at xd %d" % xd
        pos = rig.check_frames([lay], pos=pos, kernels=names(True), what="xd %d noise" % xd)


def test_noisekey_values(rig):
    """noisekey 1, 2000, 20001, 30000: the last two hit at every pixel; at 2000 every row of the checker's hit map
    has both outcomes."""
    w, h = rig.w, rig.h
    pos = 3 * w * h + 17
    for nk in (1, 2000, 20001, 30000):
        lay = R.layer(color=KEY, threshhold=96, noisekey=nk)
        hit = R.noise_hits(lay, h, w, pos)
        if nk == 2000:
            assert all(hit[y].any() and not hit[y].all() for y in range(h))
        if nk > 20000:
            assert hit.all()
        pos = rig.check_frames([lay], pos=pos, kernels=names(True), what="noisekey %d" % nk)


def test_fade_invert_threshhold_color(rig):
    for fade in (0, 1, 128, 256, 300):                                           # 300: the factor 256 - fade wraps
        for inv in (0, 1):
            rig.check_frames([R.layer(color=KEY, threshhold=96, fade=fade, invert=inv)], kernels=names(False),
                             what="fade %d inv %d" % (fade, inv))
    for thr in (0, 1, 96, 765, 766, -1):
        for inv in (0, 1):
            rig.check_frames([R.layer(color=KEY, threshhold=thr, invert=inv, fade=3)], kernels=names(False),
                             what="threshhold %d inv %d" % (thr, inv))
    rig.check_frames([R.layer(color=0xFF102030, threshhold=200)], kernels=names(False), what="color")


def test_layer_counts_absent_layers_and_positions(rig):
    """1, 2, 5 and 9 layers (fast and general form), a NULL layer in the middle, a noisy layer behind a quiet one and
    behind an absent noisy one: the positions skip what was not drawn."""
    def lay(k, nk=0):
        return R.layer(color=KEY if k % 2 == 0 else 0x102030, threshhold=60 + 25 * k, xdivr=1 + k % 4, fade=(k % 3) * 5,
                       invert=1 if k % 5 == 3 else 0, noisekey=nk)
    for n in (1, 2, 5, 9):
        quiet = [lay(k) for k in range(n)]
        rig.check_frames(quiet, kernels=names(False, n > 4), what="%d layers" % n)
        noisy = [lay(k, nk=(400 if k % 2 == 1 or n == 1 else 0)) for k in range(n)]
        rig.check_frames(noisy, pos=99, kernels=names(True, n > 4), what="%d layers noise" % n)
        if n >= 5:
            present = [1] * n
            present[1] = present[n // 2] = 0                                     # a noisy layer (1) and a middle one absent
            rig.check_frames(noisy, present=present, pos=99, kernels=names(True, True), what="%d layers, absent" % n)
    rig.check_frames([lay(0, 300), lay(1), lay(2, 300)], present=[1, 0, 1], pos=7, kernels=names(True), what="NULL in the middle")
    rig.check_frames([lay(0, 300), lay(1)], present=[0, 1], pos=7, kernels=names(False), what="only noisy layer absent")
    rig.check_frames([lay(0), lay(1)], present=[0, 0], kernels=names(False), what="nothing present")


def _clip_setup(rig, layers, delay, T, absent=()):
    nl = len(layers)
    ring = [rig.frame(np.zeros((rig.h, rig.w, 4), np.uint8)) for _ in range(delay)]          # :1013-1016
    src = [[None if (t, l) in absent else rig.frame() for t in range(T)] for l in range(nl)]
    out = [rig.frame(np.full((rig.h, rig.w, 4), 0x5A, np.uint8)) for _ in range(T)]
    return ring, src, out


def _want_buf(rig, f, content):
    want = f[0].copy()
    np.lib.stride_tricks.as_strided(want[rig.off:], shape=(rig.h, rig.w, 4), strides=(rig.ls, 4, 1))[...] = content
    return want


CLIP_LAYERS = {
    "fast1": [R.layer(color=KEY, threshhold=96, fade=8, xdivr=2)],
    "fast3_noise": [R.layer(color=KEY, threshhold=96, xdivr=7), R.layer(color=0x102030, threshhold=200, noisekey=900),
                    R.layer(color=KEY, threshhold=150, invert=1, fade=2)],
    "fast4_noise": [R.layer(color=KEY, threshhold=60 + 40 * k, fade=k, xdivr=k, noisekey=(250 if k == 2 else 0)) for k in range(4)],
    "fast": [R.layer(color=KEY, threshhold=96, fade=8), R.layer(color=0x102030, threshhold=200, invert=1, xdivr=3)],
    "fast_noise": [R.layer(color=KEY, threshhold=96, fade=8, noisekey=500, xdivr=3), R.layer(color=0x102030, threshhold=200, invert=1)],
    "general": [R.layer(color=KEY, threshhold=70 + 30 * k, fade=k, xdivr=1 + k) for k in range(5)],
    "general_noise": [R.layer(color=KEY, threshhold=70 + 30 * k, fade=k, xdivr=1 + k, noisekey=(300 if k in (1, 4) else 0)) for k in range(5)],
}


@pytest.mark.parametrize("delay", [1, 2, 3, 5, 9])
def test_clip_equals_checker_frames_form_and_split_calls(rig, delay):
    for form in sorted(CLIP_LAYERS):
        _clip_case(rig, delay, form)


def _clip_case(rig, delay, form):
    """T = 7 output frames over rings of 1, 2, 3, 5 and 9 (> T) frames: one clip call, the same clip as two calls
    (ring, ring index and draw position carried over) and the frames form called frame by frame all give the
    checker's outputs and leave the checker's ring."""
    T = 7
    layers = CLIP_LAYERS[form]
    nl = len(layers)
    noise = "noise" in form
    absent = {(2, 0), (4, nl - 1)} if delay in (2, 5) else set()
    pos0 = 41
    ck = rig.keyer(layers, delay)
    ring, src, out = _clip_setup(rig, layers, delay, T, absent)
    # the checker
    cring = [np.zeros((rig.h, rig.w, 4), np.uint8) for _ in range(delay)]
    frames = [[src[l][t][1] if src[l][t] else None for l in range(nl)] for t in range(T)]
    want, want_ri, want_pos = R.key_clip(cring, frames, layers, 0, pos0)

    def run(pieces):
        for f in ring:
            f[2].copy_(rig.torch.from_numpy(f[0]))
        for f in out:
            f[2].copy_(rig.torch.from_numpy(f[0]))
        ri, pos = 0, pos0
        for a, b in pieces:
            ri, pos = ck.key_clip([f[3] for f in ring], [[(s[3] if s else None) for s in lay[a:b]] for lay in src],
                                  [f[3] for f in out[a:b]], ri, pos)
            assert ck.last_kernels() == (names(noise, nl > 4, clip=True, nl=nl) if b > a else [])
        ck.sync()
        assert (ri, pos) == (want_ri, want_pos)
        for t in range(T):
            rig.same(out[t][2], _want_buf(rig, out[t], want[t]), "out[%d] %r" % (t, pieces))
        for i in range(delay):
            rig.same(ring[i][2], _want_buf(rig, ring[i], cring[i]), "ring[%d] %r" % (i, pieces))

    run([(0, T)])
    run([(0, 3), (3, T)])
    run([(0, 0), (0, 1), (1, T)])
    if noise:
        # a bound on the hit bits that lets one frame into a launch: one call becomes T launches, same bytes
        ck.debug_set_bits_limit(1)
        run([(0, T)])
        ck.debug_set_bits_limit(0)
    # the frames form, one call per frame, on the same ring
    for f in ring:
        f[2].copy_(rig.torch.from_numpy(f[0]))
    pos = pos0
    for t in range(T):
        present = [src[l][t] is not None for l in range(nl)]
        ck.key_frames([(ring[t % delay][3], [(src[l][t][3] if src[l][t] else None) for l in range(nl)], pos)])
        pos = ck.rand_advance(pos, present)
        ck.sync()
        rig.same(ring[t % delay][2], _want_buf(rig, ring[t % delay], want[t]), "frames form, frame %d" % t)
    assert pos == want_pos
    for l in range(nl):
        for s in src[l]:
            if s:
                rig.same(s[2], s[0], "source")


def test_descriptors_of_one_call_take_effect_in_order(rig):
    """Three descriptors, the first and the last on the same destination, the second reading what the first wrote."""
    layers = [R.layer(color=KEY, threshhold=96, fade=16, noisekey=300), R.layer(color=0x102030, threshhold=150, xdivr=2)]
    ck = rig.keyer(layers)
    a, b = rig.frame(), rig.frame()
    s = [rig.frame() for _ in range(5)]
    p0 = 10
    p1 = ck.rand_advance(p0)
    p2 = ck.rand_advance(p1)
    ck.key_frames([(a[3], [s[0][3], s[1][3]], p0), (b[3], [a[3], s[2][3]], p1), (a[3], [s[3][3], s[4][3]], p2)])
    ck.sync()
    assert ck.last_kernels() == names(True) * 3
    fa, fb = np.ascontiguousarray(a[1]), np.ascontiguousarray(b[1])
    R.key_frame(fa, [s[0][1], s[1][1]], layers, p0)
    R.key_frame(fb, [fa, s[2][1]], layers, p1)
    R.key_frame(fa, [s[3][1], s[4][1]], layers, p2)
    rig.same(a[2], _want_buf(rig, a, fa), "a")
    rig.same(b[2], _want_buf(rig, b, fb), "b")
    # the same call cut into one launch per descriptor by the bound on the hit bits
    for f in (a, b):
        f[2].copy_(rig.torch.from_numpy(f[0]))
    ck.debug_set_bits_limit(1)
    ck.key_frames([(a[3], [s[0][3], s[1][3]], p0), (b[3], [a[3], s[2][3]], p1), (a[3], [s[3][3], s[4][3]], p2)])
    ck.sync()
    ck.debug_set_bits_limit(0)
    rig.same(a[2], _want_buf(rig, a, fa), "a, one frame per launch")
    rig.same(b[2], _want_buf(rig, b, fb), "b, one frame per launch")
    # independent descriptors share one launch
    c = rig.frame()
    ck.key_frames([(a[3], [s[0][3], s[1][3]], 0), (c[3], [s[2][3], s[3][3]], 0)])
    ck.sync()
    assert ck.last_kernels() == names(True)


def test_host_frames_equal_device_call(rig):
    layers = [R.layer(color=KEY, threshhold=96, fade=8, noisekey=400, xdivr=3), R.layer(color=0x102030, threshhold=200, invert=1)]
    ck = rig.keyer(layers)
    w, h = rig.w, rig.h
    dst = [rig.frame(), rig.frame()]
    src = [rig.frame() for _ in range(3)]
    jobs = [(0, [0, 1], 0), (1, [2, None], ck.rand_advance(0)), (0, [1, 2], 77)]
    ck.key_frames([(dst[d][3], [(src[k][3] if k is not None else None) for k in ss], pos) for d, ss, pos in jobs])
    ck.sync()
    hbuf = [f[0].copy() for f in dst]
    hview = [np.lib.stride_tricks.as_strided(bf[rig.off:], shape=(h, w, 4), strides=(rig.ls, 4, 1)) for bf in hbuf]
    ck.key_frames_host([(hview[d], [(src[k][1] if k is not None else None) for k in ss], pos) for d, ss, pos in jobs])
    for d in range(2):
        rig.same(dst[d][2], hbuf[d], "host call, destination %d" % d)
    want = [np.ascontiguousarray(f[1]) for f in dst]
    for d, ss, pos in jobs:
        R.key_frame(want[d], [(src[k][1] if k is not None else None) for k in ss], layers, pos)
    for d in range(2):
        assert int((hview[d] != want[d]).sum()) == 0


def test_full_size_frame():
    """720 x 486, two layers, noise behind a quiet layer, a held distance, fade: frames form and a short clip."""
    r = Rig(720, 486, "aligned")
    try:
        layers = [R.layer(color=KEY, threshhold=96, fade=8), R.layer(color=KEY, threshhold=120, noisekey=2000, xdivr=3)]
        pos = r.check_frames(layers, pos=0, kernels=names(True), what="720x486")
        ck = r.keyer(layers, 2)
        ring, src, out = _clip_setup(r, layers, 2, 3)
        ri, end = ck.key_clip([f[3] for f in ring], [[s[3] for s in lay] for lay in src], [f[3] for f in out], 0, pos)
        ck.sync()
        assert ck.last_kernels() == names(True, clip=True, nl=2)
        cring = [np.zeros((486, 720, 4), np.uint8) for _ in range(2)]
        want, wri, wpos = R.key_clip(cring, [[src[l][t][1] for l in range(2)] for t in range(3)], layers, 0, pos)
        assert (ri, end) == (wri, wpos)
        for t in range(3):
            r.same(out[t][2], _want_buf(r, out[t], want[t]), "out[%d]" % t)
        for i in range(2):
            r.same(ring[i][2], _want_buf(r, ring[i], cring[i]), "ring[%d]" % i)
    finally:
        r.close()


def test_error_codes():
    import torch
    sim = ntscsim.FieldSimulator(device=0)
    try:
        lib = sim._lib
        a = torch.zeros((32, 96, 4), dtype=torch.uint8, device="cuda")
        b = torch.zeros((32, 96, 4), dtype=torch.uint8, device="cuda")
        small = torch.zeros((32, 64, 4), dtype=torch.uint8, device="cuda")
        # unbound ctx
        d = _capi.KeyDesc()
        assert lib.ntscsim_key_frames_device(sim._h, C.byref(d), 1, None) == _capi.E_ARG
        assert lib.ntscsim_key_frames_host(sim._h, C.byref(d), 1) == _capi.E_ARG
        # bad delay
        for delay in (0, 257):
            p = _capi.make_key_params(["-i", "x"], width=96, height=32)
            p.delay = delay
            with pytest.raises(ntscsim.NtscsimError) as e:
                ntscsim.ColorKeyer(params=p, sim=sim)
            assert e.value.code == _capi.E_PARAM
        ck = ntscsim.ColorKeyer(["-i", "x", "-threshhold", "96", "-i", "y"], width=96, height=32, sim=sim)
        with pytest.raises(ntscsim.NtscsimError) as e:
            ck.key_frames([(small, [small, small], 0)])                           # not the bound size
        assert e.value.code == _capi.E_SIZE
        with pytest.raises(ntscsim.NtscsimError) as e:
            ck.key_frames([(a, [b], 0)])                                          # not the bound layer count
        assert e.value.code == _capi.E_SIZE
        with pytest.raises(ntscsim.NtscsimError) as e:
            ck.key_frames([(a, [b, a], 0)])                                       # a source overlaps the destination
        assert e.value.code == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:
            ck.key_clip([a], [[b], [a]], [torch.zeros_like(a)])                   # a source overlaps the ring
        assert e.value.code == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:
            ck.key_clip([a], [[b], [b]], [a])                                     # an output overlaps the ring
        assert e.value.code == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:
            ck.key_clip([a], [[b], [b]], [torch.zeros_like(a)], ring_index=1)     # ring index outside the ring
        assert e.value.code == _capi.E_ARG
        ck.key_frames([])
        ck.key_frames([(a, [b, None], 0)])
        ck.sync()
    finally:
        sim.close()


def test_simulator_output_is_keyed_without_leaving_the_device():
    """A few -vhs fields from ntscsim_fields_device stay in device memory and go into the key stage as the top layer
    over a background: the result is the checker applied to the simulator's downloaded output."""
    import torch
    w, h, n = 96, 32, 4
    p = L.make_params(["-vhs"])
    sim = ntscsim.FieldSimulator(params=p, device=0)
    try:
        layers = [R.layer(threshhold=0), R.layer(color=0x101010, threshhold=120, noisekey=300, xdivr=2)]
        ck = ntscsim.ColorKeyer(flags_of(layers, 2), width=w, height=h, sim=sim)
        frames = np.stack([L.noise_frame(w, h, 0x51 + i) for i in range(n // 2)])
        frames[:, :, : w // 2] //= 8                                              # a dark half: keyed out
        jobs = [(k // 2, k, (k & 1) ^ 1, k) for k in range(n)]
        src = torch.from_numpy(frames).cuda()
        fields = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
        sim.fields(src, fields, jobs)
        bg = [R.make_frame(w, h, 900 + t) for t in range(n)]
        dbg = [torch.from_numpy(f).cuda() for f in bg]
        ring = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
        out = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
        ri, pos = ck.key_clip(ring, [dbg, [fields[t] for t in range(n)]], out)
        ck.sync()
        sim_out = fields.cpu().numpy()
        cring = [np.zeros((h, w, 4), np.uint8) for _ in range(2)]
        want, wri, wpos = R.key_clip(cring, [[bg[t], sim_out[t]] for t in range(n)], layers)
        assert (ri, pos) == (wri, wpos)
        got = np.stack([o.cpu().numpy() for o in out])
        assert int((got != want).sum()) == 0
        assert 0.05 < float((got == np.stack(bg)).all(axis=3).mean()) < 0.95      # both layers show
    finally:
        sim.close()
