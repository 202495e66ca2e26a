"""The device half of the posterize and colormap stages (ntscsim_post_* / ntscsim_cmap_*: frames_device, frames_host,
the colour table's get / set / reset, the hand-off from the field simulator) against the checker tests/_pixmap_ref.py,
byte for byte: both stages move and mask whole dwords, so the tolerance is zero.  Every byte of every destination
buffer is compared -- row padding and the guard bytes around the frame included -- and the sources and maps are checked
to be untouched.  The colormap's table is read back through ntscsim_cmap_get_table, so that a wrong table is told from
a wrong gather.

A workgroup owns a band of 8 rows and a lane a quad of 4 pixels: the shapes straddle those numbers (18 rows are two
bands and a quarter; 1, 3, 37 and 260 wide end in a quad that is not whole; 64 and 256 do not), and the three layouts
take the 16-byte stores, the dword stores, and 16-byte stores from sources that are only dword-aligned."""
import ctypes as C

import numpy as np
import pytest

import _libs as L
import _pixmap_ref as R
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (37, 5), (64, 18), (256, 2), (260, 18), (1, 18), (260, 1), (37, 1), (256, 5)]
# (destination, source and map): rows and base 16-byte aligned (the vector path) | linesize and base only 4-byte aligned (dwords)
LAYOUTS = {"aligned": ("v", "v"), "unaligned": ("d", "d"), "mixed": ("v", "d")}
ALL_THRESHHOLDS = sum((["-i", "in%d" % t, "-threshhold", str(t)] for t in range(9)), [])


def geometry(w, kind):
    return ((4 * w + 15) // 16 * 16 + 16, 0) if kind == "v" else (4 * w + 4, 4)


def host_frame(w, h, ls, off, frame=None, seed=0):
    """A frame inside a padded byte buffer: rows of `ls` bytes starting `off` bytes in; padding random."""
    buf = np.random.RandomState(seed).randint(0, 256, size=off + h * ls + 16, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w, 4), strides=(ls, 4, 1))
    if frame is not None:
        view[...] = frame
    return buf, view


@pytest.fixture(scope="module")
def sim():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


class Rig:
    def __init__(self, sim, w, h, layout):
        import torch
        self.torch = torch
        self.sim, self.w, self.h = sim, w, h
        self.dgeo, self.sgeo = geometry(w, LAYOUTS[layout][0]), geometry(w, LAYOUTS[layout][1])
        self.rng = np.random.RandomState(w * 1000 + h)
        self.seed = 7000

    def noise(self):
        return self.rng.randint(0, 256, size=(self.h, self.w, 4)).astype(np.uint8)

    def put(self, geo, content=None):
        """(host buffer, host view, device buffer, device view)"""
        self.seed += 1
        ls, off = geo
        buf, view = host_frame(self.w, self.h, ls, off, content, self.seed)
        t = self.torch.from_numpy(buf).cuda()
        return buf, view, t, self.torch.as_strided(t, (self.h, self.w, 4), (ls, 4, 1), off)

    def want_buf(self, f, geo, content):
        want = f[0].copy()
        np.lib.stride_tricks.as_strided(want[geo[1]:], shape=(self.h, self.w, 4), strides=(geo[0], 4, 1))[...] = content
        return want

    def same(self, f, geo, content, what):
        bad = int((f[2].cpu().numpy() != self.want_buf(f, geo, content)).sum())
        assert bad == 0, "%s: %d bytes differ" % (what, bad)

    def untouched(self, f, what):
        assert int((f[2].cpu().numpy() != f[0]).sum()) == 0, "%s written" % what

    def host_copy(self, f, geo):
        buf = f[0].copy()
        return buf, np.lib.stride_tricks.as_strided(buf[geo[1]:], shape=(self.h, self.w, 4), strides=(geo[0], 4, 1))


@pytest.fixture(params=[(w, h, lay) for (w, h) in SIZES for lay in sorted(LAYOUTS)], ids=lambda p: "%dx%d-%s" % p)
def rig(request, sim):
    return Rig(sim, *request.param)


# ---- posterize -----------------------------------------------------------------------------------------------------

def test_posterize_every_threshhold_in_one_call(rig):
    post = ntscsim.Posterizer(ALL_THRESHHOLDS, width=rig.w, height=rig.h, sim=rig.sim)
    frames = [rig.noise() for _ in range(9)]
    frames[8][...] = 0xFF                                                         # the mask itself comes out
    src = [rig.put(rig.sgeo, f) for f in frames]
    dst = [rig.put(rig.dgeo) for _ in frames]
    post.frames([(dst[t][3], src[t][3], t) for t in range(9)])
    post.sync()
    assert post.last_kernels() == ["k_post_frames"]
    for t in range(9):
        rig.same(dst[t], rig.dgeo, R.posterize(frames[t], t), "threshhold %d" % t)
        rig.untouched(src[t], "source %d" % t)
    assert not R.posterize(frames[0], 0).any() and (R.posterize(frames[7], 8) == frames[7]).all()


def test_posterize_in_place_and_two_layers_on_one_destination(rig):
    post = ntscsim.Posterizer(["-i", "a", "-threshhold", "2", "-i", "b", "-threshhold", "5"], width=rig.w, height=rig.h, sim=rig.sim)
    fa, fb = rig.noise(), rig.noise()
    a = rig.put(rig.dgeo, fa)
    post.frames([(a[3], a[3], 0)])
    post.sync()
    rig.same(a, rig.dgeo, R.posterize(fa, 2), "in place")
    # the tool's loop: every input in turn onto one output frame; the last one stands, in either order
    a, b, out = rig.put(rig.sgeo, fa), rig.put(rig.sgeo, fb), rig.put(rig.dgeo)
    post.frames([(out[3], a[3], 0), (out[3], b[3], 1)])
    post.sync()
    assert post.last_kernels() == ["k_post_frames"] * 2
    rig.same(out, rig.dgeo, R.posterize_loop([fa, fb], [2, 5]), "two layers")
    post.frames([(out[3], b[3], 1), (out[3], a[3], 0)])
    post.sync()
    rig.same(out, rig.dgeo, R.posterize(fa, 2), "two layers, the other order")
    assert (R.posterize(fa, 2) != R.posterize(fb, 5)).any()
    post.frames([(out[3], b[3])])                                       # no index: the last input
    post.sync()
    rig.same(out, rig.dgeo, R.posterize(fb, 5), "default layer")


def test_posterize_host_frames_equal_device_call(rig):
    post = ntscsim.Posterizer(ALL_THRESHHOLDS, width=rig.w, height=rig.h, sim=rig.sim)
    frames = [rig.noise() for _ in range(3)]
    src = [rig.put(rig.sgeo, f) for f in frames]
    dst = [rig.put(rig.dgeo) for _ in frames]
    ts = (1, 3, 6)
    post.frames([(d[3], s[3], t) for d, s, t in zip(dst, src, ts)])
    post.sync()
    host = [rig.host_copy(d, rig.dgeo) for d in dst]
    post.frames_host([(hv, s[1], t) for (_, hv), s, t in zip(host, src, ts)])
    assert post.last_kernels() == ["k_post_frames"]
    for i in range(3):
        assert int((dst[i][2].cpu().numpy() != host[i][0]).sum()) == 0, "host call, frame %d" % i
        assert int((host[i][1] != R.posterize(frames[i], ts[i])).sum()) == 0
        assert int((src[i][1] != frames[i]).sum()) == 0
    # b = post(a), c = post(b) on host arrays: the second reads what the first wrote, a batch and a launch each
    a, b, c = frames[0].copy(), np.full_like(frames[0], 0x11), np.full_like(frames[0], 0x22)
    post.frames_host([(b, a, 6), (c, b, 3)])
    assert post.last_kernels() == ["k_post_frames"] * 2
    assert (b == R.posterize(frames[0], 6)).all() and (c == R.posterize(frames[0], 3)).all()


# ---- colormap ------------------------------------------------------------------------------------------------------

CLIP_MAPS = [None, 0, None, None, 1, 2, None]


def cmap_clip(rig):
    """(sources, maps per frame (None: absent), entry table, [(output, table behind the frame)] by the checker)"""
    frames = [rig.noise() for _ in CLIP_MAPS]
    pool = [rig.noise() for _ in range(3)]
    maps = [None if m is None else pool[m] for m in CLIP_MAPS]
    entry = rig.rng.randint(0, 1 << 32, size=256, dtype=np.uint64).astype(np.uint32)
    s = R.ColorStream(entry)
    want = []
    for f, m in zip(frames, maps):
        out = s.frame(f, m)
        want.append((out, s.table.copy()))
    return frames, maps, entry, want


def run_clip(rig, cm, frames, maps, cuts, host=False):
    """The clip through calls that end at `cuts`; returns the destinations (and what must not have been written)."""
    src = [rig.put(rig.sgeo, f) for f in frames]
    mp = [None if m is None else rig.put(rig.sgeo, m) for m in maps]
    dst = [rig.put(rig.dgeo) for _ in frames]
    hosts = [rig.host_copy(d, rig.dgeo) for d in dst]
    kernels, first = [], 0
    for end in cuts:
        if host:
            cm.frames_host([(hosts[i][1], src[i][1], None if mp[i] is None else mp[i][1]) for i in range(first, end)])
        else:
            cm.frames([(dst[i][3], src[i][3], None if mp[i] is None else mp[i][3]) for i in range(first, end)])
        kernels.append(cm.last_kernels())
        first = end
    cm.sync()
    return src, mp, dst, hosts, kernels


def test_colormap_clip_in_one_call_and_split(rig):
    """State at entry (a table that was set), carried inside a launch group, and left behind the call; then the same
    clip as calls of 3 + 4 frames: the same bytes and the same table."""
    cm = ntscsim.ColorMapper(width=rig.w, height=rig.h, sim=rig.sim)
    frames, maps, entry, want = cmap_clip(rig)
    assert (cm.table == R.identity_table()).all()                                 # bind resets
    cm.table = entry
    src, mp, dst, _, kernels = run_clip(rig, cm, frames, maps, [7])
    assert kernels == [["k_cmap_frames", "k_cmap_take"]]
    for i in range(7):
        rig.same(dst[i], rig.dgeo, want[i][0], "one call, frame %d" % i)
        rig.untouched(src[i], "source %d" % i)
        if mp[i] is not None:
            rig.untouched(mp[i], "map %d" % i)
    assert (cm.table == want[-1][1]).all() and (want[-1][1] == R.take(maps[5])).all()
    assert (want[0][0] == R.apply(frames[0], entry)).all()                        # frame 0 went by the entry table
    cm.table = entry
    src, mp, dst2, _, kernels = run_clip(rig, cm, frames, maps, [3, 7])
    assert kernels == [["k_cmap_frames", "k_cmap_take"]] * 2
    for i in range(7):
        rig.same(dst2[i], rig.dgeo, want[i][0], "3 + 4, frame %d" % i)
    assert (cm.table == want[-1][1]).all()
    # a call without a map leaves the table alone and launches no k_cmap_take
    run_clip(rig, cm, frames[:1], [None], [1])
    assert cm.last_kernels() == ["k_cmap_frames"] and (cm.table == want[-1][1]).all()


def test_colormap_set_table_and_reset(rig):
    cm = ntscsim.ColorMapper(width=rig.w, height=rig.h, sim=rig.sim)
    f = rig.noise()
    table = rig.rng.randint(0, 1 << 32, size=256, dtype=np.uint64).astype(np.uint32)
    cm.table = table
    assert (cm.table == table).all()
    src, dst = rig.put(rig.sgeo, f), rig.put(rig.dgeo)
    cm.frames([(dst[3], src[3], None)])
    rig.same(dst, rig.dgeo, R.apply(f, table), "set table")
    cm.reset()
    assert (cm.table == R.identity_table()).all()
    cm.frames([(dst[3], src[3], None)])
    rig.same(dst, rig.dgeo, np.repeat(f[:, :, 1:2], 4, axis=2), "identity grey")
    with pytest.raises(ntscsim.NtscsimError):
        cm.table = table[:255]


def test_colormap_map_written_by_an_earlier_descriptor_and_in_place(rig):
    """Job 1's map is what job 0 wrote: it goes into a later launch group, behind job 0's k_cmap_frames (which had no
    map, so no k_cmap_take follows it)."""
    cm = ntscsim.ColorMapper(width=rig.w, height=rig.h, sim=rig.sim)
    f0, f1 = rig.noise(), rig.noise()
    table = rig.rng.randint(0, 1 << 32, size=256, dtype=np.uint64).astype(np.uint32)
    cm.table = table
    a, b = rig.put(rig.sgeo, f0), rig.put(rig.sgeo, f1)
    mid, out = rig.put(rig.sgeo), rig.put(rig.dgeo)
    cm.frames([(mid[3], a[3], None), (out[3], b[3], mid[3])])
    cm.sync()
    assert cm.last_kernels() == ["k_cmap_frames", "k_cmap_frames", "k_cmap_take"]
    made = R.apply(f0, table)
    rig.same(mid, rig.sgeo, made, "the map that was made")
    rig.same(out, rig.dgeo, R.apply(f1, R.take(made)), "the frame mapped by it")
    assert (cm.table == R.take(made)).all()
    # in place, with a map
    m = rig.noise()
    c, mp = rig.put(rig.dgeo, f0), rig.put(rig.sgeo, m)
    cm.frames([(c[3], c[3], mp[3])])
    rig.same(c, rig.dgeo, R.apply(f0, R.take(m)), "in place")
    # a destination on the middle row of its own map
    with pytest.raises(ntscsim.NtscsimError) as e:
        cm.frames([(mp[3], a[3], mp[3])])
    assert e.value.code == _capi.E_ARG
    rig.untouched(mp, "the refused map")


def test_colormap_host_frames_equal_device_call(rig):
    cm = ntscsim.ColorMapper(width=rig.w, height=rig.h, sim=rig.sim)
    frames, maps, entry, want = cmap_clip(rig)
    cm.table = entry
    src, mp, dst, hosts, kernels = run_clip(rig, cm, frames, maps, [3, 7], host=True)
    assert kernels == [["k_cmap_frames", "k_cmap_take"]] * 2
    assert (cm.table == want[-1][1]).all()
    cm.table = entry
    cm.frames([(dst[i][3], src[i][3], None if mp[i] is None else mp[i][3]) for i in range(7)])
    cm.sync()
    for i in range(7):
        # the host buffers started as copies of the device buffers: every byte is the same, guard bytes included
        assert int((dst[i][2].cpu().numpy() != hosts[i][0]).sum()) == 0, "host call, frame %d" % i
        assert int((hosts[i][1] != want[i][0]).sum()) == 0, "host call against the checker, frame %d" % i
        assert int((src[i][1] != frames[i]).sum()) == 0
        assert mp[i] is None or int((mp[i][1] != maps[i]).sum()) == 0


def test_host_call_leaves_guard_bytes_alone(sim):
    import torch  # noqa: F401
    w, h = 37, 5
    rig = Rig(sim, w, h, "unaligned")
    cm = ntscsim.ColorMapper(width=w, height=h, sim=sim)
    f, m = rig.noise(), rig.noise()
    buf, view = host_frame(w, h, 4 * w + 7, 3, None, 77)                          # a linesize and a base no device call takes
    before = buf.copy()
    cm.frames_host([(view, f, m)])
    want = before.copy()
    np.lib.stride_tricks.as_strided(want[3:], shape=(h, w, 4), strides=(4 * w + 7, 4, 1))[...] = R.apply(f, R.take(m))
    assert (buf == want).all()


# ---- both ----------------------------------------------------------------------------------------------------------

def test_simulator_output_is_mapped_without_leaving_the_device():
    """A few -vhs fields from ntscsim_fields_device stay in device memory and are the sources (and the map) of the two
    stages: the results are the checker applied to the simulator's downloaded output."""
    import torch
    w, h, n = 96, 32, 4
    fs = ntscsim.FieldSimulator(params=L.make_params(["-vhs"]), device=0)
    try:
        post = ntscsim.Posterizer(["-i", "sim", "-threshhold", "2"], width=w, height=h, sim=fs)
        cm = ntscsim.ColorMapper(width=w, height=h, sim=fs)
        frames = np.stack([L.noise_frame(w, h, 0x91 + i) for i in range(n // 2)])
        jobs = [(k // 2, k, (k & 1) ^ 1, k) for k in range(n)]
        src = torch.from_numpy(frames).cuda()
        fields = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
        fs.fields(src, fields, jobs)
        out = torch.zeros((2, n, h, w, 4), dtype=torch.uint8, device="cuda")
        post.frames([(out[0, t], fields[t]) for t in range(n)])
        assert post.last_kernels() == ["k_post_frames"]
        cm.frames([(out[1, t], fields[t], fields[0] if t == 1 else None) for t in range(n)])
        assert cm.last_kernels() == ["k_cmap_frames", "k_cmap_take"]
        cm.sync()
        sim_out = fields.cpu().numpy()
        got = out.cpu().numpy()
        s = R.ColorStream()
        for t in range(n):
            assert int((got[0, t] != R.posterize(sim_out[t], 2)).sum()) == 0
            assert int((got[1, t] != s.frame(sim_out[t], sim_out[0] if t == 1 else None)).sum()) == 0
        assert (sim_out[:, :, :, :3] & 0x3F).any()                                # the posteriser had bits to clear
    finally:
        fs.close()


def test_error_codes():
    import torch
    fs = ntscsim.FieldSimulator(device=0)
    try:
        lib = fs._lib
        for stage, desc in (("post", _capi.PostDesc), ("cmap", _capi.CmapDesc)):
            d = desc()
            assert getattr(lib, "ntscsim_%s_frames_device" % stage)(fs._h, C.byref(d), 1, None) == _capi.E_ARG    # no bind
            assert getattr(lib, "ntscsim_%s_frames_host" % stage)(fs._h, C.byref(d), 1) == _capi.E_ARG
        table = (C.c_uint32 * 256)()
        assert lib.ntscsim_cmap_reset(fs._h) == _capi.E_ARG and lib.ntscsim_cmap_get_table(fs._h, table) == _capi.E_ARG
        assert lib.ntscsim_cmap_set_table(fs._h, table) == _capi.E_ARG
        for cls, flags in ((ntscsim.Posterizer, ["-i", "a"]), (ntscsim.ColorMapper, [])):
            for wh in ((0, 1), (1, 0), (16385, 16), (16, 16385), (-1, -1)):
                with pytest.raises(ntscsim.NtscsimError) as e:
                    cls(flags, width=wh[0], height=wh[1], sim=fs)
                assert e.value.code == _capi.E_SIZE, wh
        with pytest.raises(ntscsim.NtscsimError) as e:
            ntscsim.Posterizer(["-i", "a", "-threshhold", "9"], width=16, height=16, sim=fs)
        assert e.value.code == _capi.E_PARAM
        post = ntscsim.Posterizer(["-i", "a", "-i", "b"], width=96, height=32, sim=fs)
        cm = ntscsim.ColorMapper(width=96, height=32, sim=fs)
        assert lib.ntscsim_cmap_get_table(fs._h, None) == _capi.E_ARG and lib.ntscsim_cmap_set_table(fs._h, None) == _capi.E_ARG
        a, b, m = (torch.zeros((32, 96, 4), dtype=torch.uint8, device="cuda") for _ in range(3))
        small = torch.zeros((32, 64, 4), dtype=torch.uint8, device="cuda")
        wide = torch.zeros((32, 97, 4), dtype=torch.uint8, device="cuda")
        odd = torch.as_strided(wide, (32, 96, 4), (386, 4, 1), 0)                  # linesize not a multiple of 4
        narrow = torch.as_strided(wide, (32, 96, 4), (380, 4, 1), 0)               # linesize below 4 * width
        off2 = torch.as_strided(wide.view(-1), (32, 96, 4), (388, 4, 1), 2)        # a pointer that is not a multiple of 4
        big = torch.zeros((40, 96, 4), dtype=torch.uint8, device="cuda")

        def code(stage, jobs):
            with pytest.raises(ntscsim.NtscsimError) as e:
                stage.frames(jobs)
            return e.value.code

        for stage, extra in ((post, (0,)), (cm, (None,))):
            assert code(stage, [(small, small.clone()) + extra]) == _capi.E_SIZE   # not the bound size
            for bad in (odd, narrow, off2):
                assert code(stage, [(bad, b) + extra]) == _capi.E_SIZE and code(stage, [(a, bad) + extra]) == _capi.E_SIZE
            assert code(stage, [(big[:32], big[8:]) + extra]) == _capi.E_ARG       # overlapping by some rows
            assert code(stage, [(b, a) + extra, (big[:32], big[8:]) + extra]) == _capi.E_ARG   # checked before anything is launched
            stage.frames([(a, a) + extra])                                         # in place is not an overlap
            stage.frames([])
        assert code(post, [(b, a, 2)]) == _capi.E_ARG and code(post, [(b, a, -1)]) == _capi.E_ARG   # layer outside the bound list
        for bad in (odd, narrow, off2):
            assert code(cm, [(b, a, bad)]) == _capi.E_SIZE
        assert code(cm, [(m, a, m)]) == _capi.E_ARG                                # dst is the map
        assert code(cm, [(big[:32], a, big[8:])]) == _capi.E_ARG                   # dst covers the map's middle row
        tall = torch.zeros((60, 96, 4), dtype=torch.uint8, device="cuda")
        cm.frames([(tall[:32], a, tall[20:52])])                               # dst overlaps the map, not its middle row
        pd = (_capi.PostDesc * 1)()
        pd[0].dst, pd[0].dst_linesize, pd[0].src_linesize = a.data_ptr(), 384, 384
        assert lib.ntscsim_post_frames_device(fs._h, pd, 1, None) == _capi.E_ARG   # NULL source
        assert lib.ntscsim_post_frames_device(fs._h, None, 1, None) == _capi.E_ARG
        assert lib.ntscsim_post_frames_device(fs._h, pd, -1, None) == _capi.E_ARG
        cd = (_capi.CmapDesc * 1)()
        cd[0].src, cd[0].dst_linesize, cd[0].src_linesize = a.data_ptr(), 384, 384
        assert lib.ntscsim_cmap_frames_device(fs._h, cd, 1, None) == _capi.E_ARG   # NULL destination
        assert lib.ntscsim_cmap_frames_host(fs._h, cd, 1) == _capi.E_ARG
        fs.sync()
    finally:
        fs.close()
