"""The device half of the frameblend stage (ntscsim_blend_frames_device / _clip_device / _frames_host, the
frameblend_cli host and the hand-off into the field simulator) against the checker tests/_blend_ref.py, byte for
byte: the stage is integer arithmetic on tables computed by the same libm call, so the tolerance is zero."""
import os
import subprocess

import numpy as np
import pytest

import _blend_ref as R
import _libs as L
import ntscsim

pytestmark = pytest.mark.gpu

CLI = os.path.join(L.PKG, "frameblend_cli")
PAD = 0xA5


def host_frame(w, h, ls, off, seed):
    """A frame inside a padded byte buffer: rows of `ls` bytes starting `off` bytes in; everything random."""
    buf = np.random.RandomState(seed).randint(0, 256, size=off + h * ls + 16, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w, 4), strides=(ls, 4, 1))
    return buf, view


def dev_view(torch, buf, w, h, ls, off):
    t = torch.from_numpy(buf).cuda()
    return t, torch.as_strided(t, (h, w, 4), (ls, 4, 1), off)


SIZES = [(96, 32), (100, 35), (720, 486), (1920, 1080)]
# rows 16-byte aligned (the vector path) | linesize and base pointer only 4-byte aligned (the dword path)
LAYOUTS = {"aligned": (0, 0), "unaligned": (4, 4)}


@pytest.mark.parametrize("gamma", [2.2, None], ids=["gamma", "plain"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("w, h", SIZES)
def test_frames_device_equals_checker(w, h, layout, gamma):
    """Fast form for 0, 1, 2, 3, 4 taps (one of them with a weight of 0), the 64-bit fast form forced by weights that
    break the u32 bound, general form for 5 and 40 taps: every byte of every destination buffer, row padding
    included, and the kernel names."""
    import torch
    extra, off = LAYOUTS[layout]
    ls = 4 * w + extra + (16 if layout == "aligned" else 0)          # padded rows in both layouts
    nsrc = 8
    srcs = [host_frame(w, h, ls, off, 100 + k) for k in range(nsrc)]
    dsrc = [dev_view(torch, b, w, h, ls, off) for b, _ in srcs]
    fb = ntscsim.FrameBlender(("-gamma", repr(gamma)) if gamma else ())
    g = "true" if gamma else "false"

    def taps(n, seed):
        rs = np.random.RandomState(seed)
        cut = np.sort(rs.randint(0, 65537, size=n - 1)) if n > 1 else np.array([], dtype=np.int64)
        wts = np.diff(np.concatenate([[0], cut, [65536]])).tolist()
        return [((seed + 3 * k) % nsrc, int(x)) for k, x in enumerate(wts)]

    groups = {
        "k_blend_fast<%s,false>" % g: [[], taps(1, 1), taps(2, 2), taps(3, 3), taps(4, 4), [(1, 65536), (5, 0)],
                                        [(2, 30000), (6, 35537)], [(3, 20000), (0, 45535)]],
        "k_blend_fast<%s,true>" % g: [[(0, 9000000), (4, 9000001)], taps(2, 9)],
        "k_blend_general<%s,false>" % g: [taps(5, 5), taps(40, 6), taps(2, 7)],
        "k_blend_general<%s,true>" % g: [taps(5, 8) + [(7, 20000000)]],
    }
    try:
        for kernel, lists in groups.items():
            dst = [host_frame(w, h, ls, off, 900 + i) for i in range(len(lists))]
            ddst = [dev_view(torch, b, w, h, ls, off) for b, _ in dst]
            fb.blend_frames([(ddst[i][1], [(dsrc[s][1], wt) for s, wt in tl]) for i, tl in enumerate(lists)])
            fb.sync()
            assert fb.last_kernels() == [kernel]
            for i, tl in enumerate(lists):
                want_buf = dst[i][0].copy()
                want = np.lib.stride_tricks.as_strided(want_buf[off:], shape=(h, w, 4), strides=(ls, 4, 1))
                want[...] = R.blend_frame((h, w), [srcs[s][1] for s, _ in tl], [wt for _, wt in tl], gamma)
                got = ddst[i][0].cpu().numpy()
                bad = int((got != want_buf).sum())
                assert bad == 0, "%s desc %d (%d taps): %d bytes differ" % (kernel, i, len(tl), bad)
        for k, (b, _) in enumerate(srcs):                             # sources untouched
            assert int((dsrc[k][0].cpu().numpy() != b).sum()) == 0
    finally:
        fb.close()


def test_argument_errors():
    import torch
    from ntscsim import _capi
    fb = ntscsim.FrameBlender()
    try:
        a = torch.zeros((32, 32, 4), dtype=torch.uint8, device="cuda")
        b = torch.zeros((32, 32, 4), dtype=torch.uint8, device="cuda")
        with pytest.raises(ntscsim.NtscsimError) as e:
            fb.blend_frames([(a, [(a, 65536)])])                     # destination is a source
        assert e.value.code == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:
            fb.blend_frames([(a, [(b, 0xFFFFFFFF)] * 65)])           # sum(weight16) >= 2^38
        assert e.value.code == _capi.E_ARG
        fb.blend_frames([])
    finally:
        fb.close()


def _clip(w, h, n, seed=5):
    return np.stack([R.noise_frame(w, h, seed + k) for k in range(n)])


def test_clip_device_host_and_cli_equal_checker(tmp_path):
    """48 frames of 720x486 at 24000/1001 -> 60000/1001 with -gamma ntsc: FrameBlender.blend, the host-frame call and
    frameblend_cli all give the checker's frames; the CLI writes the tool's number of frames."""
    import torch
    w, h, n = 720, 486, 48
    src = _clip(w, h, n)
    fb = ntscsim.FrameBlender(("-gamma", "ntsc"))
    try:
        times = fb.frame_times(n, 24000, 1001)
        assert times == [R.frame_time(k, 1001, 24000, 60000, 1001) for k in range(n)]
        plan = R.plan_clip(times)
        assert len(plan) == fb.n_out(times) == 119
        want = np.stack([R.blend_frame((h, w), [src[i] for i in ids], w16, 2.2) for ids, w16 in plan])

        dsrc = torch.from_numpy(src).cuda()
        out = torch.zeros((len(plan), h, w, 4), dtype=torch.uint8, device="cuda")
        fb.blend(dsrc, times, out)
        fb.sync()
        assert fb.last_kernels() == ["k_blend_fast<true,false>"]
        assert int((out.cpu().numpy() != want).sum()) == 0
        # a window of the clip: the planner still runs from period 0
        part = torch.zeros((10, h, w, 4), dtype=torch.uint8, device="cuda")
        fb.blend(dsrc, times, part, first=70, last=80)
        fb.sync()
        assert int((part.cpu().numpy() != want[70:80]).sum()) == 0

        hout = np.full((len(plan), h, w + 3, 4), PAD, dtype=np.uint8)      # padded destination rows
        fb.blend_frames_host([(hout[k][:, :w], [(src[i], wt) for i, wt in zip(ids, w16)]) for k, (ids, w16) in enumerate(plan)])
        assert int((hout[:, :, :w] != want).sum()) == 0 and int((hout[:, :, w:] != PAD).sum()) == 0
    finally:
        fb.close()

    fin, fout = tmp_path / "in.bgra", tmp_path / "out.bgra"
    src.tofile(str(fin))
    r = subprocess.run([CLI, "-i", str(fin), "-o", str(fout), "-width", str(w), "-height", str(h), "-ir", "24000/1001",
                        "-gamma", "ntsc"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    got = np.fromfile(str(fout), dtype=np.uint8)
    assert got.size == want.size, "frames written: %r" % (got.size / (w * h * 4),)
    assert int((got.reshape(want.shape) != want).sum()) == 0


def test_cli_long_clip_releases_frames(tmp_path):
    """200 frames with -fa 2: the planner erases three times and more, the CLI recycles the released device frames
    and still names the right ones."""
    w, h, n = 96, 32, 200
    src = _clip(w, h, n, seed=77)
    times = [R.frame_time(k, 1001, 24000, 60000, 1001) for k in range(n)]
    plan = R.plan_clip(times, fa=2)
    want = np.stack([R.blend_frame((h, w), [src[i] for i in ids], w16, None) for ids, w16 in plan])
    fin, fout = tmp_path / "in.bgra", tmp_path / "out.bgra"
    src.tofile(str(fin))
    r = subprocess.run([CLI, "-i", str(fin), "-o", str(fout), "-width", str(w), "-height", str(h), "-ir", "24000/1001",
                        "-fa", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    got = np.fromfile(str(fout), dtype=np.uint8)
    assert got.size == want.size and int((got.reshape(want.shape) != want).sum()) == 0


def test_blend_feeds_the_field_simulator():
    """Blend on the device, hand the output frames (never copied to the host) to FieldSimulator.fields with -vhs on the
    same context: the result is the NTSC oracle applied to the checker's frames."""
    import torch
    w, h, n = 96, 32, 8
    src = _clip(w, h, n, seed=31)
    p = L.make_params(["-vhs"])
    sim = ntscsim.FieldSimulator(params=p, device=0)
    fb = ntscsim.FrameBlender(("-gamma", "ntsc"), sim=sim)
    try:
        times = fb.frame_times(n, 24000, 1001)
        plan = R.plan_clip(times)
        nout = len(plan)
        frames = np.stack([R.blend_frame((h, w), [src[i] for i in ids], w16, 2.2) for ids, w16 in plan])
        jobs = [(k, k, (k & 1) ^ 1, k) for k in range(nout)]
        exp = np.zeros((nout, h, w, 4), np.uint8)
        o = L.OracleStream(p)
        for (si, di, field, fieldno) in jobs:
            o.field(exp[di], np.ascontiguousarray(frames[si]), field, fieldno)

        dsrc = torch.from_numpy(src).cuda()
        mid = torch.zeros((nout, h, w, 4), dtype=torch.uint8, device="cuda")
        dst = torch.zeros((nout, h, w, 4), dtype=torch.uint8, device="cuda")
        fb.blend(dsrc, times, mid)
        sim.fields(mid, dst, jobs)
        sim.sync()
        assert int((dst.cpu().numpy() != exp).sum()) == 0
        assert int((mid.cpu().numpy() != frames).sum()) == 0
    finally:
        fb.close()
        sim.close()
