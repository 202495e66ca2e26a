"""The host half of the frameblend stage (ntscsim_blend_params / _parse_argv / _frame_time / _plan_* / _tables) and
its checker tests/_blend_ref.py, against tests/golden/frameblend_golden.npz (no GPU needed).

Pinning: the table and planner fixtures come from the reference's own lines, built with libc / STL headers only
(frameblend.cpp:44-51, :685-732, :929-1030; tests/golden/make_golden_frameblend.py) -- they pin both the library and
the checker.  The pixel fixtures (:1032-1081) needed a two-member AVFrame stand-in to build and are therefore
UNPINNED by this project's rule: they are compared all the same.  parse_argv() (:512-634) does not extract without
libav (it touches new_input_file() and output_file), so its expected values below are derived BY HAND from the cited
lines."""
import ctypes as C
import os

import numpy as np
import pytest

import _blend_ref as R
import _libs as L
import ntscsim
from ntscsim import _capi

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frameblend_golden.npz"))
PLAN_CASES = sorted(k[len("plan_"):-len("_args")] for k in GOLD.files if k.startswith("plan_") and k.endswith("_args"))
PIX_CASES = sorted(k[len("px_"):-len("_out")] for k in GOLD.files if k.startswith("px_") and k.endswith("_out"))


def parse(flags, require_io=False):
    lib = L.product()
    p = _capi.BlendParams()
    lib.ntscsim_blend_params_init(C.byref(p))
    argv = [b"frameblend"] + [f.encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    return lib.ntscsim_blend_parse_argv(C.byref(p), len(argv), arr, int(require_io)), p


def test_defaults_are_the_reference_globals():
    """:44-57 and preset_NTSC() :491-494"""
    rc, p = parse([])
    assert rc == _capi.OK and p.struct_size == C.sizeof(_capi.BlendParams)
    assert (p.rate_num, p.rate_den, p.output_width, p.output_height) == (60000, 1001, -1, -1)
    assert (p.squelch_near_match, p.fullframealt, p.framealt, p.underscan, p.use_422_colorspace) == (0, 0, 1, 0, 0)
    assert p.gamma_correction == -1 and p.n_inputs == 0 and p.input_path is None and p.output_path is None


@pytest.mark.parametrize("arg, num, den", [
    ("29.97", 299700, 10000),        # strtof(29.97) = 29.969999..., x 10000 + 0.5 floors to 299700 (:591-592)
    ("30000/1001", 30000, 1001),     # d > 1: floor(n + 0.5) over d (:586-589)
    ("3", 50000, 10000),             # below 5 fps: n = 5, d = 1 (:581-584), then the bare-number form
    ("24:1", 240000, 10000),         # d = 1 is not "> 1": stored x 10000 (:590-593)
    ("60000\\1001", 60000, 1001),    # the third separator (:572)
    ("23.976", 239760, 10000),
    ("50/0", 500000, 10000),         # d < 1 -> 1 (:575)
    ("-7", 50000, 10000),            # n < 0 -> 0 (:578), then the floor
    ("9/2", 50000, 10000),           # 4.5 fps: floor
    ("11/2", 11, 2),
])
def test_or_forms(arg, num, den):
    rc, p = parse(["-or", arg])
    assert rc == _capi.OK and (p.rate_num, p.rate_den) == (num, den)


def test_every_switch():
    rc, p = parse(["-width", "720", "--height", "0x1e6", "-sqnr", "-ffa", "-fa", "3", "-gamma", "1.8", "-underscan", "7",
                   "-422", "-i", "a.avi", "-i", "b.avi", "-o", "out.mkv", "-or", "25"], require_io=True)
    assert rc == _capi.OK
    assert (p.output_width, p.output_height) == (720, 486)           # strtoul(.., 0): hex accepted (:529, :535)
    assert (p.squelch_near_match, p.fullframealt, p.framealt) == (1, 1, 3)
    assert p.gamma_correction == 1.8 and p.underscan == 7 and p.use_422_colorspace == 1
    assert p.n_inputs == 2 and p.input_path == b"b.avi" and p.output_path == b"out.mkv"
    assert (p.rate_num, p.rate_den) == (250000, 10000)
    assert parse(["-422", "-420"])[1].use_422_colorspace == 0


def test_clamps_and_gamma_names():
    assert parse(["-fa", "0"])[1].framealt == 1 and parse(["-fa", "-3"])[1].framealt == 1       # :548-550
    assert parse(["-fa", "8"])[1].framealt == 8 and parse(["-fa", "99"])[1].framealt == 8
    assert parse(["-underscan", "-1"])[1].underscan == 0 and parse(["-underscan", "500"])[1].underscan == 99   # :603-605
    assert parse(["-gamma", "ntsc"])[1].gamma_correction == 2.2 and parse(["-gamma", "vga"])[1].gamma_correction == 2.2
    assert parse(["-gamma", "pal"])[1].gamma_correction == -1        # neither a digit nor a known name: unchanged (:556-559)
    assert parse(["-gamma", ".5"])[1].gamma_correction == -1         # isdigit('.') is false
    assert parse(["-gamma", "2.4"])[1].gamma_correction == 2.4


@pytest.mark.parametrize("flags, code", [
    (["-h"], _capi.E_HELP), (["--help"], _capi.E_HELP),
    (["-bogus"], _capi.E_FLAG), (["stray"], _capi.E_FLAG),
    (["-width", "31"], _capi.E_FLAG), (["-height", "16"], _capi.E_FLAG), (["-width", "-5"], _capi.E_FLAG),
    (["-width"], _capi.E_FLAG), (["-fa"], _capi.E_FLAG), (["-gamma"], _capi.E_FLAG), (["-or"], _capi.E_FLAG),
    (["-i"], _capi.E_FLAG), (["-o"], _capi.E_FLAG), (["-underscan"], _capi.E_FLAG),
])
def test_rejections(flags, code):
    assert parse(flags)[0] == code


def test_io_checks():
    """:624-631, applied with require_io"""
    assert parse(["-i", "a"], require_io=True)[0] == _capi.E_FLAG
    assert parse(["-o", "b"], require_io=True)[0] == _capi.E_FLAG
    assert parse(["-i", "a", "-o", "b"], require_io=True)[0] == _capi.OK
    assert parse([], require_io=False)[0] == _capi.OK


def test_frame_time_two_roundings():
    """:100-110 -- multiply by one integer product, divide by the other; not pts * (a / b)."""
    lib = L.product()
    for orate in ((60000, 1001), (599400, 10000), (50000, 10000)):
        _, p = parse([])
        p.rate_num, p.rate_den = orate
        for tb in ((1001, 24000), (1, 25), (1, 90000), (1001, 30000)):
            for pts in (0, 1, 7, 1001, 123457, 2 ** 40 + 3):
                got = lib.ntscsim_blend_frame_time(pts, tb[0], tb[1], C.byref(p))
                assert got == R.frame_time(pts, tb[0], tb[1], orate[0], orate[1])
    _, p = parse([])
    assert lib.ntscsim_blend_frame_time(3, 1001, 24000, C.byref(p)) == 3.0 * (1001 * 60000) / (24000 * 1001)


@pytest.mark.parametrize("gi", range(4))
def test_tables_equal_the_reference(gi):
    g = float(GOLD["tab_gamma"][gi])
    dec, enc = (C.c_uint16 * 256)(), (C.c_uint8 * 8193)()
    assert L.product().ntscsim_blend_tables(g, dec, enc) == _capi.OK
    assert np.array_equal(np.frombuffer(dec, dtype=np.uint16), GOLD["tab_dec"][gi])
    assert np.array_equal(np.frombuffer(enc, dtype=np.uint8), GOLD["tab_enc"][gi])
    rdec, renc = R.tables(g)
    assert np.array_equal(rdec, GOLD["tab_dec"][gi]) and np.array_equal(renc, GOLD["tab_enc"][gi])


def test_tables_reject_bad_gamma():
    dec, enc = (C.c_uint16 * 256)(), (C.c_uint8 * 8193)()
    assert L.product().ntscsim_blend_tables(0.0, dec, enc) == _capi.E_PARAM
    assert L.product().ntscsim_blend_tables(-1.0, dec, enc) == _capi.E_PARAM


def _golden_plan(name):
    n, ids, w16 = GOLD["plan_%s_n" % name], GOLD["plan_%s_ids" % name], GOLD["plan_%s_w16" % name]
    out, at = [], 0
    for k in n:
        out.append(([int(x) for x in ids[at:at + k]], [int(x) for x in w16[at:at + k]]))
        at += k
    return out


def _params_of(name):
    rn, rd, sqnr, ffa, fa = [int(x) for x in GOLD["plan_%s_args" % name]]
    _, p = parse([])
    p.rate_num, p.rate_den, p.squelch_near_match, p.fullframealt, p.framealt = rn, rd, sqnr, ffa, fa
    return p


@pytest.mark.parametrize("name", PLAN_CASES)
def test_planner_equals_the_reference(name):
    """Period by period: stable ids and weight16 of the library's planner and of the checker == the reference's scan
    driven with the same read-ahead and erase."""
    want = _golden_plan(name)
    times = [float(x) for x in GOLD["plan_%s_times" % name]]
    p = _params_of(name)
    assert len(want) == R.clip_periods(times[-1]) == L.product().ntscsim_blend_clip_periods(times[-1])
    got = ntscsim.blend_plan(p, times)
    ref = R.plan_clip(times, p.squelch_near_match, p.fullframealt, p.framealt)
    for cur, (w, g, r) in enumerate(zip(want, got, ref)):
        assert g == w, "library, period %d" % cur
        assert r == w, "checker, period %d" % cur
    assert len(got) == len(want) and len(ref) == len(want)


def test_fixture_covers_the_cases():
    need = {"film_to_ntsc", "pal_to_ntsc", "r30_to_ntsc", "r30_to_ntsc_sqnr", "near_match_sqnr", "nearer_match_sqnr",
            "r60_to_24", "r120_to_5", "fa2", "fa3_ffa", "jitter", "single", "long_fa2"}
    assert need <= set(PLAN_CASES)
    assert max(GOLD["plan_r60_to_24_n"]) > 2 and max(GOLD["plan_r120_to_5_n"]) >= 20
    assert len(GOLD["plan_long_fa2_times"]) >= 200 and int((GOLD["plan_long_fa2_cutoff"] >= 32).sum()) >= 3
    assert GOLD["plan_near_match_sqnr_w16"].tolist() != GOLD["plan_near_match_w16"].tolist()


def test_planner_release_and_small_cap():
    """release_below follows the erase (ids stay stable), and a too small `cap` leaves the state unchanged."""
    lib = L.product()
    name = "long_fa2"
    times = [float(x) for x in GOLD["plan_%s_times" % name]]
    want = _golden_plan(name)
    h = C.c_void_p()
    assert lib.ntscsim_blend_plan_create(C.byref(_params_of(name)), C.byref(h)) == _capi.OK
    for k, t in enumerate(times):
        assert lib.ntscsim_blend_plan_push(h, t) == k
    ids, w16, n, rel = (C.c_int64 * 8)(), (C.c_uint32 * 8)(), C.c_int(0), C.c_int64(-1)
    releases = []
    for cur in range(len(want)):
        if len(want[cur][0]) > 0:
            assert lib.ntscsim_blend_plan_next(h, cur, ids, w16, len(want[cur][0]) - 1, C.byref(n), C.byref(rel)) == _capi.E_SIZE
            assert n.value == len(want[cur][0])
        assert lib.ntscsim_blend_plan_next(h, cur, ids, w16, 8, C.byref(n), C.byref(rel)) == _capi.OK
        assert ([ids[k] for k in range(n.value)], [w16[k] for k in range(n.value)]) == want[cur]
        assert all(i >= rel.value for i in want[cur][0])
        releases.append(rel.value)
    assert releases == sorted(releases) and len(set(releases)) >= 4 and releases[-1] >= 96
    lib.ntscsim_blend_plan_reset(h)
    assert lib.ntscsim_blend_plan_push(h, 0.0) == 0
    lib.ntscsim_blend_plan_destroy(h)


@pytest.mark.parametrize("name", PIX_CASES)
def test_checker_pixels_equal_the_reference_loop(name):
    """UNPINNED (see the module docstring): the checker's pixel function against frames the reference's loops
    :1032-1081 rendered -- gamma and plain, widths that are and are not multiples of 4, weights summing to 65535,
    65536, 65537 and beyond (the clamps)."""
    src, w16, g = GOLD["px_%s_src" % name], GOLD["px_%s_w16" % name], float(GOLD["px_%s_gamma" % name])
    got = R.blend_pixels([s for s in src], [int(x) for x in w16], g)
    assert np.array_equal(got, GOLD["px_%s_out" % name])


def test_pixel_fixture_covers_the_cases():
    sums = {int(GOLD["px_%s_w16" % n].astype(np.int64).sum()) for n in PIX_CASES}
    assert {65535, 65536, 65537} <= sums
    assert any(GOLD["px_%s_src" % n].shape[2] % 4 for n in PIX_CASES)
    assert any(float(GOLD["px_%s_gamma" % n]) > 1 for n in PIX_CASES) and any(float(GOLD["px_%s_gamma" % n]) < 1 for n in PIX_CASES)


def test_blend_kernels_use_no_scratch_memory():
    """Code-object metadata of csrc/ntsc_blend.o (as test_no_product_kernel_uses_scratch_memory does for the other device
    objects): all eight forms, no private segment, no spill, and the gamma forms hold exactly the two tables in LDS."""
    import shutil
    import subprocess
    obj = os.path.join(L.ROOT, "composite-video-simulator_amd", "csrc", "ntsc_blend.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("device object or llvm tools not present")
    out = subprocess.run(["sh", os.path.join(L.ROOT, "tools", "kres.sh"), obj], cwd=L.ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr
    rows = [l for l in out.stdout.splitlines() if "\t" in l and "ntscsim::k_blend_" in l]
    assert len(rows) == 8, out.stdout
    bad = [l for l in rows if " scratch 0 " not in l + " " or not l.rstrip().endswith("spill 0")]
    assert not bad, "\n".join(bad)
    for l in rows:
        assert (" lds 8720 " in l) == ("<true," in l), l         # 512 bytes dec + 8196 bytes enc (+ alignment)
