"""Host half of the colorkey stage (csrc/key_params.cpp: ntscsim_key_params_*, _parse_argv, _rand_advance, the start
states of the draw kernel's lanes) and the checker tests/_key_ref.py against the fixtures generated from the
reference's own composite_layer() (tests/golden/make_golden_colorkey.py; AVFrame / InputFile stand-ins: unpinned).
No GPU.  The expected values of the parser are derived by hand from ffmpeg_colorkey.cpp:629-739, :68, :571-613."""
import ctypes as C
import os

import numpy as np
import pytest

import _key_ref as R
import _libs as L
import ntscsim
from ntscsim import _capi

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colorkey_golden.npz"))
CASES = sorted(k[3:-5] for k in GOLD.files if k.endswith("_geom"))
FIELDS = ("color", "threshhold", "fade", "xdivr", "invert", "noisekey")


def layers_of(p):
    return [tuple(int(getattr(p.layers[l], f)) for f in FIELDS) for l in range(p.n_layers)]


def test_defaults():
    p = _capi.make_key_params([])
    assert p.struct_size == C.sizeof(_capi.KeyParams)
    assert (p.width, p.height, p.tv_standard, p.delay, p.use_422_colorspace, p.n_layers) == (720, 480, 0, 1, 0, 0)   # :44-62, :606-613
    p = _capi.make_key_params(["-i", "a"])
    assert layers_of(p) == [(0, 0, 0, 1, 0, 0)] and p.layers[0].path == b"a"      # InputFile() :68


@pytest.mark.parametrize("flags, field, want", [
    (["-color", "0x8020C040"], "color", 0x8020C040), (["-color", "255"], "color", 255),
    (["-threshhold", "96"], "threshhold", 96), (["-threshhold", "-1"], "threshhold", -1),      # (int)strtoul :681
    (["-f", "128"], "fade", 128), (["-f", "300"], "fade", 300), (["-xd", "7"], "xdivr", 7), (["-xd", "0"], "xdivr", 0),
    (["-inv", "1"], "invert", 1), (["-inv", "0"], "invert", 0), (["-inv", "5"], "invert", 1),  # > 0 :676
    (["-noise", "2000"], "noisekey", 2000), (["--noise", "0x10"], "noisekey", 16),            # base 0, any number of dashes
])
def test_each_layer_switch(flags, field, want):
    p = _capi.make_key_params(["-i", "a"] + flags)
    assert int(getattr(p.layers[0], field)) == want
    others = dict(zip(FIELDS, (0, 0, 0, 1, 0, 0)))
    for f in FIELDS:
        if f != field:
            assert int(getattr(p.layers[0], f)) == others[f]


def test_global_switches():
    p = _capi.make_key_params(["-d", "256", "-width", "960", "-422", "-o", "out", "-i", "a"], require_io=True)
    assert (p.delay, p.width, p.height, p.use_422_colorspace, p.output_path) == (256, 960, 480, 1, b"out")
    p = _capi.make_key_params(["-422", "-420", "-d", "1"])
    assert (p.use_422_colorspace, p.delay) == (0, 1)
    p = _capi.make_key_params(["-width", "960", "-tvstd", "pal"])                  # preset_PAL() :597-604 resets the width
    assert (p.tv_standard, p.width, p.height) == (1, 720, 576)
    p = _capi.make_key_params(["-tvstd", "pal", "-tvstd", "ntsc"])
    assert (p.tv_standard, p.width, p.height) == (0, 720, 480)
    p = _capi.make_key_params(["-i", "a"], width=96, height=32)
    assert (p.width, p.height) == (96, 32)


def test_second_input_inherits_then_overrides():
    """new_input_file() :571-589 copies the last input, reset_on_dup() :90-92 clears only the path."""
    p = _capi.make_key_params(["-i", "a", "-color", "0x00FF00", "-threshhold", "96", "-f", "8", "-xd", "3", "-inv", "1",
                               "-noise", "500", "-i", "b", "-threshhold", "200", "-inv", "0", "-i", "c"])
    assert layers_of(p) == [(0x00FF00, 96, 8, 3, 1, 500), (0x00FF00, 200, 8, 3, 0, 500), (0x00FF00, 200, 8, 3, 0, 500)]
    assert [p.layers[l].path for l in range(3)] == [b"a", b"b", b"c"]
    many = []
    for k in range(40):                                                            # no limit on the layer count
        many += ["-i", "f%d" % k, "-threshhold", str(k)]
    p = _capi.make_key_params(many)
    assert p.n_layers == 40 and [int(p.layers[k].threshhold) for k in range(40)] == list(range(40))


@pytest.mark.parametrize("flags, code", [
    (["-d", "0"], _capi.E_FLAG), (["-d", "257"], _capi.E_FLAG), (["-width", "16"], _capi.E_FLAG),
    (["-tvstd", "secam"], _capi.E_FLAG), (["-bogus"], _capi.E_FLAG), (["stray"], _capi.E_FLAG), (["-i"], _capi.E_FLAG),
    (["-i", "a", "-noise"], _capi.E_FLAG), (["-h"], _capi.E_HELP), (["-help"], _capi.E_HELP),
    # a per-layer switch before any -i: the tool throws (current_input_file() :562-569)
    (["-f", "8", "-i", "a"], _capi.E_ARG), (["-xd", "2"], _capi.E_ARG), (["-noise", "5"], _capi.E_ARG),
    (["-inv", "1"], _capi.E_ARG), (["-threshhold", "3"], _capi.E_ARG), (["-color", "1"], _capi.E_ARG),
])
def test_refused(flags, code):
    with pytest.raises(ntscsim.NtscsimError) as e:
        _capi.make_key_params(flags)
    assert e.value.code == code


def test_require_io():
    for flags in (["-i", "a"], ["-o", "out"]):                                     # :729-736
        with pytest.raises(ntscsim.NtscsimError) as e:
            _capi.make_key_params(flags, require_io=True)
        assert e.value.code == _capi.E_FLAG


# ---- positions of the draws ------------------------------------------------------------------------------------

def _advance(p, pos, present=None):
    v = C.c_uint64(pos)
    pm = None if present is None else (C.c_uint8 * len(present))(*present)
    assert L.product().ntscsim_key_rand_advance(C.byref(p), pm, C.byref(v)) == _capi.OK
    return int(v.value)


@pytest.mark.parametrize("noisekeys", [(0,), (7,), (0, 5), (5, 0), (3, 4), (0, 0, 9), (2, 0, 9), (1, 2, 3)])
def test_rand_advance_equals_the_draws_the_checker_made(noisekeys):
    """The helper, chained over several frames with layers coming and going, lands where the checker's serial rand()
    actually stood after keying those frames."""
    w, h = 33, 5
    layers = [R.layer(color=0x203040, threshhold=90, noisekey=nk, xdivr=1 + l) for l, nk in enumerate(noisekeys)]
    flags = []
    for lay in layers:
        flags += R.layer_flags(lay)
    p = _capi.make_key_params(flags, width=w, height=h)
    nl = len(layers)
    rs = np.random.RandomState(len(noisekeys) * 7 + sum(noisekeys))
    pos_lib = pos_ref = 11                                                         # not from 0: positions are relative
    dst = np.zeros((h, w, 4), np.uint8)
    for t in range(5):
        present = [1] * nl if t == 0 else [int(x) for x in rs.randint(0, 2, size=nl)]
        srcs = [R.make_frame(w, h, 50 + t * 4 + l, key=0x203040) if present[l] else None for l in range(nl)]
        pos_ref = R.key_frame(dst, srcs, layers, pos_ref)
        pos_lib = _advance(p, pos_lib, present)
        assert pos_lib == pos_ref
    assert _advance(p, 0) == 3 * w * h * sum(1 for nk in noisekeys if nk > 0)      # NULL mask: every layer present


def test_checker_rand_is_the_library_stream():
    lib = L.product()
    for pos, n in ((0, 64), (1000, 40), (3 * 96 * 32, 31)):
        out = (C.c_uint32 * n)()
        lib.ntscsim_rng_draw(pos, n, out)
        assert list(out) == R.RAND.draws(pos, n).tolist()
    assert R.RAND.draws(0, 3).tolist() == [1804289383, 846930886, 1681692777]       # glibc's first three, unseeded


@pytest.mark.parametrize("w, h, pos", [(96, 32, 0), (100, 35, 3 * 100 * 35), (99, 33, 12345), (720, 486, 2 * 3 * 720 * 486 + 5)])
def test_lane_start_states_equal_the_serial_stream(w, h, pos):
    """The window every lane of k_key_draw starts from (per-lane polynomial applied to the layer's window, as the
    launcher computes it) is the serial generator's window 768 * lane draws further on."""
    lib = L.product()
    lanes = (w * h + 255) // 256
    picks = sorted(set([0, 1, 2, lanes // 2, lanes - 1]) & set(range(lanes)))
    if w * h <= 4096:
        picks = list(range(lanes))
    out = (C.c_uint32 * 31)()
    for lane in picks:
        assert lib.ntscsim_key_debug_lane_state(w, h, pos, lane, out) == _capi.OK
        assert list(out) == R.RAND.window(pos + 768 * lane), lane
    assert lib.ntscsim_key_debug_lane_state(w, h, pos, lanes, out) == _capi.E_ARG


# ---- the checker against the reference's own function ----------------------------------------------------------

def _case(name):
    w, h, delay, T, nl = (int(x) for x in GOLD["ck_%s_geom" % name])
    layers = [R.layer(**dict(zip(FIELDS, (int(v) for v in row)))) for row in GOLD["ck_%s_layers" % name]]
    return w, h, delay, T, nl, layers, GOLD["ck_%s_present" % name], GOLD["ck_%s_src" % name], GOLD["ck_%s_out" % name]


def test_fixture_set_is_complete():
    delays = {name: int(GOLD["ck_%s_geom" % name][2]) for name in CASES}
    noisy = {name: bool((GOLD["ck_%s_layers" % name][:, 5] > 0).any()) for name in CASES}
    frames = {name: int(GOLD["ck_%s_geom" % name][3]) for name in CASES}
    for d in (1, 2, 3):
        for nz in (False, True):
            assert any(delays[n] == d and noisy[n] == nz and frames[n] == 7 for n in CASES), (d, nz)
    assert any(frames[n] == 1 and noisy[n] for n in CASES) and any(frames[n] == 1 and not noisy[n] for n in CASES)
    assert any((GOLD["ck_%s_present" % n] == 0).any() for n in CASES)


@pytest.mark.parametrize("name", CASES)
def test_checker_equals_reference_fixture(name):
    w, h, delay, T, nl, layers, present, src, want = _case(name)
    ring = [np.zeros((h, w, 4), np.uint8) for _ in range(delay)]                  # :1013-1016
    frames = [[src[t, l] if present[t, l] else None for l in range(nl)] for t in range(T)]
    got, ri, pos = R.key_clip(ring, frames, layers)
    assert int((got != want).sum()) == 0
    assert ri == T % delay
    assert pos == sum(3 * w * h for t in range(T) for l in range(nl) if present[t, l] and layers[l]["noisekey"] > 0)
    # the pixel-by-pixel form of the checker gives the same frames
    ring = [np.zeros((h, w, 4), np.uint8) for _ in range(delay)]
    p2, idx = 0, 0
    for t in range(T):
        p2 = R.key_frame(ring[idx], frames[t], layers, p2, scalar=True)
        assert int((ring[idx] != want[t]).sum()) == 0, t
        idx = (idx + 1) % delay
    assert p2 == pos


def test_struct_layouts_match_ctypes(tmp_path):
    """The four structs of the key stage have the size and field offsets of their ctypes mirrors (strict C99)."""
    import shutil
    import subprocess
    assert shutil.which("gcc") is not None, "gcc is needed to check the struct layouts"
    structs = {"ntscsim_key_layer": _capi.KeyLayer, "ntscsim_key_params": _capi.KeyParams,
               "ntscsim_key_src": _capi.KeySrc, "ntscsim_key_desc": _capi.KeyDesc}
    lines = ['#include "ntscsim.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {"]
    for cname, mirror in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(L.ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, mirror in structs.items():
        assert int(out[cname]) == C.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert int(out["%s.%s" % (cname, fname)]) == getattr(mirror, fname).offset, (cname, fname)
    assert _capi.KEY_FAST_LAYERS == 4
