"""Host half of the posterize and colormap stages: ntscsim_pixmap_params_init / _parse_argv and the two stages' names
for them, by hand against the tools' text (ffmpeg_posterize.cpp:604-611 and :620-696; ffmpeg_colormap.cpp:622-693 is the
same function without -threshhold), and the struct layouts against the ctypes mirrors.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import _libs as L
import ntscsim
from ntscsim import _capi

STAGES = ("post", "cmap")


def parse(stage, flags, require_io=False):
    try:
        return _capi.make_pixmap_params(stage, flags, require_io=require_io)
    except ntscsim.NtscsimError as e:
        return e.code


def layers(p):
    return [(p.layers[i].path, p.layers[i].threshhold) for i in range(p.n_layers)]


@pytest.mark.parametrize("stage", STAGES)
def test_defaults_after_preset_ntsc(stage):
    p = parse(stage, [])
    assert p.struct_size == C.sizeof(_capi.PixmapParams) == 56
    assert (p.width, p.height, p.field_rate_num, p.field_rate_den, p.output_pal) == (720, 480, 60000, 1001, 0)
    assert p.use_422_colorspace == 0 and p.n_layers == 0 and not p.layers and p.output_path is None


@pytest.mark.parametrize("stage", STAGES)
def test_tvstd_width_and_colorspace(stage):
    p = parse(stage, ["-tvstd", "pal"])
    assert (p.width, p.height, p.field_rate_num, p.field_rate_den, p.output_pal) == (720, 576, 50, 1, 1)
    p = parse(stage, ["-tvstd", "pal", "--tvstd", "ntsc"])
    assert (p.width, p.height, p.field_rate_num, p.field_rate_den, p.output_pal) == (720, 480, 60000, 1001, 0)
    assert parse(stage, ["-width", "64", "-tvstd", "pal"]).width == 720         # the preset sets the width again
    assert parse(stage, ["-tvstd", "secam"]) == _capi.E_FLAG
    assert parse(stage, ["-tvstd"]) == _capi.E_FLAG                              # the tool hands the NULL to strcmp
    assert parse(stage, ["-width", "31"]) == _capi.E_FLAG
    assert parse(stage, ["-width", "32"]).width == 32
    assert parse(stage, ["-width", "0x40"]).width == 64
    assert parse(stage, ["-width", "0100"]).width == 64
    assert parse(stage, ["-width", "-1"]) == _capi.E_FLAG                        # (int)strtoul("-1") = -1 < 32
    assert parse(stage, ["-width", "junk"]) == _capi.E_FLAG
    assert parse(stage, ["-width"]) == _capi.E_FLAG
    assert parse(stage, ["-422"]).use_422_colorspace == 1
    assert parse(stage, ["-422", "---420"]).use_422_colorspace == 0
    assert parse(stage, ["-height", "480"]) == _capi.E_FLAG                      # the tools have no -height


def test_threshhold_belongs_to_the_current_input():
    p = parse("post", ["-i", "a"])
    assert layers(p) == [(b"a", 3)]                                              # InputFile() :71
    p = parse("post", ["-i", "a", "-threshhold", "5", "-i", "b", "-i", "c", "-threshhold", "0x2", "-i", "d"])
    assert layers(p) == [(b"a", 5), (b"b", 5), (b"c", 2), (b"d", 2)]             # new_input_file() copies the one before
    p = parse("post", ["-i", "a", "-threshhold", "1", "-threshhold", "8"])
    assert layers(p) == [(b"a", 8)]
    assert parse("post", ["-threshhold", "5", "-i", "a"]) == _capi.E_FLAG        # current_input_file() throws
    assert parse("post", ["-threshhold", "5"]) == _capi.E_FLAG
    assert parse("post", ["-i", "a", "-threshhold"]) == _capi.E_FLAG
    p = parse("post", ["-i", "a", "-i", "b", "-i", "c", "-i", "d", "-i", "e", "-threshhold", "7"])   # the list grows
    assert layers(p) == [(b"a", 3), (b"b", 3), (b"c", 3), (b"d", 3), (b"e", 7)]


def test_threshhold_out_of_range_parses_and_is_refused_at_bind():
    """The parser records what the tool records; the tool's shift count is then undefined, so bind refuses it.  The
    parameters are checked before the ctx is looked at, which a host without a device can use."""
    lib = ntscsim.lib()
    for text, value in (("9", 9), ("-1", -1), ("100", 100), ("junk", 0)):
        p = parse("post", ["-i", "a", "-threshhold", text])
        assert layers(p) == [(b"a", value)]
        want = _capi.E_ARG if 0 <= value <= 8 else _capi.E_PARAM                 # E_ARG: only the ctx is missing
        assert lib.ntscsim_post_bind(None, C.byref(p)) == want, text
    p = parse("post", ["-i", "a", "-threshhold", "9", "-i", "b", "-threshhold", "8"])
    assert lib.ntscsim_post_bind(None, C.byref(p)) == _capi.E_PARAM              # every input is looked at
    for t in range(9):
        p = parse("post", ["-i", "a", "-threshhold", str(t)])
        assert lib.ntscsim_post_bind(None, C.byref(p)) == _capi.E_ARG
    for stage in STAGES:
        bind = getattr(lib, "ntscsim_%s_bind" % stage)
        for wh in ((0, 1), (1, 0), (16385, 1), (1, 16385), (-1, -1)):
            p = _capi.make_pixmap_params(stage, ["-i", "a"], width=wh[0], height=wh[1])
            assert bind(None, C.byref(p)) == _capi.E_SIZE, wh
        p = _capi.make_pixmap_params(stage, ["-i", "a"], width=16384, height=1)
        assert bind(None, C.byref(p)) == _capi.E_ARG


def test_colormap_has_no_threshhold():
    assert parse("cmap", ["-i", "a", "-threshhold", "5"]) == _capi.E_FLAG
    assert parse("cmap", ["-threshhold", "5"]) == _capi.E_FLAG
    assert layers(parse("cmap", ["-i", "a", "-i", "b"])) == [(b"a", 3), (b"b", 3)]
    lib = ntscsim.lib()
    p = _capi.PixmapParams()
    lib.ntscsim_pixmap_params_init(C.byref(p))
    argv = (C.c_char_p * 5)(b"x", b"-i", b"a", b"-threshhold", b"6")
    assert lib.ntscsim_pixmap_parse_argv(C.byref(p), 5, argv, 0, 0) == _capi.E_FLAG
    lib.ntscsim_pixmap_params_free(C.byref(p))
    lib.ntscsim_pixmap_params_init(C.byref(p))
    assert lib.ntscsim_pixmap_parse_argv(C.byref(p), 5, argv, 0, 1) == _capi.OK and p.layers[0].threshhold == 6


@pytest.mark.parametrize("stage", STAGES)
def test_require_io_help_unknown_switch_and_bare_word(stage):
    assert parse(stage, [], require_io=True) == _capi.E_FLAG
    assert parse(stage, ["-i", "a"], require_io=True) == _capi.E_FLAG            # "No output file specified"
    assert parse(stage, ["-o", "b"], require_io=True) == _capi.E_FLAG            # "No input files specified"
    assert parse(stage, ["-o", "", "-i", "a"], require_io=True) == _capi.E_FLAG  # output_file.empty()
    p = parse(stage, ["-o", "b", "-i", "a"], require_io=True)
    assert p.output_path == b"b" and layers(p) == [(b"a", 3)]
    assert parse(stage, ["-o", "b", "-o", "c"]).output_path == b"c"
    assert parse(stage, ["-h"]) == _capi.E_HELP and parse(stage, ["--help"]) == _capi.E_HELP
    assert parse(stage, ["-i", "a", "-h", "-bogus"]) == _capi.E_HELP             # in order: -h ends the parse
    assert parse(stage, ["-bogus"]) == _capi.E_FLAG
    assert parse(stage, ["-d", "2"]) == _capi.E_FLAG                             # average_delay's, not these tools'
    assert parse(stage, ["stray"]) == _capi.E_FLAG
    assert parse(stage, ["-422", "stray"]) == _capi.E_FLAG
    assert parse(stage, ["-i"]) == _capi.E_FLAG and parse(stage, ["-o"]) == _capi.E_FLAG


def test_null_and_size_guards():
    lib = ntscsim.lib()
    p = _capi.PixmapParams()
    lib.ntscsim_pixmap_params_init(C.byref(p))
    assert lib.ntscsim_pixmap_parse_argv(None, 0, None, 0, 1) == _capi.E_ARG
    assert lib.ntscsim_pixmap_parse_argv(C.byref(p), 2, None, 0, 1) == _capi.E_ARG
    for stage in STAGES:
        assert getattr(lib, "ntscsim_%s_parse_argv" % stage)(None, 0, None, 0) == _capi.E_ARG
        assert getattr(lib, "ntscsim_%s_bind" % stage)(None, None) == _capi.E_ARG
        assert getattr(lib, "ntscsim_%s_frames_device" % stage)(None, None, 0, None) == _capi.E_ARG
        assert getattr(lib, "ntscsim_%s_frames_host" % stage)(None, None, 0) == _capi.E_ARG
    assert lib.ntscsim_cmap_reset(None) == _capi.E_ARG
    assert lib.ntscsim_cmap_get_table(None, None) == _capi.E_ARG
    assert lib.ntscsim_cmap_set_table(None, None) == _capi.E_ARG
    p.struct_size = 8
    assert lib.ntscsim_pixmap_parse_argv(C.byref(p), 0, None, 0, 1) == _capi.E_ARG
    assert lib.ntscsim_post_bind(None, C.byref(p)) == _capi.E_ARG
    lib.ntscsim_pixmap_params_free(C.byref(p))                                   # not this struct: left alone
    lib.ntscsim_pixmap_params_free(None)


def test_struct_layouts_equal_the_ctypes_mirrors(tmp_path):
    """sizeof and every offsetof of the new structs, from a C99 program that includes the header."""
    assert shutil.which("gcc") is not None, "gcc is needed to read the layouts of include/ntscsim.h"
    structs = {"ntscsim_pixmap_layer": _capi.PixmapLayer, "ntscsim_pixmap_params": _capi.PixmapParams,
               "ntscsim_post_params": _capi.PostParams, "ntscsim_cmap_params": _capi.CmapParams,
               "ntscsim_post_desc": _capi.PostDesc, "ntscsim_cmap_desc": _capi.CmapDesc}
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
    assert C.sizeof(_capi.PostDesc) == 32 and C.sizeof(_capi.CmapDesc) == 48
    for stage in STAGES:
        for name in ("params_init", "params_free", "parse_argv", "bind", "frames_device", "frames_host"):
            assert "ntscsim_%s_%s" % (stage, name) in _capi.EXPORTS
