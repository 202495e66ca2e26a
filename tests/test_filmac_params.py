"""Host half of the filmac stage: ntscsim_filmac_params_init / _parse_argv.  filmac.cpp's globals :40-56 and parse_argv()
:476-584 are ffmpeg_vhsled.cpp's text for text, so the two stages share one parser body (csrc/led_params.cpp) and must
give the same results on the same argument lists; what differs is that filmac acts on -gamma.  No GPU."""
import ctypes as C

import pytest

import _libs as L  # noqa: F401  (puts the package on the path)
import ntscsim
from ntscsim import _capi

FIELDS = ("struct_size", "width", "height", "underscan", "use_422_colorspace", "field_rate_num", "field_rate_den",
          "gamma_correction", "input_path", "output_path")

ARGV = [
    [], ["-i", "a", "-422", "-i", "b", "-o", "out", "-width", "720", "-height", "486"], ["-422", "-420"], ["---422"],
    ["--width", "64"], ["-h"], ["--help"], ["-i", "a", "-h", "-bogus"], ["-width", "0x40"], ["-height", "0100"],
    ["-width", "31"], ["-height", "31"], ["-width", "-1"], ["-width", "4294967396"], ["-width", "junk"], ["-width", "5000"],
    ["-gamma", "1.8"], ["-gamma", "2"], ["-gamma", "vga"], ["-gamma", "ntsc"], ["-gamma", "pal"], ["-gamma", "-3"],
    ["-gamma", ".5"], ["-gamma", "3x"], ["-gamma", "1.5", "-gamma", "none"], ["-gamma", "0.9"], ["-gamma", "1"],
    ["-underscan", "5"], ["-underscan", "1000"], ["-underscan", "-4"], ["-underscan", "7.9"],
    ["-or", "30"], ["-or", "29.97"], ["-or", "60000/1001"], ["-or", "60000:1001"], ["-or", "60000\\1001"], ["-or", "24/1"],
    ["-or", "30/0"], ["-or", "59.6/2"], ["-or", "4.99"], ["-or", "9/2"], ["-or", "-30"], ["-or", "junk"],
    ["-bogus"], ["-fa", "2"], ["-tvstd", "pal"], ["stray"], ["-422", "stray"],
    ["-i"], ["-o"], ["-or"], ["-width"], ["-height"], ["-gamma"], ["-underscan"], ["-422", "-gamma"],
]


def outcome(make, flags, require_io):
    try:
        p = make(flags, require_io=require_io)
    except ntscsim.NtscsimError as e:
        return ("error", e.code)
    return tuple(getattr(p, f) for f in FIELDS)


@pytest.mark.parametrize("require_io", [False, True])
def test_same_results_as_the_vhsled_parser(require_io):
    io = [[], ["-i", "a"], ["-o", "b"], ["-o", "b", "-i", "a"], ["-i", "", "-o", "b"]]
    n = 0
    for flags in ARGV:
        for tail in (io if require_io else [[]]):
            got = outcome(_capi.make_filmac_params, flags + tail, require_io)
            assert got == outcome(_capi.make_led_params, flags + tail, require_io), flags + tail
            n += got[0] != "error"
    assert n > 10                                                                  # and not by refusing everything


def test_defaults_and_layout():
    p = _capi.make_filmac_params([])
    assert p.struct_size == C.sizeof(_capi.FilmacParams) == 56
    assert (p.width, p.height) == (-1, -1) and (p.field_rate_num, p.field_rate_den) == (60000, 1001)
    assert p.gamma_correction == -1 and p.underscan == 0 and p.use_422_colorspace == 0
    assert C.sizeof(_capi.FilmacDesc) == 32 and C.sizeof(_capi.FilmacState) == 24
    for name in ("params_init", "parse_argv", "bind", "frames_device", "frames_host", "reset", "get_state", "set_state", "debug_levels"):
        assert "ntscsim_filmac_" + name in _capi.EXPORTS


def test_gamma_is_honoured():
    """-gamma ntsc / vga / a number above 1 switch the stage to linear light (:859); 1, a value below it and a word the
    parser does not know leave it off.  Seen from the host through what the parser records -- the device side of the
    same switch is tests/test_filmac_gpu.py."""
    for flags, want in ((["-gamma", "ntsc"], 2.2), (["-gamma", "vga"], 2.2), (["-gamma", "1.8"], 1.8), (["-gamma", "1"], 1.0),
                        (["-gamma", "0.5"], 0.5), (["-gamma", "pal"], -1.0), ([], -1.0)):
        assert _capi.make_filmac_params(flags).gamma_correction == want, flags


def test_null_and_size_guards():
    lib = ntscsim.lib()
    p = _capi.FilmacParams()
    lib.ntscsim_filmac_params_init(C.byref(p))
    assert lib.ntscsim_filmac_parse_argv(None, 0, None, 0) == _capi.E_ARG
    assert lib.ntscsim_filmac_parse_argv(C.byref(p), 2, None, 0) == _capi.E_ARG
    assert lib.ntscsim_filmac_bind(None, C.byref(p)) == _capi.E_ARG
    assert lib.ntscsim_filmac_reset(None) == _capi.E_ARG
    assert lib.ntscsim_filmac_get_state(None, None) == _capi.E_ARG
    assert lib.ntscsim_filmac_set_state(None, None) == _capi.E_ARG
    assert lib.ntscsim_filmac_debug_levels(None, 0, None) == _capi.E_ARG
    p.struct_size = 8
    assert lib.ntscsim_filmac_parse_argv(C.byref(p), 0, None, 0) == _capi.E_ARG
