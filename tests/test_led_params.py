"""Host half of the vhsled stage (csrc/led_params.cpp: ntscsim_led_params_init, _parse_argv).  No GPU.  The expected
values are derived by hand from ffmpeg_vhsled.cpp: the globals :44-52, preset_NTSC() :457-460 and parse_argv()
:476-584."""
import ctypes as C

import pytest

import _libs as L  # noqa: F401  (puts the package on the path)
import ntscsim
from ntscsim import _capi


def code_of(flags, require_io=False):
    with pytest.raises(ntscsim.NtscsimError) as e:
        _capi.make_led_params(flags, require_io=require_io)
    return e.value.code


def rate_of(flags):
    p = _capi.make_led_params(flags)
    return (p.field_rate_num, p.field_rate_den)


def test_defaults():
    p = _capi.make_led_params([])
    assert p.struct_size == C.sizeof(_capi.LedParams) == 56
    assert (p.width, p.height) == (-1, -1)                                          # :50-51
    assert (p.field_rate_num, p.field_rate_den) == (60000, 1001)                   # preset_NTSC()
    assert p.gamma_correction == -1 and p.underscan == 0 and p.use_422_colorspace == 0
    assert not p.input_path and not p.output_path
    assert "ntscsim_led_bind" in _capi.EXPORTS and "ntscsim_led_frames_device" in _capi.EXPORTS


def test_switches():
    p = _capi.make_led_params(["-i", "a", "-422", "-i", "b", "-o", "out", "-width", "720", "-height", "486"])
    assert (p.input_path, p.output_path) == (b"b", b"out")                         # one input: the last -i
    assert (p.width, p.height, p.use_422_colorspace) == (720, 486, 1)
    assert _capi.make_led_params(["-422", "-420"]).use_422_colorspace == 0
    assert _capi.make_led_params(["---422"]).use_422_colorspace == 1               # any number of leading dashes :484
    assert _capi.make_led_params(["--width", "64"]).width == 64
    assert code_of(["-h"]) == _capi.E_HELP and code_of(["--help"]) == _capi.E_HELP
    assert code_of(["-i", "a", "-h", "-bogus"]) == _capi.E_HELP                    # in argv order


def test_sizes_go_through_strtoul_base_0_and_the_cast():
    for sw, field in (("-width", "width"), ("-height", "height")):
        assert getattr(_capi.make_led_params([sw, "0x40"]), field) == 64
        assert getattr(_capi.make_led_params([sw, "0100"]), field) == 64
        assert getattr(_capi.make_led_params([sw, "32"]), field) == 32
        assert code_of([sw, "31"]) == _capi.E_FLAG                                 # :494 / :500
        assert code_of([sw, "0"]) == _capi.E_FLAG
        assert code_of([sw, "-1"]) == _capi.E_FLAG                                 # (int)0xFFFFFFFFFFFFFFFF = -1 < 32
        assert code_of([sw, "4294967296"]) == _capi.E_FLAG                         # (int)2^32 = 0
        assert getattr(_capi.make_led_params([sw, "4294967396"]), field) == 100    # (int)(2^32 + 100)
        assert code_of([sw, "junk"]) == _capi.E_FLAG                               # strtoul gives 0
    p = _capi.make_led_params(["-width", "100"])
    assert (p.width, p.height) == (100, -1)                                        # each switch sets its own field only
    assert _capi.make_led_params(["-width", "5000"]).width == 5000                 # the parser has no upper bound; bind has


def test_gamma_forms():
    assert _capi.make_led_params(["-gamma", "1.8"]).gamma_correction == 1.8
    assert _capi.make_led_params(["-gamma", "2"]).gamma_correction == 2.0
    assert _capi.make_led_params(["-gamma", "vga"]).gamma_correction == 2.2
    assert _capi.make_led_params(["-gamma", "ntsc"]).gamma_correction == 2.2
    assert _capi.make_led_params(["-gamma", "pal"]).gamma_correction == -1         # any other word leaves the value alone
    assert _capi.make_led_params(["-gamma", "1.5", "-gamma", "none"]).gamma_correction == 1.5
    assert _capi.make_led_params(["-gamma", "-3"]).gamma_correction == -1          # '-' is not a digit :506
    assert _capi.make_led_params(["-gamma", ".5"]).gamma_correction == -1          # nor is '.'
    assert _capi.make_led_params(["-gamma", "3x"]).gamma_correction == 3.0         # atof reads what it can


def test_underscan_is_clamped():
    for text, want in (("0", 0), ("5", 5), ("99", 99), ("100", 99), ("1000", 99), ("-4", 0), ("junk", 0), ("7.9", 7)):
        assert _capi.make_led_params(["-underscan", text]).underscan == want, text


def test_output_rate_forms():
    assert rate_of(["-or", "30"]) == (300000, 10000)                               # no denominator: n * 10000 / 10000
    assert rate_of(["-or", "29.97"]) == (299700, 10000)                            # strtof(29.97) * 10000 rounds to it
    assert rate_of(["-or", "60000/1001"]) == (60000, 1001)
    assert rate_of(["-or", "60000:1001"]) == (60000, 1001)
    assert rate_of(["-or", "60000\\1001"]) == (60000, 1001)
    assert rate_of(["-or", "24/1"]) == (240000, 10000)                             # d = 1 takes the other branch :540
    assert rate_of(["-or", "30/0"]) == (300000, 10000)                             # d < 1 becomes 1
    assert rate_of(["-or", "25/junk"]) == (250000, 10000)
    assert rate_of(["-or", "59.6/2"]) == (60, 2)                                   # floor(n + 0.5)
    # the 5 per second floor
    assert rate_of(["-or", "4.99"]) == (50000, 10000)
    assert rate_of(["-or", "5"]) == (50000, 10000)
    assert rate_of(["-or", "9/2"]) == (50000, 10000)                               # 4.5 < 5: n = 5, d = 1
    assert rate_of(["-or", "10/2"]) == (10, 2)
    assert rate_of(["-or", "-30"]) == (50000, 10000)                               # negative: 0, then the floor
    assert rate_of(["-or", "junk"]) == (50000, 10000)


def test_refusals():
    assert code_of(["-bogus"]) == _capi.E_FLAG                                     # unknown switch :563-566
    assert code_of(["-fa", "2"]) == _capi.E_FLAG                                   # in the help text, not in the parser
    assert code_of(["-fa"]) == _capi.E_FLAG
    assert code_of(["-tvstd", "pal"]) == _capi.E_FLAG                              # the other tools' switch, not this one's
    assert code_of(["stray"]) == _capi.E_FLAG                                      # bare argument :568-571
    assert code_of(["-422", "stray"]) == _capi.E_FLAG
    for sw in ("-i", "-o", "-or", "-width", "-height", "-gamma", "-underscan"):
        assert code_of([sw]) == _capi.E_FLAG, sw                                   # missing value
        assert code_of(["-422", sw]) == _capi.E_FLAG, sw


def test_require_io():
    assert code_of([], require_io=True) == _capi.E_FLAG
    assert code_of(["-i", "a"], require_io=True) == _capi.E_FLAG                   # "No output file specified"
    assert code_of(["-o", "b"], require_io=True) == _capi.E_FLAG                   # "No input files specified"
    assert code_of(["-i", "", "-o", "b"], require_io=True) == _capi.E_FLAG         # empty() :578
    p = _capi.make_led_params(["-o", "b", "-i", "a"], require_io=True)
    assert (p.input_path, p.output_path) == (b"a", b"b")
    assert code_of(["-o", "b", "-i", "a", "-bogus"], require_io=True) == _capi.E_FLAG


def test_null_and_size_guards():
    lib = ntscsim.lib()
    p = _capi.LedParams()
    lib.ntscsim_led_params_init(C.byref(p))
    assert lib.ntscsim_led_parse_argv(None, 0, None, 0) == _capi.E_ARG
    assert lib.ntscsim_led_parse_argv(C.byref(p), 2, None, 0) == _capi.E_ARG
    p.struct_size = 8
    assert lib.ntscsim_led_parse_argv(C.byref(p), 0, None, 0) == _capi.E_ARG
    assert lib.ntscsim_led_bind(None, C.byref(p)) == _capi.E_ARG
