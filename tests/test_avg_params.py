"""Host half of the average_delay stage (csrc/avg_params.cpp: ntscsim_avg_params_*, _parse_argv).  No GPU.  The
expected values are derived by hand from ffmpeg_average_delay.cpp: parse_argv() :623-708, InputFile() :73,
new_input_file() :571-589, current_input_file() :562-569, the globals :44-68 and the presets :597-613."""
import ctypes as C

import pytest

import _libs as L  # noqa: F401  (puts the package on the path)
import ntscsim
from ntscsim import _capi


def levels_of(p):
    return [int(p.layers[l].newlevel) for l in range(p.n_layers)]


def code_of(flags, require_io=False):
    with pytest.raises(ntscsim.NtscsimError) as e:
        _capi.make_avg_params(flags, require_io=require_io)
    return e.value.code


def test_defaults():
    p = _capi.make_avg_params([])
    assert p.struct_size == C.sizeof(_capi.AvgParams)
    assert (p.width, p.height, p.tv_standard, p.delay, p.use_422_colorspace, p.n_layers) == (720, 480, 0, 1, 0, 0)   # :67, :606-613
    assert not p.output_path
    p = _capi.make_avg_params(["-i", "a"])
    assert levels_of(p) == [128] and p.layers[0].path == b"a"                      # InputFile() :73


def test_newlevel_is_inherited_by_the_next_input():
    """new_input_file() :571-589 copies the last input, newlevel included; reset_on_dup() :94-96 clears only the path."""
    p = _capi.make_avg_params(["-i", "a", "-n", "64", "-i", "b", "-i", "c", "-n", "200", "-i", "d"])
    assert levels_of(p) == [64, 64, 200, 200]
    assert [p.layers[l].path for l in range(4)] == [b"a", b"b", b"c", b"d"]
    many = []
    for k in range(40):                                                            # no limit on the layer count
        many += ["-i", "f%d" % k, "-n", str(k)]
    p = _capi.make_avg_params(many)
    assert levels_of(p) == list(range(40))


@pytest.mark.parametrize("text, want", [("-1", -1), ("0x100", 256), ("300", 300), ("0", 0), ("256", 256), ("010", 8),
                                        ("65536", 65536), ("1000", 1000), ("4294967295", -1), ("junk", 0)])
def test_newlevel_values(text, want):
    """(int)strtoul(a, NULL, 0) :655: base 0, a minus sign negates in unsigned long and the cast keeps the low 32 bits."""
    assert levels_of(_capi.make_avg_params(["-i", "a", "-n", text])) == [want]
    assert levels_of(_capi.make_avg_params(["-i", "a", "---n", text])) == [want]   # any number of leading dashes :631


def test_newlevel_before_the_first_input_is_the_tools_throw():
    assert code_of(["-n", "64"]) == _capi.E_ARG                                    # current_input_file() :562-569
    assert code_of(["-n", "64", "-i", "a"]) == _capi.E_ARG
    assert code_of(["-d", "2", "-n", "64"]) == _capi.E_ARG


def test_delay():
    assert code_of(["-d", "0"]) == _capi.E_FLAG                                    # "Invalid delay" :647-650
    assert code_of(["-d", "257"]) == _capi.E_FLAG
    assert code_of(["-d", "-1"]) == _capi.E_FLAG                                   # (unsigned int) of -1 is > 256
    assert _capi.make_avg_params(["-d", "256"]).delay == 256
    assert _capi.make_avg_params(["-d", "1"]).delay == 1
    assert _capi.make_avg_params(["-d", "0x10"]).delay == 16


def test_width():
    assert code_of(["-width", "31"]) == _capi.E_FLAG                               # :641
    assert code_of(["-width", "-5"]) == _capi.E_FLAG                               # (int) of it is negative
    p = _capi.make_avg_params(["-width", "32"])
    assert (p.width, p.height) == (32, 480)
    p = _capi.make_avg_params(["-i", "a"], width=96, height=32)
    assert (p.width, p.height) == (96, 32)


def test_tvstd_and_colourspace():
    p = _capi.make_avg_params(["-width", "960", "-tvstd", "pal"])                  # preset_PAL() :597-604 resets the width
    assert (p.tv_standard, p.width, p.height) == (1, 720, 576)
    p = _capi.make_avg_params(["-tvstd", "pal", "-tvstd", "ntsc"])
    assert (p.tv_standard, p.width, p.height) == (0, 720, 480)
    assert code_of(["-tvstd", "secam"]) == _capi.E_FLAG                            # "Unknown tv std" :682-685
    assert code_of(["-tvstd"]) == _capi.E_FLAG
    assert _capi.make_avg_params(["-422"]).use_422_colorspace == 1
    assert _capi.make_avg_params(["-422", "-420"]).use_422_colorspace == 0


def test_unknown_switch_bare_word_missing_value_and_help():
    assert code_of(["-bogus"]) == _capi.E_FLAG                                     # "Unknown switch" :687-690
    assert code_of(["-f", "8"]) == _capi.E_FLAG                                    # the keyer's switch is not this tool's
    assert code_of(["word"]) == _capi.E_FLAG                                       # "Unhandled arg" :692-695
    assert code_of(["-i", "a", "word"]) == _capi.E_FLAG
    for sw in ("-i", "-o", "-d", "-n", "-width"):                                  # `if (a == NULL) return 1`
        assert code_of(["-i", "a", sw] if sw == "-n" else [sw]) == _capi.E_FLAG
    for h in ("-h", "-help", "--help", "---h"):                                    # :633-636
        assert code_of([h]) == _capi.E_HELP
    assert code_of(["-i", "a", "-o", "b", "-h"], require_io=True) == _capi.E_HELP


def test_require_io():
    assert code_of(["-i", "a"], require_io=True) == _capi.E_FLAG                   # "No output file specified" :698-701
    assert code_of(["-o", "out"], require_io=True) == _capi.E_FLAG                 # "No input files specified" :702-705
    assert code_of(["-i", "a", "-o", ""], require_io=True) == _capi.E_FLAG         # output_file.empty()
    p = _capi.make_avg_params(["-i", "a", "-o", "out"], require_io=True)
    assert (p.output_path, p.n_layers) == (b"out", 1)
    p = _capi.make_avg_params(["-o", "out"])                                       # off: the library's callers bring frames, not files
    assert (p.output_path, p.n_layers) == (b"out", 0)
    assert _capi.make_avg_params([]).n_layers == 0


def test_add_layer_and_free():
    lib = _capi.lib()
    p = _capi.AvgParams()
    lib.ntscsim_avg_params_init(C.byref(p))
    assert lib.ntscsim_avg_params_add_layer(C.byref(p), b"a") == 0
    p.layers[0].newlevel = 7
    for k in range(1, 9):                                                          # grows past the first block of four
        assert lib.ntscsim_avg_params_add_layer(C.byref(p), None) == k
    assert levels_of(p) == [7] * 9 and p.layers[8].path is None
    lib.ntscsim_avg_params_free(C.byref(p))
    assert (p.n_layers, p.layers_cap) == (0, 0) and not p.layers
    bad = _capi.AvgParams()
    assert lib.ntscsim_avg_params_add_layer(C.byref(bad), b"a") == _capi.E_ARG      # struct_size not set
    assert lib.ntscsim_avg_parse_argv(C.byref(bad), 0, None, 0) == _capi.E_ARG
