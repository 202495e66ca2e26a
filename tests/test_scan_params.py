"""Host half of the scanimate stage (csrc/scan_params.cpp: ntscsim_scan_params_init, _parse_argv, ntscsim_scan_effect,
ntscsim_scan_field_of).  No GPU.  The expected values are derived by hand from ffmpeg_scanimate.cpp: parse_argv()
:643-723, the presets :601-635, the source size :190-197, the effect numbering :865-867 and the field :1224."""
import ctypes as C

import pytest

import _libs as L  # noqa: F401  (puts the package on the path)
import _scan_ref as R
import ntscsim
from ntscsim import _capi


def code_of(flags, require_io=False):
    with pytest.raises(ntscsim.NtscsimError) as e:
        _capi.make_scan_params(flags, require_io=require_io)
    return e.value.code


def out_of(p):
    return (p.output_width, p.output_height, p.tv_standard, p.field_rate_num, p.field_rate_den, p.output_pal)


def test_defaults():
    p = _capi.make_scan_params([])
    assert p.struct_size == C.sizeof(_capi.ScanParams)
    assert out_of(p) == (720, 480, 0, 60000, 1001, 0)                              # preset_NTSC() :610-617
    assert (p.input_ntsc, p.use_422_colorspace, p.n_inputs) == (0, 0, 0)
    assert (p.src_width, p.src_height) == (600, 800)                               # :195-196
    assert not p.last_input_path and not p.output_path


@pytest.mark.parametrize("name, want", [("pal", (720, 576, 1, 50, 1, 1)), ("ntsc", (720, 480, 0, 60000, 1001, 0)),
                                        ("720p60", (1280, 720, 2, 60000, 1001, 0)), ("1080p60", (1920, 1080, 3, 60000, 1001, 0))])
def test_presets(name, want):
    assert out_of(_capi.make_scan_params(["-tvstd", name])) == want
    assert out_of(_capi.make_scan_params(["-tvstd", "pal", "--tvstd", name])) == want   # a later preset resets the PAL flag


def test_switches():
    p = _capi.make_scan_params(["-i", "a", "-422", "-i", "b", "-o", "out", "-inntsc"])
    assert (p.n_inputs, p.last_input_path, p.output_path) == (2, b"b", b"out")     # the last input is the one that shows
    assert (p.use_422_colorspace, p.input_ntsc) == (1, 1)
    assert _capi.make_scan_params(["-422", "-420"]).use_422_colorspace == 0
    assert _capi.make_scan_params(["---inntsc"]).input_ntsc == 1                   # any number of leading dashes :651
    assert code_of(["-h"]) == _capi.E_HELP and code_of(["--help"]) == _capi.E_HELP


def test_width():
    assert code_of(["-width", "31"]) == _capi.E_FLAG                               # :661
    p = _capi.make_scan_params(["-width", "32"])
    assert (p.output_width, p.output_height) == (32, 480)                          # the width only
    p = _capi.make_scan_params(["-tvstd", "pal", "-width", "0x100"])
    assert (p.output_width, p.output_height) == (256, 576)                         # strtoul base 0
    assert _capi.make_scan_params(["-width", "0100"]).output_width == 64
    assert _capi.make_scan_params(["-width", "640", "-tvstd", "ntsc"]).output_width == 720   # a later preset overrides it
    assert code_of(["-width", "-1"]) == _capi.E_FLAG                               # (int)0xFFFFFFFFFFFFFFFF = -1 < 32
    assert code_of(["-width", "4294967296"]) == _capi.E_FLAG                       # (int)2^32 = 0
    assert _capi.make_scan_params(["-width", "4294967396"]).output_width == 100    # (int)(2^32 + 100)
    assert code_of(["-width", "junk"]) == _capi.E_FLAG                             # strtoul gives 0


def test_missing_values_and_unknown_words():
    for sw in ("-width", "-i", "-o", "-tvstd"):                                    # `if (a == NULL) return 1`; -tvstd: see the header
        assert code_of([sw]) == _capi.E_FLAG, sw
    assert code_of(["-tvstd", "secam"]) == _capi.E_FLAG                            # "Unknown tv std" :697-700
    assert code_of(["-bogus"]) == _capi.E_FLAG                                     # "Unknown switch" :702-705
    assert code_of(["-d", "2"]) == _capi.E_FLAG                                    # the other tools' switches are not this one's
    assert code_of(["word"]) == _capi.E_FLAG                                       # "Unhandled arg" :707-710
    assert code_of(["-inntsc", "word"]) == _capi.E_FLAG


def test_require_io():
    assert code_of([], require_io=True) == _capi.E_FLAG
    assert code_of(["-i", "a"], require_io=True) == _capi.E_FLAG                   # "No output file" :713-716
    assert code_of(["-o", "b"], require_io=True) == _capi.E_FLAG                   # "No input files" :717-720
    assert code_of(["-i", "a", "-o", ""], require_io=True) == _capi.E_FLAG         # output_file.empty()
    p = _capi.make_scan_params(["-i", "a", "-o", "b"], require_io=True)
    assert (p.last_input_path, p.output_path) == (b"a", b"b")
    assert _capi.make_scan_params(["-o", "b"]).output_path == b"b"                 # not required: no check


def test_source_size_is_derived_behind_argv():
    """:190-197 runs when the inputs are opened: -inntsc before or after -tvstd pal gives the same size."""
    assert [(p.src_width, p.src_height) for p in (_capi.make_scan_params(["-inntsc"]),)] == [(480, 480)]
    for flags in (["-inntsc", "-tvstd", "pal"], ["-tvstd", "pal", "-inntsc"]):
        p = _capi.make_scan_params(flags)
        assert (p.src_width, p.src_height) == (480, 576), flags
    for flags in (["-tvstd", "pal", "-inntsc", "-tvstd", "720p60"], ["-inntsc", "-tvstd", "1080p60"]):
        p = _capi.make_scan_params(flags)
        assert (p.src_width, p.src_height) == (480, 480), flags                  # only preset_PAL sets output_pal
    assert [(p.src_width, p.src_height) for p in (_capi.make_scan_params(["-tvstd", "pal"]),)] == [(600, 800)]


@pytest.mark.parametrize("fieldno, effect, ef_field, field", [(0, 0, 0, 1), (179, 0, 179, 0), (180, 1, 0, 1), (719, 3, 179, 0),
                                                              (720, 0, 0, 1), ((1 << 32) + 5, 1, 81, 0)])
def test_effect_and_field(fieldno, effect, ef_field, field):
    lib = ntscsim.lib()
    e, f = C.c_uint32(99), C.c_uint32(99)
    lib.ntscsim_scan_effect(fieldno, C.byref(e), C.byref(f))
    assert (e.value, f.value) == (effect, ef_field) == R.effect_of(fieldno)
    assert lib.ntscsim_scan_field_of(fieldno) == field == R.field_of(fieldno)
    lib.ntscsim_scan_effect(fieldno, None, None)                                   # either pointer may be NULL


def test_effect_in_the_tools_types_behind_180_times_2_to_the_32():
    """effect is an unsigned int: the quotient is cut to 32 bits before it is multiplied back."""
    lib = ntscsim.lib()
    fieldno = 180 * (1 << 32) + 7
    e, f = C.c_uint32(), C.c_uint32()
    lib.ntscsim_scan_effect(fieldno, C.byref(e), C.byref(f))
    assert (e.value, f.value) == (0, 7 + ((180 << 32) & 0xFFFFFFFF)) == R.effect_of(fieldno)


def test_exports():
    lib = ntscsim.lib()
    for sym in _capi.EXPORTS:
        if sym.startswith("ntscsim_scan_"):
            getattr(lib, sym)
    assert sum(1 for s in _capi.EXPORTS if s.startswith("ntscsim_scan_")) == 12
