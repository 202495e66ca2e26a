"""csrc/cass_params.cpp: ffmpeg_cassette's switches and the settings derived from them, worked out by hand here from the
tool's text (parse_argv :441-590, :582, :338, LowpassFilter::setFilter :84-92, the set-up :864-880)."""
import ctypes as C
import math

import pytest

import _libs as L  # noqa: F401  (puts the package on the path)
from ntscsim import _capi
from ntscsim._capi import NtscsimError, make_cass_params


def alpha(hz, rate=44100):
    interval = 1.0 / rate
    tau = 1 / (hz * 2 * math.pi)
    return interval / (tau + interval)


def code(flags, **kw):
    try:
        make_cass_params(flags, **kw)
    except NtscsimError as e:
        return e.code
    return _capi.OK


def test_defaults():
    p = make_cass_params([])
    assert (p.channels, p.rate, p.passes, p.preemphasis, p.deemphasis, p.mono) == (2, 44100, 6, 0, 0, 0)
    assert (p.lowpass_hz, p.highpass_hz, p.emphasis_hz, p.head_tilt, p.head_tilt_waver, p.hiss_db) == (20000, 20, 4000, 0.2, 0.5, -45)
    assert p.hiss_level == int(math.pow(10.0, -45 / 20.0) * 5000) == 28
    assert p.taps == 8                                                           # floor(0.4 + 0.6 + 7.5)
    assert (p.alpha_lowpass, p.alpha_highpass) == (alpha(20000), alpha(20))
    assert p.alpha_pre == p.alpha_post == alpha(4000)
    assert (p.transcode_start, p.transcode_end, p.transcode_dur) == (0, -1, -1)  # :570 turns the initial -1 into 0
    init = _capi.CassParams()
    _capi.lib().ntscsim_cass_params_init(C.byref(init))
    assert (init.taps, init.hiss_level, init.struct_size) == (8, 28, C.sizeof(_capi.CassParams))


@pytest.mark.parametrize("k,want", [(0, (16000, 100, 0.55, 3.5, 25)), (1, (14000, 100, 0.6, 6, 37)), (2, (10000, 100, 0.5, 3, 22)),
                                    (3, (16000, 20, 0.75, 10, 57)), (4, (16000, 20, 0.25, 1.1, 13))])
def test_presets(k, want):
    p = make_cass_params(["-preset", k])
    assert (p.lowpass_hz, p.highpass_hz, p.head_tilt_waver, p.head_tilt, p.taps) == want
    assert (p.alpha_lowpass, p.alpha_highpass) == (alpha(want[0]), alpha(want[1]))


@pytest.mark.parametrize("tilt,taps", [(0, 7), (0.2, 8), (3.5, 25), (10, 57), (-3, 22), (100, 507)])
def test_taps(tilt, taps):
    p = make_cass_params([])
    p.head_tilt = tilt
    assert _capi.lib().ntscsim_cass_params_derive(C.byref(p)) == _capi.OK
    assert p.taps == taps == int(math.floor(abs(tilt * 2) + abs(tilt * 3) + 7.5))


def test_switches_and_their_order():
    p = make_cass_params(["-headalign", "7", "-preset", "2"])                   # the preset comes later: it wins
    assert (p.head_tilt, p.head_tilt_waver, p.lowpass_hz) == (3, 0.5, 10000)
    p = make_cass_params(["-preset", "2", "-headalign", "7", "-headalignwaver", "2", "-low", "9000", "-high", "0x32"])
    assert (p.head_tilt, p.head_tilt_waver, p.lowpass_hz, p.highpass_hz, p.taps) == (7, 2, 9000, 50, 42)
    p = make_cass_params(["-headalign", "2.9", "-headalignwaver", "0.9"])       # atoi: only the presets give fractions
    assert (p.head_tilt, p.head_tilt_waver, p.taps) == (2, 0, 17)
    p = make_cass_params(["-headalign", "-3"])
    assert (p.head_tilt, p.taps) == (-3, 22)
    p = make_cass_params(["--mono", "-preemphasis", "1", "-deemphasis", "2", "-preemphasis", "0"])   # any number of dashes; n > 0
    assert (p.mono, p.preemphasis, p.deemphasis) == (1, 0, 1)
    p = make_cass_params(["-audio-hiss", "0"])
    assert p.hiss_level == 5000
    p = make_cass_params(["-audio-hiss", "-200"])
    assert p.hiss_level == 0
    p = make_cass_params(["-low", "010"])                                       # strtoul with base 0: octal
    assert p.lowpass_hz == 8


def test_recorded_but_unused_switches():
    p = make_cass_params(["-i", "in.wav", "-o", "out.wav", "-a", "3", "-ss", "1.5", "-t", "2"], require_io=True)
    assert (p.input_path, p.output_path, p.audio_stream_index) == (b"in.wav", b"out.wav", 3)
    assert (p.transcode_start, p.transcode_dur, p.transcode_end) == (1.5, 2, 3.5)
    p = make_cass_params(["-an", "-ss", "1", "-se", "4"])
    assert (p.audio_stream_index, p.transcode_dur) == (-1, 3)
    q = make_cass_params([])
    for f in ("taps", "hiss_level", "alpha_lowpass", "alpha_highpass", "alpha_pre", "alpha_post", "mono"):
        assert getattr(p, f) == getattr(q, f)


def test_refusals():
    assert code(["-h"]) == code(["--help"]) == _capi.E_HELP
    assert code(["-nosuch"]) == _capi.E_FLAG
    assert code(["stray"]) == _capi.E_FLAG
    assert code(["-preset", "5"]) == code(["-preset", "-1"]) == _capi.E_FLAG
    assert code(["-headalign"]) == code(["-preset"]) == code(["-ss"]) == _capi.E_FLAG   # a switch without its value
    assert code(["-ss", "5", "-se", "4"]) == _capi.E_FLAG                       # "nothing to transcode"
    assert code([], require_io=True) == _capi.E_FLAG
    assert code(["-i", "x"], require_io=True) == _capi.E_FLAG


def test_zero_cutoff_and_tap_cap():
    # a cut-off of 0: HiLoComboPass::init() :198 returns without filters and the tool dies in its assert :335
    assert code(["-low", "0"]) == code(["-high", "0"]) == code(["-high", "junk"]) == _capi.E_ARG
    assert code(["-low", "-5"]) == _capi.E_PARAM                                # (int)strtoul wraps to -5: not run
    assert make_cass_params(["-headalign", "100"]).taps == 507
    assert make_cass_params(["-headalign", "-100"]).taps == 507
    assert make_cass_params(["-headalign", "100"]).taps <= _capi.CASS_MAX_TAPS == 512
    assert code(["-headalign", "101"]) == _capi.OK                              # 512 taps exactly
    assert make_cass_params(["-headalign", "101"]).taps == 512
    assert code(["-headalign", "102"]) == code(["-headalign", "-102"]) == code(["-headalign", "100000"]) == _capi.E_PARAM
    assert code(["-audio-hiss", "200"]) == _capi.E_PARAM                        # the level leaves int
