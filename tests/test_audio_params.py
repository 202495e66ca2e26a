"""ntscsim_audio_params_from_cli(): the settings composite_audio_process() reads, for the switch orders that matter,
against values written out by hand from the reference's text (parse_argv :1051-1203, the derivation :1229-1267, the
set-up :2031-2067, the line constants :903-907)."""
import ctypes as C
import math

import pytest

import _libs as L  # noqa: F401
from ntscsim import _capi

LEVEL_70 = 1        # (int)(10^(-70/20) * 5000) = (int)1.58
LEVEL_72 = 1        # (int)(10^(-72/20) * 5000) = (int)1.25
LEVEL_42 = 39       # (int)(10^(-42/20) * 5000) = (int)39.7

# switches: (channels, hifi, pre, de, hiss_level, lowpass, highpass, emphasis_hz)
ORDERS = {
    (): (2, 1, 1, 1, LEVEL_72, 20000, 20, 16000),
    ("-vhs",): (2, 1, 0, 0, LEVEL_70, 20000, 20, 16000),                        # -vhs clears the emphasis :1144
    ("-vhs", "-vhs-hifi", "0"): (1, 0, 0, 0, LEVEL_42, 10000, 100, 8000),
    ("-vhs-hifi", "0", "-vhs"): (1, 0, 0, 0, LEVEL_70, 10000, 100, 8000),       # -vhs afterwards overwrites the hiss :1146
    ("-vhs-hifi", "0"): (1, 0, 1, 1, LEVEL_42, 10000, 100, 8000),               # implies -vhs, leaves the emphasis on
    ("-vhs-hifi", "1"): (2, 1, 1, 1, LEVEL_70, 20000, 20, 16000),
    ("-vhs", "-vhs-hifi", "1"): (2, 1, 1, 1, LEVEL_70, 20000, 20, 16000),       # Hi-Fi turns the emphasis back on :1196
    ("-vhs", "-preemphasis", "1"): (2, 1, 1, 0, LEVEL_70, 20000, 20, 16000),
    ("-preemphasis", "1", "-vhs"): (2, 1, 0, 0, LEVEL_70, 20000, 20, 16000),
    ("-vhs-speed", "ep", "-vhs-hifi", "0"): (1, 0, 1, 1, LEVEL_42, 4000, 100, 8000),
    ("-vhs-hifi", "0", "-vhs-speed", "lp"): (1, 0, 1, 1, LEVEL_42, 7000, 100, 8000),
    ("-vhs-speed", "ep"): (2, 1, 1, 1, LEVEL_72, 20000, 20, 16000),             # Hi-Fi ignores the tape speed
    ("-audio-hiss", "0"): (2, 1, 1, 1, 5000, 20000, 20, 16000),
    ("-audio-hiss", "-200"): (2, 1, 1, 1, 0, 20000, 20, 16000),
}


def alpha(hz):
    interval = 1.0 / 44100
    tau = 1 / (hz * 2 * math.pi)
    return interval / (tau + interval)


@pytest.mark.parametrize("tool", ["ntsc", "to_composite"])
@pytest.mark.parametrize("flags", sorted(ORDERS), ids=lambda f: " ".join(f) or "default")
def test_derived_settings(flags, tool):
    ap, _ = _capi.make_audio_params(list(flags), tool)
    want = ORDERS[flags]
    got = (ap.channels, ap.hifi, ap.preemphasis, ap.deemphasis, ap.hiss_level, ap.lowpass_hz, ap.highpass_hz, ap.emphasis_hz)
    assert got == want
    assert ap.struct_size == C.sizeof(_capi.AudioParams) and ap.enabled == 1
    assert (ap.rate, ap.passes, ap.boost_hz, ap.boost_gain) == (44100, 6, 10000, 0.25)
    assert ap.buzz == math.pow(10.0, -42 / 20.0)
    assert (ap.hsync_hz, ap.vsync_lines, ap.vpulse_end) == (15734, 525, 10)
    assert ap.hpulse_end == 15734 * (4.7 / 1000000)
    assert ap.alpha_lowpass == alpha(want[5]) and ap.alpha_highpass == alpha(want[6])
    assert ap.alpha_pre == alpha(want[7]) == ap.alpha_post and ap.alpha_boost == alpha(10000)


def test_pal_nocomp_buzz_and_boost_switches():
    ap, _ = _capi.make_audio_params(["-tvstd", "pal", "-vhs-linear-video-crosstalk", "-30", "-vhs-linear-high-boost", "0.5"])
    assert (ap.hsync_hz, ap.vsync_lines, ap.vpulse_end, ap.tv_standard) == (15625, 625, 12, 1)
    assert ap.hpulse_end == 15625 * (4.0 / 1000000)
    assert ap.buzz == math.pow(10.0, -30 / 20.0) and ap.boost_gain == 0.5
    ap, _ = _capi.make_audio_params(["-vhs", "-nocomp"])
    assert ap.enabled == 0 and ap.channels == 2


def test_bad_arguments():
    lib = _capi.lib()
    p, cli, ap = _capi.Params(), _capi.Cli(), _capi.AudioParams()
    lib.ntscsim_params_init(C.byref(p))
    lib.ntscsim_cli_init(C.byref(cli))
    assert lib.ntscsim_audio_params_from_cli(None, C.byref(p), C.byref(cli)) == _capi.E_ARG
    assert lib.ntscsim_audio_params_from_cli(C.byref(ap), None, C.byref(cli)) == _capi.E_ARG
    assert lib.ntscsim_audio_params_from_cli(C.byref(ap), C.byref(p), None) == _capi.E_ARG
    p.struct_size = 4
    assert lib.ntscsim_audio_params_from_cli(C.byref(ap), C.byref(p), C.byref(cli)) == _capi.E_ARG
