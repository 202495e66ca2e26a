"""ntscsim_mixed_field422_desc / ntscsim_mixed_fields422_device as a C program sees them, against ntscsim/_capi.py: the
struct's layout compiled from include/ntscsim.h (strict C99), the header still compiling as C++, the symbol exported, and
-- without a GPU -- the argument checks that need no device and the Python veneer's sets of ffmpeg_to_composite flags."""
import ctypes as C
import os
import shutil
import subprocess

import _libs as L
import ntscsim
from ntscsim import _capi


def test_struct_layout_matches_the_ctypes_mirror(tmp_path):
    assert shutil.which("gcc") is not None, "gcc is needed to read the header's layout"
    structs = {"ntscsim_mixed_field422_desc": _capi.MixedField422Desc, "ntscsim_field422_desc": _capi.Field422Desc}
    lines = ['#include "ntscsim.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {"]
    for cname, mirror in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    inc = os.path.join(L.ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe)])
    out = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, mirror in structs.items():
        assert int(out[cname]) == C.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert int(out["%s.%s" % (cname, fname)]) == getattr(mirror, fname).offset, (cname, fname)
    # the 422 descriptor is 9 pointers + 9 linesizes + 4 words + 2 x 64 bits = 140 -> 144 bytes; `set` follows it
    assert C.sizeof(_capi.Field422Desc) == 144
    assert C.sizeof(_capi.MixedField422Desc) == 152 and _capi.MixedField422Desc.set.offset == 144
    if shutil.which("g++"):
        cpp = tmp_path / "hdr.cpp"
        cpp.write_text('#include "ntscsim.h"\nint main() { ntscsim_mixed_field422_desc d; d.set = -1; return d.set + 1; }\n')
        subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(cpp)])


def test_symbol_is_exported_and_bound():
    assert "ntscsim_mixed_fields422_device" in _capi.EXPORTS
    fn = L.product().ntscsim_mixed_fields422_device
    assert fn.restype is C.c_int and len(fn.argtypes) == 8


def test_a_null_context_is_refused_without_a_gpu():
    """the argument checks that need no device: NULL ctx, then nothing else is looked at"""
    lib = L.product()
    d = (_capi.MixedField422Desc * 1)()
    assert lib.ntscsim_mixed_fields422_device(None, None, 0, d, 1, 96, 32, None) == _capi.E_ARG
    assert lib.ntscsim_mixed_fields422_device(None, None, 0, None, 0, 96, 32, None) == _capi.E_ARG


def test_flag_lists_are_accepted_as_sets():
    """ffmpeg_to_composite's switches, not ffmpeg_ntsc's: -bkey-feedback exists only there, and the 8-bit tool's defaults
    differ (vhs_out_sharpen_chroma)"""
    sets = ntscsim.FieldSimulator.build_sets422([L.make_params_tocomp(["-vhs"]), ["-vhs", "-vhs-speed", "ep"], [],
                                                 ["-bkey-feedback", "3"]])
    assert len(sets) == 4 and sets[0].emulating_vhs and sets[1].output_vhs_tape_speed == 2 and not sets[2].emulating_vhs
    assert sets[3].black_key_level_feedback == 3 and sets[2].black_key_level_feedback == -1
    assert all(s.vhs_out_sharpen_chroma == 0.85 for s in sets)
    assert all(s.struct_size == C.sizeof(_capi.Params) for s in sets)
    assert ntscsim.FieldSimulator.build_sets422([]) is None
