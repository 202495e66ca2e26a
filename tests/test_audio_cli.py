"""vhsaudio_cli's host fallback (--host: csrc/audio_chain.hpp run serially, no GPU touched): the byte stream equals the
checker's, a pipe fed in pieces equals a file, --block leaves the bytes unchanged, the sibling tool's parser is taken
with --tool to_composite."""
import os
import subprocess

import numpy as np
import pytest

import _audio_ref as A
import _libs as L
from ntscsim import _capi

EXE = os.path.join(L.PKG, "vhsaudio_cli")
FLAGS = ["-vhs", "-vhs-hifi", "0", "-vhs-speed", "lp"]


def run(args, data=None):
    r = subprocess.run([EXE, "--host"] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    return r


@pytest.mark.parametrize("tool", ["ntsc", "to_composite"])
def test_bytes_equal_the_checker(tmp_path, tool):
    ap, _ = _capi.make_audio_params(FLAGS, tool)
    a = A.make_input("music", 3001, ap.channels, 3)
    want, _state, pos = A.run_checker(ap, a, rng_pos=123)
    inp, out = tmp_path / "in.s16", tmp_path / "out.s16"
    a.tofile(str(inp))
    r = run(["--tool", tool, "--rng-pos", "123"] + FLAGS + ["-i", str(inp), "-o", str(out)])
    got = np.fromfile(str(out), np.int16).reshape(a.shape)
    assert (got == want).all()
    assert ("rand() position %d" % pos) in r.stderr.decode()


def test_pipe_in_pieces_and_blocks(tmp_path):
    ap, _ = _capi.make_audio_params([])
    a = A.make_input("music", 40000, 2, 4)                                      # 160,000 bytes: more than one pipe buffer
    want, _state, _pos = A.run_checker(ap, a)
    inp, out = tmp_path / "in.s16", tmp_path / "out.s16"
    a.tofile(str(inp))
    run(["-i", str(inp), "-o", str(out)])
    assert (np.fromfile(str(out), np.int16).reshape(a.shape) == want).all()
    # through pipes, written in pieces that cut sample frames
    p = subprocess.Popen([EXE, "--host", "-i", "-", "-o", "-"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    raw = a.tobytes()
    import threading
    got = []
    t = threading.Thread(target=lambda: got.append(p.stdout.read()))
    t.start()
    for at in range(0, len(raw), 4099):
        p.stdin.write(raw[at:at + 4099])
        p.stdin.flush()
    p.stdin.close()
    t.join(60)
    assert p.wait(60) == 0, p.stderr.read().decode()
    p.stderr.close()
    p.stdout.close()
    assert got[0] == want.tobytes()
    for block in ("1", "1601"):
        run(["--block", block, "-i", str(inp), "-o", str(out)])
        assert (np.fromfile(str(out), np.int16).reshape(a.shape) == want).all(), block
