"""cassette_cli's host fallback (--host: csrc/cass_chain.hpp run serially, no GPU touched): the byte stream equals the
checker's on this host's libm, a pipe fed in pieces equals a file, --block leaves the bytes unchanged -- with 57 taps
the FIR's history then crosses every call."""
import os
import subprocess
import threading

import numpy as np

import _cass_ref as A
import _libs as L
from ntscsim import _capi

EXE = os.path.join(L.PKG, "cassette_cli")
FLAGS = ["-preset", "3", "-mono", "-preemphasis", "1", "-deemphasis", "1"]


def run(args, data=None):
    r = subprocess.run([EXE, "--host"] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    return r


def test_bytes_equal_the_checker(tmp_path):
    cp = _capi.make_cass_params(FLAGS)
    a = A.make_input("music", 3001, 2, 3)
    want, _state, pos = A.run_checker(cp, a, rng_pos=123)
    inp, out = tmp_path / "in.s16", tmp_path / "out.s16"
    a.tofile(str(inp))
    r = run(["--rng-pos", "123"] + FLAGS + ["-i", str(inp), "-o", str(out)])
    got = np.fromfile(str(out), np.int16).reshape(a.shape)
    assert (got == want).all()
    assert (got[:, 0] == got[:, 1]).all()
    assert ("57 taps, on the host, rand() position %d" % pos) in r.stderr.decode()


def test_pipe_in_pieces_and_blocks(tmp_path):
    flags = ["-preset", "3"]
    cp = _capi.make_cass_params(flags)
    a = A.make_input("music", 40000, 2, 4)                                      # 160,000 bytes: more than one pipe buffer
    want, _state, _pos = A.run_checker(cp, a)
    inp, out = tmp_path / "in.s16", tmp_path / "out.s16"
    a.tofile(str(inp))
    run(flags + ["-i", str(inp), "-o", str(out)])
    assert (np.fromfile(str(out), np.int16).reshape(a.shape) == want).all()
    # through pipes, written in pieces that cut sample frames
    p = subprocess.Popen([EXE, "--host"] + flags + ["-i", "-", "-o", "-"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    raw = a.tobytes()
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
    for block in ("1", "3", "1601"):
        run(["--block", block] + flags + ["-i", str(inp), "-o", str(out)])
        assert (np.fromfile(str(out), np.int16).reshape(a.shape) == want).all(), block


def test_refusals(tmp_path):
    for args in (["-o", "x"], ["-i", "x", "-o", "y", "-low", "0"], ["-i", "x", "-o", "y", "-headalign", "200"], ["-i", "x", "-o", "y", "-nosuch"]):
        r = subprocess.run([EXE, "--host"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, cwd=str(tmp_path))
        assert r.returncode == 1 and b"cassette_cli:" in r.stderr, args
