"""cassette_cli --tracks: a library of tapes, each with its own switches, in one run.  On the host (--host: the serial
chain of csrc/cass_chain.hpp per track) a run of four lines -- the common deck, a worn 57-tap one, one with both emphasis
filters, a silent mono one at -high 100 -- equals four single runs with --rng-pos chained, bytes and reported positions,
and the checker; a malformed line is an error that writes nothing.  On the device the same list goes through ONE
ntscsim_cass_mixed_tracks_host call and gives the bytes of the --host run."""
import os
import re
import subprocess

import numpy as np
import pytest

import _cass_ref as A
import _libs as L
from ntscsim import _capi

EXE = os.path.join(L.PKG, "cassette_cli")
COMMON = ["-audio-hiss", "-40"]
LINES = [[], ["-preset", "3"], ["-deemphasis", "1", "-preemphasis", "1"], ["-mono", "-high", "100", "-audio-hiss", "-200"]]
FRAMES = [3001, 2500, 1800, 700]


def positions(stderr):
    return [int(x) for x in re.findall(r"rand\(\) position (\d+)", stderr.decode())]


def make_list(tmp_path, tag):
    """inputs, the list file, the output paths"""
    inputs, outs, text = [], [], ["# in out switches", ""]
    for t, (flags, frames) in enumerate(zip(LINES, FRAMES)):
        cp = _capi.make_cass_params(COMMON + flags)
        a = A.make_input("music", frames, 2, 30 + t)
        inp, out = tmp_path / ("in%d.s16" % t), tmp_path / ("%s%d.s16" % (tag, t))
        a.tofile(str(inp))
        inputs.append((cp, a))
        outs.append(out)
        text.append("  ".join([str(inp), str(out)] + flags))
    lst = tmp_path / (tag + ".list")
    lst.write_text("\n".join(text) + "\n")
    return inputs, lst, outs


def test_tracks_equal_chained_single_runs(tmp_path):
    inputs, lst, outs = make_list(tmp_path, "tracks")
    r = subprocess.run([EXE, "--host", "--tracks", str(lst), "--rng-pos", "123"] + COMMON, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    got_pos = positions(r.stderr)
    assert len(got_pos) == 4
    pos = 123
    for t, ((cp, a), flags) in enumerate(zip(inputs, LINES)):
        single = tmp_path / ("single%d.s16" % t)
        s = subprocess.run([EXE, "--host", "--rng-pos", str(pos)] + COMMON + flags + ["-i", str(tmp_path / ("in%d.s16" % t)), "-o", str(single)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert s.returncode == 0, s.stderr.decode()
        want, _state, checker_pos = A.run_checker(cp, a, rng_pos=pos)
        got = np.fromfile(str(outs[t]), np.int16).reshape(a.shape)
        assert (got == np.fromfile(str(single), np.int16).reshape(a.shape)).all(), t
        assert (got == want).all(), t
        pos = positions(s.stderr)[0]
        assert got_pos[t] == pos == checker_pos, t
    assert [cp.taps for cp, _ in inputs] == [8, 57, 8, 8] and inputs[3][0].hiss_level == 0
    assert pos == 123 + 2 * (3001 + 2500 + 1800)                                # the silent tape draws nothing


@pytest.mark.parametrize("bad", ["lonely_word", "IN OUT -no-such-switch", "/no/such/input OUT", "IN OUT -headalign 200"])
def test_a_malformed_line_writes_nothing(tmp_path, bad):
    inputs, lst, outs = make_list(tmp_path, "bad")
    text = lst.read_text().splitlines()
    bad = " ".join({"IN": str(tmp_path / "in0.s16"), "OUT": str(tmp_path / "never.s16")}.get(w, w) for w in bad.split())
    lst.write_text("\n".join(text + [bad]) + "\n")                              # behind four good lines
    r = subprocess.run([EXE, "--host", "--tracks", str(lst)] + COMMON, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and b"cassette_cli:" in r.stderr
    assert not any(o.exists() for o in outs) and not (tmp_path / "never.s16").exists()


@pytest.mark.gpu
def test_device_tracks_equal_the_host_run(tmp_path):
    inputs, lst, outs = make_list(tmp_path, "dev")
    r = subprocess.run([EXE, "--tracks", str(lst), "--rng-pos", "123"] + COMMON, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert b"on the device" in r.stderr
    dev = [np.fromfile(str(o), np.int16) for o in outs]
    dev_pos = positions(r.stderr)
    r = subprocess.run([EXE, "--host", "--tracks", str(lst), "--rng-pos", "123"] + COMMON, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    assert positions(r.stderr) == dev_pos
    for t, o in enumerate(outs):
        assert (np.fromfile(str(o), np.int16) == dev[t]).all(), t
