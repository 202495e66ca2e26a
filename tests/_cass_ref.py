"""What the cassette tests share: the recorded cases of tests/golden/cass_ref.npz and the host checker
(tests/cass_chain_check.cpp over csrc/cass_chain.hpp), built once per test session.  The inputs are
tests/_audio_ref.py's integer generator."""
import functools
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

import _libs as L
from _audio_ref import make_input
from ntscsim import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "cass_ref.npz")

# name: (switches, input kind, frames, seed, count0, rng0, block, swap channels)
BAD_DECK = ["-preset", "3"]                                                      # tilt 10: 57 taps
CASES = {
    "default": ([], "music", 2048, 1, 0, 0, 0, False),
    "default_swapped": ([], "music", 2048, 1, 0, 0, 0, True),
    "preset0": (["-preset", "0"], "music", 1024, 2, 0, 0, 0, False),
    "preset1": (["-preset", "1"], "music", 1024, 3, 0, 0, 0, False),
    "preset2": (["-preset", "2"], "music", 1024, 4, 0, 0, 0, False),
    "preset3": (BAD_DECK, "music", 2048, 5, 0, 0, 0, False),
    "preset3_b1": (BAD_DECK, "music", 2048, 5, 0, 0, 1, False),
    "preset3_b3": (BAD_DECK, "music", 2048, 5, 0, 0, 3, False),
    "preset3_b1601": (BAD_DECK, "music", 2048, 5, 0, 0, 1601, False),
    "preset4": (["-preset", "4"], "music", 1024, 6, 0, 0, 0, False),
    "headalign0": (["-headalign", "0"], "music", 1024, 7, 0, 0, 0, False),
    "headalign_neg": (["-headalign", "-3"], "music", 1024, 8, 0, 0, 0, False),
    "headalign_pos": (["-headalign", "3"], "music", 1024, 8, 0, 0, 0, False),
    "nowaver": (["-headalignwaver", "0"], "music", 1024, 9, 0, 0, 0, False),
    "pre": (["-preemphasis", "1"], "music", 1024, 10, 0, 0, 0, False),
    "post": (["-deemphasis", "1"], "music", 1024, 10, 0, 0, 0, False),
    "both": (["-preemphasis", "1", "-deemphasis", "1"], "music", 2048, 10, 0, 0, 0, False),
    "both_swapped": (["-preemphasis", "1", "-deemphasis", "1"], "music", 2048, 10, 0, 0, 0, True),
    "mono": (["-mono"], "music", 2048, 1, 0, 0, 0, False),
    "mono_both_preset1": (["-mono", "-preset", "1", "-preemphasis", "1", "-deemphasis", "1"], "music", 1024, 11, 0, 77, 0, False),
    "hiss_off": (["-audio-hiss", "-200"], "music", 1024, 12, 0, 0, 0, False),
    "hiss_off_silence": (["-audio-hiss", "-200"], "silence", 1024, 13, 0, 0, 0, False),
    "hiss_full": (["-audio-hiss", "0"], "quiet", 1024, 14, 0, 12345, 0, False),
    "silence": ([], "silence", 1024, 15, 0, 3, 0, False),
    "clip": ([], "loud", 2048, 16, 0, 0, 0, False),
    "clip_both": (["-preemphasis", "1", "-deemphasis", "1", "-preset", "0"], "loud", 2048, 17, 0, 0, 0, False),
    "override": (["-preset", "3", "-headalign", "2", "-low", "9000", "-high", "0x32"], "music", 1024, 18, 0, 0, 0, False),
    "count_2p31": (["-preset", "0"], "music", 2048, 19, (1 << 31) + 12345, 0, 0, False),
    "count_3e9": (["-deemphasis", "1"], "quiet", 2048, 20, 3000000000, 5, 0, False),
    "long_20hz": (BAD_DECK + ["-deemphasis", "1"], "music", 60000, 21, 0, 100000, 0, False),
    "long_100hz": (["-preset", "1", "-mono", "-preemphasis", "1", "-deemphasis", "1"], "loud", 12000, 22, 0, 31, 0, False),
}
FULL_OUTPUT_FRAMES = 2048                                                        # longer runs are recorded as SHA-256
SINE_COUNT0 = (0, (1 << 31) + 12345, 3000000000)                                 # one recorded table of 2048 sines each


def case_input(name):
    _flags, kind, frames, seed, _count0, _rng0, _block, swap = CASES[name]
    a = make_input(kind, frames, 2, seed)
    if swap:
        a = np.ascontiguousarray(a[:, ::-1])
    return a


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(FIXTURE)
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta"}


def recorded_sines(count0, frames):
    """The tool's sin() results of frames count0 .. count0 + frames - 1, or None if no table holds them."""
    _meta, arrays = fixture()
    key = "sines_%d" % count0
    if key in arrays and frames <= arrays[key].size:
        return arrays[key][:frames]
    return None


# ------------------------------------------------------------------------------------------------ the checker
_FLAGS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
_tmp = None


@functools.lru_cache(maxsize=None)
def checker(build="plain"):
    """Path of tests/cass_chain_check.cpp built with g++ (-ffp-contract=off, as the product), once per session."""
    global _tmp
    assert shutil.which("g++") is not None, "g++ is needed to build tests/cass_chain_check.cpp"
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="cass_chain_check_")
    exe = os.path.join(_tmp.name, "cass_chain_check_" + build)
    csrc = os.path.join(L.PKG, "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + _FLAGS[build] +
                          ["-I", csrc, "-I", os.path.join(L.ROOT, "include"), os.path.join(HERE, "cass_chain_check.cpp"), os.path.join(csrc, "glibc_rand.cpp"), "-o", exe])
    return exe


def write_cfg(path, cp):
    """The CassCfg of an ntscsim_cass_params, as cass_chain_check reads it."""
    ints = [cp.preemphasis, cp.deemphasis, cp.mono, cp.hiss_level, cp.taps]
    dbls = [float(cp.rate), cp.highpass_hz, cp.head_tilt, cp.head_tilt_waver, cp.alpha_lowpass, cp.alpha_highpass, cp.alpha_pre, cp.alpha_post]
    with open(path, "w") as f:
        f.write("\n".join([str(int(v)) for v in ints] + [float(v).hex() for v in dbls]) + "\n")


def _parse_state(text):
    """((28 filter values: 24 band-pass, pre[2], post[2]; count; history as [taps-1, 2]; all as bit patterns), rand() position)"""
    line = [ln for ln in text.splitlines() if ln.startswith("state ")][-1].split()
    vals = np.array([int(x, 16) for x in line[1:29]], np.uint64)
    count, pos, taps = int(line[30]), int(line[32]), int(line[34])
    hist = np.array([int(x, 16) for x in line[36:]], np.uint64).reshape(taps - 1, 2)
    return (vals, count, hist), pos


def _sines_arg(d, sines):
    if sines is None:
        return "-"
    path = os.path.join(d, "sines")
    np.ascontiguousarray(sines, np.float64).tofile(path)
    return path


def run_checker(cp, audio, count0=0, rng_pos=0, block=0, sines=None, build="plain"):
    """The serial chain on the host, every tap: (output like `audio`, state, rand() position behind it).  sines: the
    recorded sin() results of the run's frames; None: this host's libm."""
    with tempfile.TemporaryDirectory(prefix="cass_run_") as d:
        cfg, inp, outp = os.path.join(d, "cfg"), os.path.join(d, "in"), os.path.join(d, "out")
        write_cfg(cfg, cp)
        np.ascontiguousarray(audio).tofile(inp)
        r = subprocess.run([checker(build), "serial", cfg, inp, outp, str(count0), str(rng_pos), str(block), _sines_arg(d, sines)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        out = np.fromfile(outp, np.int16).reshape(np.shape(audio))
    state, pos = _parse_state(r.stdout)
    return out, state, pos


def run_checker_mode(mode, cp, audio, *args, sines=None, build="plain"):
    """planned / converge: (return code, output text)."""
    with tempfile.TemporaryDirectory(prefix="cass_run_") as d:
        cfg, inp = os.path.join(d, "cfg"), os.path.join(d, "in")
        write_cfg(cfg, cp)
        np.ascontiguousarray(audio).tofile(inp)
        r = subprocess.run([checker(build), mode, cfg, inp] + [str(a) for a in args] + [_sines_arg(d, sines)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def local_sines(cp, count0, n):
    """This host's libm: sin() of the frames count0 .. count0 + n - 1 in the tool's expression."""
    with tempfile.TemporaryDirectory(prefix="cass_run_") as d:
        cfg, outp = os.path.join(d, "cfg"), os.path.join(d, "out")
        write_cfg(cfg, cp)
        subprocess.check_call([checker(), "sines", cfg, str(count0), str(n), outp])
        return np.fromfile(outp, np.float64)


def plan_stats(cp, audio, seg_len, warmup_front, warmup_back, count0=0, rng_pos=0):
    """(segments, repaired by the front, repaired by the back) of one planned call on the host: what the device's
    stats must say for the same plan."""
    rc, out = run_checker_mode("plan", cp, audio, count0, rng_pos, seg_len, warmup_front, warmup_back)
    assert rc == 0, out
    w = out.split()
    return int(w[2]), int(w[4]), int(w[6])


def plan(cp, audio, seg_len, warmup_front, warmup_back, count0=0, rng_pos=0, build="plain"):
    """(plan_stats, [segments the front repaired], [segments the back repaired]) of one planned call on the host."""
    rc, out = run_checker_mode("plan", cp, audio, count0, rng_pos, seg_len, warmup_front, warmup_back, build=build)
    assert rc == 0, out
    w = out.split()
    assert w[0] == "plan:" and w[7] == "which_front" and "which_back" in w, out
    b = w.index("which_back")
    front, back = [int(x) for x in w[8:b]], [int(x) for x in w[b + 1:]]
    assert len(front) == int(w[4]) and len(back) == int(w[6]), out
    return (int(w[2]), int(w[4]), int(w[6])), front, back
