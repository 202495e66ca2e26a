"""What the audio tests share: the integer input generator, the recorded cases of tests/golden/audio_ref.npz, and the
host checker (tests/audio_chain_check.cpp over csrc/audio_chain.hpp), built once per test session."""
import functools
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

import _libs as L
from ntscsim import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "audio_ref.npz")

# ------------------------------------------------------------------------------------------------ inputs
def _hash(n, seed):
    """A 64-bit integer hash of 0 .. n-1 (splitmix-style), the generator's only source of irregularity."""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
    return x


def _osc(n, step, amp):
    """An integer 'sine': phase n * step mod 65536 through a parabola per half wave, peak `amp`."""
    p = (np.arange(n, dtype=np.int64) * step) & 0xFFFF
    q = p & 0x7FFF
    v = (q * (32768 - q)) >> 13                                                 # 0 .. 32768
    v = np.where(p & 0x8000, -v, v)
    return (v * amp) >> 15


def make_input(kind, frames, channels, seed=1):
    """int16 [frames, channels].  music: three oscillators and a little noise per channel; loud: the same three times
    as loud, with bursts of a slow full-scale square (each edge leaves the high-passes at nearly twice full scale, which
    the chain clips); quiet: +-3 LSB; silence: zeros."""
    out = np.zeros((frames, channels), np.int64)
    if kind == "silence":
        return out.astype(np.int16)
    for c in range(channels):
        k = seed * 7 + c * 3
        noise = (_hash(frames, seed * 1000003 + c) >> np.uint64(40)).astype(np.int64)      # 24 bits
        if kind == "quiet":
            out[:, c] = noise % 7 - 3
            continue
        s = _osc(frames, 653 + 37 * k, 6000) + _osc(frames, 3271 + 101 * k, 3500) + _osc(frames, 14563 + 211 * k, 1800)
        s += noise % 257 - 128
        if kind == "loud":
            n = np.arange(frames, dtype=np.int64)
            burst = ((n // 997 + c) % 3) == 0
            square = np.where((n // (331 + 7 * c)) & 1, 32767, -32768)
            s = np.where(burst, square, s * 3)
        out[:, c] = s
    return np.clip(out, -32768, 32767).astype(np.int16)


# ------------------------------------------------------------------------------------------------ cases
# name: (switches, input kind, frames, seed, count0, rng0, block, swap channels)
HIFI = []
CASES = {
    "hifi_default": (HIFI, "music", 2048, 1, 0, 0, 0, False),
    "hifi_default_swapped": (HIFI, "music", 2048, 1, 0, 0, 0, True),
    "hifi_default_b1": (HIFI, "music", 2048, 1, 0, 0, 1, False),
    "hifi_default_b1024": (HIFI, "music", 2048, 1, 0, 0, 1024, False),
    "hifi_default_b1601": (HIFI, "music", 2048, 1, 0, 0, 1601, False),
    "hifi_default_long": (HIFI, "music", 60000, 2, 0, 100000, 0, False),
    "hifi_noemph": (["-vhs"], "music", 2048, 3, 0, 0, 0, False),
    "hifi_noemph_clip": (["-vhs"], "loud", 2048, 4, 0, 0, 0, False),
    "hifi_noemph_long": (["-vhs"], "loud", 60000, 5, 0, 7, 0, False),
    "hifi_emph_clip": (["-vhs-hifi", "1"], "loud", 2048, 6, 0, 0, 0, False),
    "linear_sp": (["-vhs", "-vhs-hifi", "0"], "music", 2048, 7, 0, 0, 0, False),
    "linear_sp_long": (["-vhs", "-vhs-hifi", "0"], "music", 12000, 8, 0, 31, 0, False),
    "linear_sp_count_2p31": (["-vhs", "-vhs-hifi", "0"], "music", 2048, 7, (1 << 31) + 12345, 0, 0, False),
    "linear_sp_count_3e9": (["-vhs", "-vhs-hifi", "0"], "quiet", 2048, 9, 3000000000, 5, 0, False),
    "linear_lp_emph": (["-vhs-hifi", "0", "-vhs-speed", "lp"], "music", 2048, 10, 0, 0, 0, False),
    "linear_ep": (["-vhs", "-vhs-speed", "ep", "-vhs-hifi", "0"], "loud", 2048, 11, 0, 0, 0, False),
    "linear_ep_long": (["-vhs", "-vhs-speed", "ep", "-vhs-hifi", "0"], "loud", 12000, 12, 0, 0, 0, False),
    "linear_pal": (["-tvstd", "pal", "-vhs", "-vhs-hifi", "0"], "music", 2048, 13, 77, 0, 0, False),
    "linear_loud_buzz": (["-vhs", "-vhs-hifi", "0", "-vhs-linear-video-crosstalk", "-12", "-vhs-linear-high-boost", "0.6"], "quiet", 2048, 14, 0, 0,
                         0, False),
    "hiss_off": (["-audio-hiss", "-200"], "music", 2048, 15, 0, 0, 0, False),
    "hiss_off_silence": (["-audio-hiss", "-200"], "silence", 2048, 16, 0, 0, 0, False),
    "hiss_full": (["-audio-hiss", "0"], "quiet", 2048, 17, 0, 12345, 0, False),
    "nocomp": (["-nocomp"], "music", 2048, 18, 0, 9, 0, False),
}
FULL_OUTPUT_FRAMES = 2048                                                        # longer runs are recorded as SHA-256


def case_input(name):
    flags, kind, frames, seed, _count0, _rng0, _block, swap = CASES[name]
    ap, _ = _capi.make_audio_params(flags)
    a = make_input(kind, frames, ap.channels, seed)
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


# ------------------------------------------------------------------------------------------------ the checker
_FLAGS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
_tmp = None


@functools.lru_cache(maxsize=None)
def checker(build="plain"):
    """Path of tests/audio_chain_check.cpp built with g++ (-ffp-contract=off, as the product), once per session."""
    global _tmp
    assert shutil.which("g++") is not None, "g++ is needed to build tests/audio_chain_check.cpp"
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="audio_chain_check_")
    exe = os.path.join(_tmp.name, "audio_chain_check_" + build)
    csrc = os.path.join(L.PKG, "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + _FLAGS[build] +
                          ["-I", csrc, "-I", os.path.join(L.ROOT, "include"), os.path.join(HERE, "audio_chain_check.cpp"), os.path.join(csrc, "glibc_rand.cpp"), "-o", exe])
    return exe


def write_cfg(path, ap):
    """The AudioCfg of an ntscsim_audio_params, as audio_chain_check reads it."""
    ints = [ap.enabled, ap.channels, ap.hifi, ap.preemphasis, ap.deemphasis, ap.hiss_level, ap.vsync_lines, ap.vpulse_end]
    dbls = [float(ap.rate), ap.highpass_hz, ap.hsync_hz, ap.hpulse_end, ap.buzz, ap.boost_gain, ap.alpha_lowpass, ap.alpha_highpass, ap.alpha_pre,
            ap.alpha_post, ap.alpha_boost]
    with open(path, "w") as f:
        f.write("\n".join([str(int(v)) for v in ints] + [float(v).hex() for v in dbls]) + "\n")


def _parse_state(text):
    line = [ln for ln in text.splitlines() if ln.startswith("state ")][-1].split()
    vals = np.array([int(x, 16) for x in line[1:31]], np.uint64).view(np.float64)
    return tuple(float(v) for v in vals), int(line[32]), int(line[34])


def run_checker(ap, audio, count0=0, rng_pos=0, block=0, build="plain"):
    """The serial chain on the host: (output like `audio`, (30 state values, count), rand() position behind it)."""
    with tempfile.TemporaryDirectory(prefix="audio_run_") as d:
        cfg, inp, outp = os.path.join(d, "cfg"), os.path.join(d, "in"), os.path.join(d, "out")
        write_cfg(cfg, ap)
        np.ascontiguousarray(audio).tofile(inp)
        r = subprocess.run([checker(build), "serial", cfg, inp, outp, str(count0), str(rng_pos), str(block)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        out = np.fromfile(outp, np.int16).reshape(np.shape(audio))
    vals, count, pos = _parse_state(r.stdout)
    return out, (vals, count), pos


def block_spec(blocks):
    """[(frames, rand() position or None), ...] as the checkers read it behind blocks="""
    return ",".join("%d:%s" % (n, "a" if p is None else p) for n, p in blocks)


def run_tracks_checker(ap, tracks, counts=None, pos=0, blocks=None, build="plain"):
    """run_checker per track, each from zeros at its count, the rand() position running through, in ONE run of the
    checker (its `tracks` mode; tests/test_audio_limits_host.py holds it against run_checker per track):
    ([(output, (30 state values, count))], rand() position behind the last)."""
    ch = ap.channels
    frames = [len(a) for a in tracks]
    whole = np.concatenate([np.ascontiguousarray(a).reshape(-1, ch) for a in tracks]) if tracks else np.zeros((0, ch), np.int16)
    with tempfile.TemporaryDirectory(prefix="audio_run_") as d:
        cfg, inp, outp, spec = os.path.join(d, "cfg"), os.path.join(d, "in"), os.path.join(d, "out"), os.path.join(d, "spec")
        write_cfg(cfg, ap)
        whole.tofile(inp)
        with open(spec, "w") as f:
            for t, n in enumerate(frames):
                f.write("%d %d %s\n" % (n, counts[t] if counts else 0, block_spec(blocks[t]) if blocks is not None and blocks[t] is not None else "-"))
        r = subprocess.run([checker(build), "tracks", cfg, inp, outp, str(pos), spec], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        out = np.fromfile(outp, np.int16).reshape(-1, ch)
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("state ")]
    assert len(lines) == len(frames), r.stdout
    res, at = [], 0
    for n, ln in zip(frames, lines):
        vals = np.array([int(x, 16) for x in ln[1:31]], np.uint64).view(np.float64)
        res.append((out[at:at + n], (tuple(float(v) for v in vals), int(ln[32]))))
        pos = int(ln[34])
        at += n
    return res, pos


def run_checker_mode(mode, ap, audio, *args, build="plain"):
    """planned / converge: (return code, output text)."""
    with tempfile.TemporaryDirectory(prefix="audio_run_") as d:
        cfg, inp = os.path.join(d, "cfg"), os.path.join(d, "in")
        write_cfg(cfg, ap)
        np.ascontiguousarray(audio).tofile(inp)
        r = subprocess.run([checker(build), mode, cfg, inp] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def plan(ap, audio, seg_len, warmup, count0=0, rng_pos=0, build="plain"):
    """((segments, repaired), [the repaired segments]) of one planned call on the host (audio_run_planned)."""
    rc, out = run_checker_mode("plan", ap, audio, count0, rng_pos, seg_len, warmup, build=build)
    assert rc == 0, out
    w = out.split()
    assert w[0] == "plan:" and w[5] == "which", out
    which = [int(x) for x in w[6:]]
    assert len(which) == int(w[4]), out
    return (int(w[2]), int(w[4])), which


def plan_stats(ap, audio, seg_len, warmup, count0=0, rng_pos=0):
    """(segments, repaired) of one planned call on the host: what the device's stats must say for the same plan."""
    return plan(ap, audio, seg_len, warmup, count0, rng_pos)[0]


def mixed_repairs(segments, which):
    """The condition of a mixed plan: some segments are repaired, not all that could be (the first never is), and at
    least one accepted segment directly follows a repaired one -- it is accepted against the truth a repair produced."""
    w = set(which)
    return 0 < len(w) < segments - 1 and any(j + 1 < segments and j + 1 not in w for j in w)


def host_pulses(ap, count0, n):
    with tempfile.TemporaryDirectory(prefix="audio_run_") as d:
        cfg, outp = os.path.join(d, "cfg"), os.path.join(d, "out")
        write_cfg(cfg, ap)
        subprocess.check_call([checker(), "pulses", cfg, str(count0), str(n), outp])
        return np.fromfile(outp, np.uint8)


def state_bits(vals):
    return np.array(vals, np.float64).view(np.uint64)
