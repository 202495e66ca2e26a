#!/usr/bin/env python3
"""Speed of YUV422P fields WITH PARAMETERS PER FIELD in one call (ntscsim_mixed_fields422_device), 720x480, resident in HBM.

In the same run:
  (a)  the case the call exists for: --sets sets (noise levels, tape speed, sharpening, head-switch phase, S-Video or
       composite out, pre-emphasis, Y/C recombine passes drawn from a fixed seed), one frame = two fields each, through ONE
       mixed call (device events, median of --reps after --warmup; the host side of the call and its wall clock are
       recorded beside them) -- against the same fields as one ntscsim_fields422_device call per set on one context per
       set, each on its context's own stream, which is what a caller had to do before (wall clock from the first call
       to the device's last kernel; the contexts are made and warmed outside the clock)
  (b)  the price of the twelve-sweep kernel: 2 * --sets fields all on ONE set (-vhs) through the mixed call, through
       ntscsim_fields422_device with ntscsim_debug_no_fast_decode(1) (k422_process, whose body the mixed call shares), and
       through ntscsim_fields422_device as it runs by itself (the streamed kernel); device events, medians

  (c)  --compare-tree PARENT: what hoisting the kernel bodies did to the single-set k422_process, against a built tree of
       the parent commit: leg (b)'s k422_process form in a fresh process per figure (this tool with --process-only
       --tree T), the two trees alternating, --rounds times.  Written under "parent_against_this" of the --out file.

The tool works in place, as the 8-bit tool does: every timed call is preceded (outside the clock) by a copy of the
pristine frames into its destination, and every descriptor carries an explicit rand() position, so all forms compute
the same fields.  Verified before a number is printed: (a)'s two forms and (b)'s three forms wrote the same bytes, whole
destination buffers (row padding included).

    python tools/bench_mixed_fields422.py [--sets 300] [--reps 5] [--warmup 2] [--compare-tree PARENT [--rounds 3]]
                                          [--out profiles/mixed_fields422.json]"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree_arg():
    """--tree T (with --process-only): import the package of that tree instead of this one"""
    if "--tree" in sys.argv[:-1]:
        return os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
    return ROOT


sys.path.insert(0, os.path.join(_tree_arg(), "composite-video-simulator_amd"))

W, H = 720, 480
LS_Y, LS_C = W + 16, W // 2 + 8          # both fields of a frame in one call: luma rows of at least W + 2; 16 / 8-byte aligned
FRAME = LS_Y * H + 2 * LS_C * H


def make_sets(n, make_params):
    rnd = random.Random(422)
    sets = []
    for i in range(n):
        flags = []
        if i % 4:
            flags += ["-vhs", "-vhs-speed", ("sp", "lp", "ep")[rnd.randrange(3)]]
            if i % 4 == 3:
                flags += ["-vhs-svideo", "1"]
        if i % 5 == 0:
            flags += [("-comp-catv", "-comp-catv2", "-comp-catv3")[rnd.randrange(3)]]
        if i % 7 == 0:
            flags += ["-yc-recomb", str(rnd.randrange(1, 3))]
        flags += ["-noise", str(rnd.randrange(0, 12)), "-chroma-noise", str(rnd.randrange(0, 24)),
                  "-chroma-phase-noise", str(rnd.randrange(0, 8))]
        sets.append(make_params(flags, vhs_out_sharpen=0.25 * rnd.randrange(0, 12), vhs_out_sharpen_chroma=0.05 * rnd.randrange(0, 20),
                                vhs_head_switching_phase=1.0 - (4.0 + rnd.random()) / 262.5))
    return sets


def compare_trees(a, parent):
    """(c): fresh processes, parent and this tree alternating"""
    def last_json(cmd, cwd):
        out = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, check=True, timeout=600).stdout
        return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])

    trees = (("parent", parent), ("this", ROOT))
    r = {"rounds": a.rounds, "k422_process_single_set_ms": {"parent": [], "this": []}}
    for _ in range(a.rounds):
        for name, tree in trees:
            j = last_json([sys.executable, os.path.abspath(__file__), "--process-only", "--sets", str(a.sets), "--reps", str(a.reps),
                           "--warmup", str(a.warmup), "--tree", tree], ROOT)
            assert j["kernels"][-1] == "k422_process", j["kernels"]
            r["k422_process_single_set_ms"][name].append(j["ms"])
    for name, _ in trees:
        v = r["k422_process_single_set_ms"][name]
        r[name + "_range_ms"] = [min(v), max(v)]
        r[name + "_spread"] = (max(v) - min(v)) / min(v)
    r["this_median_over_parent_median"] = (statistics.median(r["k422_process_single_set_ms"]["this"]) /
                                           statistics.median(r["k422_process_single_set_ms"]["parent"]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--process-only", action="store_true", help="(c) alone: one JSON line, old interface only")
    ap.add_argument("--tree", default=None, help="with --process-only: the built tree whose package is measured")
    ap.add_argument("--compare-tree", default=None, help="a built tree of the parent commit: adds (c)")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()

    import torch
    import ntscsim
    if not torch.cuda.is_available():
        sys.exit("bench_mixed_fields422.py needs a GPU")
    stream = torch.cuda.Stream()
    n_sets, n = a.sets, 2 * a.sets
    gen = torch.Generator(device="cuda")
    gen.manual_seed(422)
    # video levels in the pixels (16 .. 235), anything in the row padding
    pristine = torch.randint(16, 236, (n_sets, FRAME), dtype=torch.uint8, device="cuda", generator=gen)
    dst = [torch.zeros((n_sets, FRAME), dtype=torch.uint8, device="cuda") for _ in range(3)]

    def planes(buf, f):
        y = buf[f, :LS_Y * H].view(H, LS_Y)
        u = buf[f, LS_Y * H:LS_Y * H + LS_C * H].view(H, LS_C)
        v = buf[f, LS_Y * H + LS_C * H:].view(H, LS_C)
        return [y, u, v]

    # field k: frame k // 2, parity (k & 1) ^ 1, fieldno k, rand() position k * 2^21 (past any field's draws)
    def jobs_on(buf, ks):
        return [{"dst": planes(buf, k // 2), "field": (k & 1) ^ 1, "fieldno": k, "rng_pos": k << 21} for k in ks]

    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "width": W, "height": H,
              "fields": n, "sets": n_sets, "linesizes": [LS_Y, LS_C, LS_C]}

    def events(fn, buf):
        ms = []
        for i in range(a.warmup + a.reps):
            with torch.cuda.stream(stream):
                buf.copy_(pristine)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    def wall(fn, buf):
        ms = []
        for i in range(a.warmup + a.reps):
            buf.copy_(pristine)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    vhs = ntscsim.make_params_to_composite(["-vhs"])
    one = ntscsim.FieldSimulator(params=vhs)
    proc_descs = one.build_descs422(jobs_on(dst[1], range(n)))

    def run_process():
        one.debug_no_fast_decode(1)
        one.run_descs422(proc_descs, W, H, stream=stream.cuda_stream)
        one.debug_no_fast_decode(0)

    if a.process_only:
        r = events(run_process, dst[1])
        r["kernels"] = one.last_kernels()
        one.close()
        print(json.dumps(r))
        return

    # ---- (a)
    sets = make_sets(n_sets, ntscsim.make_params_to_composite)
    sim = ntscsim.FieldSimulator(params=ntscsim.make_params_to_composite([]))
    set_arr = sim.build_sets422(sets)
    mixed_descs = sim.build_mixed_descs422([k // 2 for k in range(n)], jobs_on(dst[0], range(n)))

    def run_mixed():
        sim.run_mixed_descs422(set_arr, mixed_descs, W, H, stream=stream.cuda_stream)

    case = events(run_mixed, dst[0])
    case["kernels"] = sim.last_kernels()
    # the host side of the one call (validating and deriving the sets, the plan, the staged records), and the call on the
    # wall clock from its start to the device's last kernel, as the per-set form is timed
    dst[0].copy_(pristine)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_mixed()
    case["host_ms_of_the_call"] = (time.perf_counter() - t0) * 1e3
    stream.synchronize()
    case["wall"] = wall(run_mixed, dst[0])
    result["a_mixed_call"] = case
    per = [ntscsim.FieldSimulator(params=p) for p in sets]
    per_descs = [c.build_descs422(jobs_on(dst[1], (2 * s, 2 * s + 1))) for s, c in enumerate(per)]

    def run_per_set():
        for c, d in zip(per, per_descs):
            c.run_descs422(d, W, H, stream=0)              # (0: the context's own stream)

    result["a_one_call_per_set"] = wall(run_per_set, dst[1])
    forms = {}
    for c in per:
        k = ";".join(c.last_kernels())
        forms[k] = forms.get(k, 0) + 1
    result["a_one_call_per_set"]["kernel_forms"] = forms
    torch.cuda.synchronize()
    if not torch.equal(dst[0], dst[1]):
        sys.exit("(a): the mixed call differs from one call per set (%d bytes)" % int((dst[0] != dst[1]).sum()))
    result["a_per_set_over_mixed"] = result["a_one_call_per_set"]["ms"] / case["ms"]
    result["a_per_set_over_mixed_wall"] = result["a_one_call_per_set"]["ms"] / case["wall"]["ms"]
    result["a_fields_per_s"] = n / (case["ms"] * 1e-3)
    for c in per:
        c.close()
    print("a", json.dumps(result), flush=True)

    # ---- (b)
    uni_descs = sim.build_mixed_descs422([0] * n, jobs_on(dst[0], range(n)))
    uni_sets = sim.build_sets422([vhs])

    def run_uniform_mixed():
        sim.run_mixed_descs422(uni_sets, uni_descs, W, H, stream=stream.cuda_stream)

    fast_descs = one.build_descs422(jobs_on(dst[2], range(n)))

    def run_fast():
        one.run_descs422(fast_descs, W, H, stream=stream.cuda_stream)

    b = {"set": "-vhs"}
    b["mixed_call"] = events(run_uniform_mixed, dst[0])
    b["mixed_call"]["kernels"] = sim.last_kernels()
    b["k422_process_single_set"] = events(run_process, dst[1])
    b["k422_process_single_set"]["kernels"] = one.last_kernels()
    b["streamed_single_set"] = events(run_fast, dst[2])
    b["streamed_single_set"]["kernels"] = one.last_kernels()
    torch.cuda.synchronize()
    if not torch.equal(dst[0], dst[1]) or not torch.equal(dst[0], dst[2]):
        sys.exit("(b): the three forms differ")
    b["mixed_over_k422_process"] = b["mixed_call"]["ms"] / b["k422_process_single_set"]["ms"]
    b["mixed_over_streamed"] = b["mixed_call"]["ms"] / b["streamed_single_set"]["ms"]
    result["b_all_fields_on_one_set"] = b
    result["verified"] = "(a) mixed call == one call per set; (b) mixed == k422_process == streamed; whole destination buffers"
    sim.close()
    one.close()
    if a.compare_tree:
        result["parent_against_this"] = compare_trees(a, os.path.abspath(a.compare_tree))
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
