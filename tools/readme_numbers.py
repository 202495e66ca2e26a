#!/usr/bin/env python3
"""Rewrites the numbers table of README.md (between the markers `<!-- numbers:begin -->` / `<!-- numbers:end -->`) from
the tracked bench files under profiles/ (run after tools/refresh_profiles.sh local <tag>):
    python tools/readme_numbers.py r06"""
import json
import sys

tag = sys.argv[1] if len(sys.argv) > 1 else "r06"
P = "profiles/%s_" % tag
line = json.load(open(P + "bench_driver_cmd.json"))          # what the driver's command printed
full = json.load(open(P + "bench.json"))                     # bench_extras.json of the same run
flt = json.load(open(P + "bench_float.json"))
f32 = json.load(open(P + "bench_fast32.json"))
toc = json.load(open(P + "bench_to_composite.json"))
try:
    dflt = json.load(open(P + "bench_line_default_cmd.json"))
except Exception:
    dflt = None
e = full.get("end_to_end", {})
fs, f4 = e.get("field_submit_detail", {}), e.get("field_submit422_detail", {})


def rate(d, k):
    x = d.get(k)
    return (x.get("fields_per_s") if isinstance(x, dict) else x) or 0


def k(v):
    return "%.0fk" % (v / 1e3) if v >= 10000 else "%.2fk" % (v / 1e3)


cb = line["cpu_baseline"]
rows = [
    ("**headline, driver's window** (`python bench.py --gpus 1 --steps 20 --warmup 5`): 600-field `-vhs` clip resident in HBM, exact mode, four steps in flight",
     "**%s fields/s** (`value`), %s sustained over 0.5 s" % (k(line["value"]), k(line["value_sustained"])), "`%sbench_driver_cmd.json`" % P),
    ("the same with `bench.py`'s own defaults (100 timed steps after 40 warm-up steps)",
     "%s fields/s" % k(dflt["value"]) if dflt else "-", "`%sbench_line_default_cmd.json`" % P),
    ("`roofline` of the dominant kernel (`k_decode_fast<true,double>`, algorithmic 8·W·L bytes per field ÷ its duration ÷ 8 TB/s)",
     "`frac` **%.3f** (%.0f GB/s); the kernel moves %.2f × those bytes over HBM (encoder + decoder: %.2f ×, the composite plane between them); the bound that applies is VALU issue: %.2f of its nominal capacity for the whole path" % (
         line["roofline"]["frac"], line["roofline"]["achieved"], (full["roofline"].get("traffic") or 0) / full["roofline"]["algorithmic_bytes_per_launch"],
         json.load(open("profiles/traffic.json"))["720x486 -vhs"]["path_over_algorithmic"], line["roofline"]["valu"]["path_frac_nominal"]), "DESIGN.md §5, `profiles/traffic.json`"),
    ("CPU beside it on the GPU box's host: the reference's own `composite_layer()` text, 1 thread like the tool",
     "%.1f fields/s (our C port: %.0f on 1 core, %.0f on %d cores)" % (cb["value"], cb["port_1core"], cb["port_all_cores"]["value"], cb["port_all_cores"]["cores"]),
     "`cpu_baseline`"),
    ("device-resident STREAM of fresh batches (descriptor validation, `rand()` windows, record upload inside the clock)", "%s fields/s" % k(line["side"]["device_stream"]), "`side.device_stream`"),
    ("other sizes, `-vhs`: 1920×1080 / 3840×2160", "%s / %s fields/s" % (k(line["side"]["sizes"]["1920x1080"]), k(line["side"]["sizes"]["3840x2160"])), "`side.sizes`"),
    ("default preset (BASELINE configs[0] on the GPU)", "%s fields/s" % k(line["side"]["presets"]["default"]), "`side.presets`"),
    ("the YUV422P tool (`ffmpeg_to_composite`), `-vhs`, device resident", "%s frames/s (sustained %s)" % (k(toc["value"]), k(toc.get("value_sustained", 0))), "`%sbench_to_composite.json`" % P),
    ("the raw-composite decoder (`ffmpeg_raw28ntsc`), 600-field capture resident in HBM", "%s fields/s" % k(line["side"]["raw28"]), "`side.raw28`"),
    ("**tolerance mode `NTSCSIM_MODE_FLOAT`** (all-float pipeline, ≤ 1 LSB, never the default)",
     "**%s fields/s**, decoder `roofline.frac` %.3f (FAST32, the exact kernels with float states: %s)" % (k(flt["value"]), flt["roofline"]["frac"], k(f32["value"])),
     "`%sbench_float.json`, DESIGN.md §3b" % P),
    ("drop-in on HOST frames, synchronous: one `ntscsim_field()` per `composite_layer()` call (`host/field_loop.cpp --mode sync`; a pipeline of wavefront roles, DESIGN §1c): `posix_memalign` frames / pinned frames / from Python",
     "%s / %s / %s fields/s (%.0f / %.0f × the reference on one core)" % (k(e.get("field_call_cpp", 0)), k(e.get("field_call_cpp_pinned", 0)), k(e.get("field_call", 0)),
                                                                       e.get("field_call_cpp", 0) / cb["value"], e.get("field_call_cpp_pinned", 0) / cb["value"]), "`side.field_call`, `side.field_call_pinned`, `side.field_call_python`"),
    ("... asynchronous, `ntscsim_submit()` / `ntscsim_wait()` at depth 32 (`host/field_loop.cpp`): frames from `ntscsim_host_frame_alloc()` / a pool declared with `ntscsim_host_pin()` / plain `posix_memalign` frames (staged)",
     "%s / %s / %s fields/s" % (k(e.get("field_submit", 0)), k(rate(fs, "depth32_declared_pool")), k(rate(fs, "depth32_malloc_frames_staged"))), "`end_to_end.field_submit*`"),
    ("the YUV422P tool's loop on host frames, depth 32 (`host/field_loop422.cpp`): pinned planes / plain heap planes, no `mallopt` / tight rows (704 wide)",
     "%s / %s / %s fields/s" % (k(e.get("field_submit422", 0)), k(rate(f4, "depth32_vhs_heap_planes")), k(rate(f4, "tight_rows_704"))),
     "`end_to_end.field_submit422*`"),
    ("... synchronous: one `ntscsim_field422()` per loop iteration (four wavefront roles, `k422_pipe`, DESIGN §7c): heap planes / pinned planes",
     "%s / %s fields/s" % (k(e.get("field_call422", 0) or rate(f4, "loop_sync_fields_per_s")), k(e.get("field_call422_pinned", 0))), "`side.field_call422`, `side.field_call422_pinned`"),
    ("whole clips from host memory (`ntscsim_frames_host`): BGRA out / YUV420P out / YUV420P in and out", "%s / %s / %s fields/s" % (
        k(e.get("bgra_pinned", 0)), k(e.get("yuv420p_pinned", 0)), k(e.get("yuv420p_in_yuv420p_out_pinned", 0))), "`end_to_end.*_pinned`"),
    ("one process per GPU, C++ host over `rccl.h` (`host/rank_bench.cpp`), with the one rank this box has", "%s fields/s, checksums verified" % k(line["side"]["multi_gpu_cpp_host"]), "`side.multi_gpu_cpp_host`"),
]


def led_row(path="profiles/led.json"):
    """The vhsled stage's row, from tools/bench_led.py's file."""
    c = json.load(open(path))
    a, b, d7, d19 = (c["cases"][n] for n in ("720x486_capture", "1920x1080_capture", "720x486_all_dark", "1920x1080_all_dark"))
    return ("the scanline left-edge aligner (`ffmpeg_vhsled`, `ntscsim_led_*`): 600 frames resident in HBM through one `ntscsim_led_frames_device` call, "
            "a dark border of 8..40 pixels jittering per row (`tools/bench_led.py`)",
            "720×486: **%s frames/s**, `frac_hbm` %.3f on 8·W·H bytes per frame, %.2f × the time of a device-to-device copy of the same traffic in the same run; "
            "1920×1080: %s frames/s, `frac_hbm` %.3f, %.2f × the copy; all-dark frames (every scan reads its whole row): %s / %s frames/s, %.2f / %.2f × the copy; "
            "the reference's loop on one CPU core of the build machine (not the GPU host): %.0f frames/s at 720×486" % (
                k(a["frames_per_s"]), a["frac_hbm"], a["led_over_copy"], k(b["frames_per_s"]), b["frac_hbm"], b["led_over_copy"],
                k(d7["frames_per_s"]), k(d19["frames_per_s"]), d7["led_over_copy"], d19["led_over_copy"], c["reference_cpu"]["frames_per_s"]),
            "`profiles/led.json`, DESIGN.md §7i")


def filmac_row(path="profiles/filmac.json"):
    """The filmac stage's row, from tools/bench_filmac.py's file."""
    c = json.load(open(path))
    a, ag, b, bg = (c["cases"][n] for n in ("720x486_plain", "720x486_gamma", "1920x1080_plain", "1920x1080_gamma"))
    km = b["kernel_ms"]
    return ("the film auto-contrast (`filmac`, `ntscsim_filmac_*`): 600 frames of drifting noise resident in HBM through one `ntscsim_filmac_frames_device` call, "
            "the level state on the device throughout (`tools/bench_filmac.py`)",
            "720×486: **%s frames/s** (%s with `-gamma ntsc`), %.2f × the time of a device-to-device copy of 8·W·H bytes per frame and %.2f × that of 12·W·H in the same run; "
            "1920×1080: %s frames/s (%s), %.2f × / %.2f × the copies; the five kernels at 1920×1080: statistics %.2f, frame levels %.3f, recurrence %.2f, tables %.3f, map %.2f ms; "
            "the reference's loop on one CPU core of the build machine (not the GPU host): %.0f frames/s at 720×486, %.0f with `-gamma 2.2`" % (
                k(a["frames_per_s"]), k(ag["frames_per_s"]), a["filmac_over_copy_8wh"], a["filmac_over_copy_12wh"],
                k(b["frames_per_s"]), k(bg["frames_per_s"]), b["filmac_over_copy_8wh"], b["filmac_over_copy_12wh"],
                km["k_filmac_stats"], km["k_filmac_frame_levels"], km["k_filmac_levels"], km["k_filmac_tables"], km["k_filmac_apply"],
                c["reference_cpu"]["frames_per_s"], c["reference_cpu"]["frames_per_s_gamma"]),
            "`profiles/filmac.json`, DESIGN.md §7j")


def pixmap_rows(path="profiles/pixmap.json"):
    """The posterize and the colormap stage's rows, from tools/bench_pixmap.py's file."""
    j = json.load(open(path))
    c = j["cases"]

    def cell(stage, size):
        g, r = c["%s_gradient_%s" % (size, stage)], c["%s_random_green_%s" % (size, stage)]
        return k(g["frames_per_s"]), k(r["frames_per_s"]), g["frac_hbm"], g["over_copy"], r["over_copy"]

    p7, p19 = cell("post", "720x486"), cell("post", "1920x1080")
    n7, n19, m7, m19 = (cell(st, sz) for st in ("cmap_nomap", "cmap_map") for sz in ("720x486", "1920x1080"))
    ref = j["reference_cpu"]
    what = "600 frames resident in HBM through one `ntscsim_%s_frames_device` call, smooth gradients / uniform random green (`tools/bench_pixmap.py`)"
    return [("the bit-mask posteriser (`ffmpeg_posterize`, `ntscsim_post_*`): " + what % "post",
             "720×486: **%s / %s frames/s**, `frac_hbm` %.3f on 8·W·H bytes per frame, %.2f / %.2f × the time of a device-to-device copy of the same traffic in the same run; "
             "1920×1080: %s / %s frames/s, `frac_hbm` %.3f, %.2f / %.2f × the copy; "
             "the reference's loop on one CPU core of the build machine (not the GPU host): %.0f frames/s at 720×486" % (p7 + p19 + (ref["frames_per_s_post"],)),
             "`profiles/pixmap.json`, DESIGN.md §7k"),
            ("the false-colour table stage (`ffmpeg_colormap`, `ntscsim_cmap_*`): " + what % "cmap" + ", the table on the device throughout",
             "no map in any descriptor, 720×486: **%s / %s frames/s**, %.2f / %.2f × the copy, %.2f / %.2f × `k_post_frames` (the random-green figure is the LDS bank-conflict test: no table replication); "
             "1920×1080: %s / %s frames/s, %.2f / %.2f × the copy; a map in every descriptor (table filled from the map's row, plus `k_cmap_take`): "
             "720×486 %s / %s frames/s, %.2f / %.2f × the copy; 1920×1080 %s / %s, %.2f / %.2f ×; "
             "the reference's loops on one CPU core of the build machine: %.0f frames/s at 720×486" % (
                 n7[0], n7[1], n7[3], n7[4], c["720x486_gradient_cmap_nomap"]["over_post"], c["720x486_random_green_cmap_nomap"]["over_post"],
                 n19[0], n19[1], n19[3], n19[4], m7[0], m7[1], m7[3], m7[4], m19[0], m19[1], m19[3], m19[4], ref["frames_per_s_cmap"]),
             "`profiles/pixmap.json`, DESIGN.md §7k")]


def audio_tracks_row(path="profiles/audio_tracks.json"):
    """The row of many audio tracks in one call, from tools/bench_audio_tracks.py's file."""
    j = json.load(open(path))
    h, s = j["cases"]["hifi"], j["cases"]["linear_sp"]

    def cell(c):
        t, b = c["tracks_call"], c["b_single_track_of_the_total_length"]
        km = t["kernel_ms"]
        return (t["ms"], c["times_real_time"], c["a_one_call_per_track"]["ms"], c["a_over_tracks"], b["ms"], c["tracks_over_b"],
                km["draws_and_pulses"], km["k_audio_track_segments"], km["k_audio_track_verify"], b["kernel_ms"]["k_audio_verify_repair"], t["repaired"])

    return ("many audio tracks in one call (`ntscsim_audio_tracks_device`): %d independent tracks of %g s resident in HBM, each with its own state on the device "
            "(`tools/bench_audio_tracks.py`); (a) the same tracks as one `ntscsim_audio_device` call each with `set_state` / `get_state` between them, wall clock; "
            "(b) one `ntscsim_audio_device` call over a single track of the same total length; all in the same run" % (j["tracks"], j["frames_per_track"] / j["rate"]),
            "stereo Hi-Fi: **%.1f ms** (%.0f × real time); (a) %.0f ms, so the one call is worth **%.1f ×**; (b) %.1f ms, the tracks call takes %.2f × that; "
            "kernels: draws %.2f, segments %.1f, verify %.2f ms (the single track's walk: %.2f ms); %d segments repaired.  "
            "Linear mono SP: %.1f ms (%.0f × real time); (a) %.0f ms, %.1f ×; (b) %.1f ms, %.2f ×; kernels: draws and pulses %.2f, segments %.1f, verify %.2f ms "
            "(the single track's: %.2f ms); %d repaired.  Bytes and end states of every track equal (a)'s" % (cell(h) + cell(s)),
            "`profiles/audio_tracks.json`, DESIGN.md §7l")


def audio_mixed_row(path="profiles/audio_mixed_tracks.json"):
    """The row of audio tracks with parameters per track, from tools/bench_audio_mixed.py's file."""
    j = json.load(open(path))
    m, a_, b = j["mixed_call"], j["a_one_bind_and_tracks_call_per_set"], j["b_all_tracks_on_one_set"]
    km = m["kernel_ms"]
    return ("audio tracks with parameters per track in one call (`ntscsim_audio_mixed_tracks_device`): %d independent tracks of %g s resident in HBM over %d sets "
            "(stereo Hi-Fi, stereo linear, mono SP, mono LP), each with its own state on the device (`tools/bench_audio_mixed.py`); (a) the same tracks as one "
            "`ntscsim_audio_bind` + `ntscsim_audio_tracks_device` per set, wall clock; (b) %d tracks all on one set (stereo Hi-Fi) through the mixed call and "
            "through `ntscsim_audio_tracks_device`; all in the same run" % (j["tracks"], j["frames_per_track"] / j["rate"], len(j["sets"]), j["tracks"]),
            "**%.1f ms** (%.0f × real time); kernels: draws and pulses %.2f, segments %.1f, verify %.2f ms; %d of %d segments repaired; (a) %.1f ms, %.2f × the "
            "mixed call; (b) mixed call %.1f ms (segments %.1f ms), tracks call %.1f ms (segments %.1f ms): %.3f ×, %d and %d repaired.  Bytes and end states of every "
            "track equal (a)'s, and in (b) each other's" % (
                m["ms"], j["times_real_time"], km["draws_and_pulses"], km["k_audio_mixed_segments"], km["k_audio_mixed_verify"], m["repaired"], m["segments"],
                a_["ms"], j["a_over_mixed"], b["mixed_call"]["ms"], b["mixed_call"]["kernel_ms"]["k_audio_mixed_segments"], b["tracks_call"]["ms"],
                b["tracks_call"]["kernel_ms"]["k_audio_track_segments"], b["mixed_over_tracks"], b["mixed_call"]["repaired"], b["tracks_call"]["repaired"]),
            "`profiles/audio_mixed_tracks.json`, DESIGN.md §7l")


def cass_tracks_row(path="profiles/cass_tracks.json"):
    """The row of many cassette tracks in one call, from tools/bench_cass_tracks.py's file."""
    j = json.load(open(path))
    c = j["cases"]

    def cell(x):
        t, b = x["tracks_call"], x["b_single_track_of_the_total_length"]
        return (t["ms"], x["times_real_time"], x["a_one_call_per_track"]["ms"], x["a_over_tracks"], b["ms"], x["tracks_over_b"])

    t8, b8 = c["taps8"]["tracks_call"], c["taps8"]["b_single_track_of_the_total_length"]
    d8 = c["taps8_deemph"]["tracks_call"]
    km, kd = t8["kernel_ms"], d8["kernel_ms"]
    return ("many cassette tracks in one call (`ntscsim_cass_tracks_device`): %d independent stereo tracks of %g s resident in HBM, all from sample count 0, each with "
            "its own state and FIR history on the device (`tools/bench_cass_tracks.py`); (a) the same tracks as one `ntscsim_cass_device` call each with `set_state` / "
            "`get_state` between them, wall clock; (b) one `ntscsim_cass_device` call over a single track of the same total length; all in the same run"
            % (j["tracks"], j["frames_per_track"] / j["rate"]),
            "8 taps: **%.1f ms** (%.0f × real time); (a) %.0f ms, so the one call is worth **%.1f ×**; (b) %.1f ms, the tracks call takes %.2f × that.  "
            "With de-emphasis: %.1f ms (%.0f ×); (a) %.0f ms, %.1f ×; (b) %.1f ms, %.2f ×.  57 taps: %.1f ms (%.0f ×); (a) %.0f ms, %.1f ×; (b) %.1f ms, %.2f ×; "
            "with de-emphasis %.1f ms (%.0f ×); (a) %.0f ms, %.1f ×; (b) %.1f ms, %.2f ×.  Kernels at 8 taps: draws %.2f, front %.1f, its verify %.2f, FIR %.2f ms, "
            "back %.2f + %.2f with de-emphasis; host `sin()` fill %.2f ms for %d sines (the union of the tracks' counts: one track's), against %.1f ms for the %d of (b); "
            "%d + %d segments repaired.  Bytes and end states of every track equal (a)'s"
            % (cell(c["taps8"]) + cell(c["taps8_deemph"]) + cell(c["taps57"]) + cell(c["taps57_deemph"]) +
               (km["k_audio_hiss"], km["k_cass_track_front"], km["k_cass_track_front_verify"], km["k_cass_track_conv"], kd["k_cass_track_back"],
                kd["k_cass_track_back_verify"], km["host_sin_fill"], t8["tilt_frames"], b8["kernel_ms"]["host_sin_fill"], b8["tilt_frames"],
                d8["repaired_front"], d8["repaired_back"])),
            "`profiles/cass_tracks.json`, DESIGN.md §7m")


def cass_mixed_row(path="profiles/cass_mixed_tracks.json"):
    """The row of cassette tracks with parameters per track, from tools/bench_cass_mixed.py's file."""
    j = json.load(open(path))
    m, a_, b = j["mixed_call"], j["a_one_bind_and_tracks_call_per_set"], j["b_all_tracks_on_one_set"]
    km = m["kernel_ms"]
    return ("cassette tracks with parameters per track in one call (`ntscsim_cass_mixed_tracks_device`): %d independent stereo tracks of %g s resident in HBM over "
            "%d sets (default, `-preset 3`, both emphasis filters, mono at `-high 100`; %s taps), all from sample count 0, each with its own state on the device "
            "(`tools/bench_cass_mixed.py`); (a) the same tracks as one `ntscsim_cass_bind` + `ntscsim_cass_tracks_device` per set, wall clock; (b) %d tracks all "
            "on one set (default) through the mixed call and through `ntscsim_cass_tracks_device`; all in the same run"
            % (j["tracks"], j["frames_per_track"] / j["rate"], len(j["sets"]), " / ".join(str(t) for t in j["taps"]), b["tracks"]),
            "**%.1f ms** (%.0f × real time); kernels: draws %.2f, front %.1f, its verify %.2f, FIR %.2f, back %.2f + %.2f ms; host `sin()` fill %.2f ms for %d sines "
            "(one tape's, shared by the four decks); %d + %d of %d segments repaired; (a) %.1f ms, %.2f × the mixed call; (b) mixed call %.1f ms (front %.1f ms), "
            "tracks call %.1f ms (front %.1f ms): %.3f ×.  Bytes and end states of every track equal (a)'s, and in (b) each other's" % (
                m["ms"], j["times_real_time"], km["k_audio_hiss"], km["k_cass_mixed_front"], km["k_cass_mixed_front_verify"], km["k_cass_mixed_conv"],
                km["k_cass_mixed_back"], km["k_cass_mixed_back_verify"], km["host_sin_fill"], m["tilt_frames"], m["repaired_front"], m["repaired_back"],
                m["segments"], a_["ms"], j["a_over_mixed"], b["mixed_call"]["ms"], b["mixed_call"]["kernel_ms"]["k_cass_mixed_front"], b["tracks_call"]["ms"],
                b["tracks_call"]["kernel_ms"]["k_cass_track_front"], b["mixed_over_tracks"]),
            "`profiles/cass_mixed_tracks.json`, DESIGN.md §7m")


def mixed_fields_row(path="profiles/mixed_fields.json"):
    """The row of fields with parameters per field, from tools/bench_mixed_fields.py's file ("unmeasured" without one)."""
    what = ("fields with parameters per field in one call (`ntscsim_mixed_fields_device`), resident in HBM (`tools/bench_mixed_fields.py`); (a) one frame "
            "per set, against the same fields as one `ntscsim_fields_device` call per set on one context per set, wall clock; (b) all fields on one set "
            "(`-vhs`) through the mixed call, through `ntscsim_fields_device` with the generic kernels forced and with its hand-tuned kernels; all in the same run")
    try:
        j = json.load(open(path))
    except OSError:
        return (what, "**unmeasured**: no GPU run of `tools/bench_mixed_fields.py` was taken on this build", "DESIGN.md §3c")
    a, p, b = j["a_mixed_call"], j["a_one_call_per_set"], j["b_all_fields_on_one_set"]
    return (what,
            "(a) %d fields over %d sets: **%.2f ms** (%.0f fields/s); one call per set %.1f ms, so the one call is worth **%.1f ×**; (b) %d fields on one set: mixed "
            "call %.3f ms, generic single-set kernels %.3f ms (%.3f ×), hand-tuned %.3f ms (the mixed call takes %.2f × that).  Whole destination buffers equal "
            "in (a) and in (b)" % (j["fields"], j["sets"], a["ms"], j["a_fields_per_s"], p["ms"], j["a_per_set_over_mixed"], j["fields"], b["mixed_call"]["ms"],
                                 b["generic_single_set"]["ms"], b["mixed_over_generic"], b["hand_tuned_single_set"]["ms"], b["mixed_over_hand_tuned"]),
            "`profiles/mixed_fields.json`, DESIGN.md §3c")


def mixed_fields_tuned_row(path="profiles/mixed_fields_tuned.json"):
    """The row of the mixed call on the hand-tuned kernels (ntscsim_set_mixed_forms), from the same tool's file."""
    what = ("the same call with `ntscsim_set_mixed_forms(NTSCSIM_MIXED_TUNED)` (off by default): sets of the default / `-vhs` preset families on the "
            "hand-tuned kernels, every other set on the generic ones, in the one call; against the generic mixed call and, in (b), against the single-set "
            "hand-tuned call; (b′) the fields of (b) over four sets; all in the same run")
    try:
        j = json.load(open(path))
    except OSError:
        return (what, "**unmeasured**: no GPU run of `tools/bench_mixed_fields.py` was taken on this build", "DESIGN.md §3c")
    a, at, b, s = j["a_mixed_call"], j["a_tuned_mixed_call"], j["b_all_fields_on_one_set"], j["b_split_over_four_sets"]
    s1, s2 = s["four_noise_levels_sp"], s["sp_lp_ep_svideo"]
    txt = ("(a) %d fields over %d sets: tuned **%.2f ms**, generic %.2f ms (**%.2f ×**); (b) %d fields on one set: tuned %.3f ms, generic mixed %.3f ms "
           "(**%.2f ×**), single-set hand-tuned %.3f ms (the tuned call takes %.2f × that); (b′) SP at four noise levels: tuned %.3f ms, generic %.3f ms "
           "(%.2f ×); SP / LP / EP / S-Video: tuned %.3f ms, generic %.3f ms (%.2f ×).  Every tuned call wrote the bytes of its generic twin"
           % (j["fields"], j["sets"], at["ms"], a["ms"], j["a_generic_over_tuned"], j["fields"], b["tuned_mixed_call"]["ms"], b["mixed_call"]["ms"],
              b["generic_over_tuned"], b["hand_tuned_single_set"]["ms"], b["tuned_over_hand_tuned"], s1["tuned_mixed_call"]["ms"], s1["mixed_call"]["ms"],
              s1["generic_over_tuned"], s2["tuned_mixed_call"]["ms"], s2["mixed_call"]["ms"], s2["generic_over_tuned"]))
    c = j.get("parent_against_this")
    if c:
        cp, ct = c["c_bench_py_fields_per_s"]["parent"], c["c_bench_py_fields_per_s"]["this"]
        txt += ("; `bench.py`, %d rounds of fresh processes: parent %.0f-%.0f, this commit %.0f-%.0f fields/s" % (c["rounds"], min(cp), max(cp), min(ct), max(ct)))
    return (what, txt, "`profiles/mixed_fields_tuned.json`, DESIGN.md §3c")


def mixed_fields422_row(path="profiles/mixed_fields422.json"):
    """The row of YUV422P fields with parameters per field, from tools/bench_mixed_fields422.py's file ("unmeasured" without one)."""
    what = ("YUV422P fields with parameters per field in one call (`ntscsim_mixed_fields422_device`), 720×480, resident in HBM "
            "(`tools/bench_mixed_fields422.py`); (a) one frame per set, against the same fields as one `ntscsim_fields422_device` call per set on one context "
            "per set, wall clock; (b) all fields on one set (`-vhs`) through the mixed call, through `ntscsim_fields422_device` on `k422_process` and on its "
            "streamed kernel; (c) the single-set `k422_process` of the parent commit and of this one, fresh processes; all in the same run")
    try:
        j = json.load(open(path))
    except OSError:
        return (what, "**unmeasured**: no GPU run of `tools/bench_mixed_fields422.py` was taken on this build", "DESIGN.md §7a")
    a, p, b, c = j["a_mixed_call"], j["a_one_call_per_set"], j["b_all_fields_on_one_set"], j.get("parent_against_this")
    host = ""
    if "wall" in a:
        host = (" (device events; %.2f ms on the wall clock, of which the host side of the call takes %.2f ms: %.1f × on the same clock)"
                % (a["wall"]["ms"], a["host_ms_of_the_call"], j["a_per_set_over_mixed_wall"]))
    txt = ("(a) %d fields over %d sets: **%.2f ms** (%.0f fields/s); one call per set %.1f ms, so the one call is worth **%.1f ×**%s; (b) %d fields on one set: "
           "mixed call %.3f ms, `k422_process` %.3f ms (%.3f ×), streamed kernel %.3f ms (the mixed call takes %.2f × that).  Whole destination buffers equal "
           "in (a) and in (b)" % (j["fields"], j["sets"], a["ms"], j["a_fields_per_s"], p["ms"], j["a_per_set_over_mixed"], host, j["fields"], b["mixed_call"]["ms"],
                                b["k422_process_single_set"]["ms"], b["mixed_over_k422_process"], b["streamed_single_set"]["ms"], b["mixed_over_streamed"]))
    if c:
        txt += ("; (c) `k422_process`, %d rounds: parent %.3f-%.3f ms, this commit %.3f-%.3f ms"
                % (c["rounds"], c["parent_range_ms"][0], c["parent_range_ms"][1], c["this_range_ms"][0], c["this_range_ms"][1]))
    return (what, txt, "`profiles/mixed_fields422.json`, DESIGN.md §7a")


for row in (led_row, filmac_row, audio_tracks_row, audio_mixed_row, cass_tracks_row, cass_mixed_row, mixed_fields_row, mixed_fields_tuned_row, mixed_fields422_row):
    try:
        rows.append(row())
    except Exception:
        pass
try:
    rows.extend(pixmap_rows())
except Exception:
    pass
tbl = "| what (1× MI355X, 720×486 unless said otherwise) | measured | where |\n|---|---|---|\n" + "\n".join("| %s | %s | %s |" % r for r in rows)
s = open("README.md").read()
a, b = s.index("<!-- numbers:begin -->"), s.index("<!-- numbers:end -->")
s = s[:a] + "<!-- numbers:begin -->\n" + tbl + "\n" + s[b:]
open("README.md", "w").write(s)
print(tbl)
