"""ctypes binding of include/ntscsim.h (the product C-ABI, libntscsim.so).

The shared object loads without a GPU (so the CPU test-suite can check the exported symbols and
use the host-side parse_argv mirror); ntscsim_create() then fails with NTSCSIM_E_NODEV.  There is
no CPU fallback anywhere in this package.
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# NTSCSIM_LIB: developer override (A/B builds of the same ABI); default = the in-tree library
PRODUCT_SO = os.environ.get("NTSCSIM_LIB") or os.path.join(PKG_DIR, "libntscsim.so")

OK, E_ARG, E_SIZE, E_NODEV, E_HIP, E_NOMEM, E_PARAM, E_FLAG, E_HELP, E_INTERNAL = \
    0, -1, -2, -3, -4, -5, -6, -7, -8, -9
RNG_AUTO = 0xFFFFFFFFFFFFFFFF
MODE_EXACT, MODE_FAST32, MODE_FLOAT = 0, 1, 2
DESC_INTERLACED, DESC_TFF, DESC_BOB = 1, 2, 0x100
SUBMIT_SAME_SRC, SUBMIT_SRC_STABLE = 0x10000, 0x20000
TICKET_ALL = 0xFFFFFFFFFFFFFFFF

# every symbol include/ntscsim.h declares
EXPORTS = (
    "ntscsim_params_init", "ntscsim_cli_init", "ntscsim_params_parse_argv",
    "ntscsim_params_validate", "ntscsim_rng_calls_per_field", "ntscsim_rng_draw",
    "ntscsim_create", "ntscsim_destroy", "ntscsim_strerror", "ntscsim_last_error",
    "ntscsim_set_mode", "ntscsim_get_rng_pos", "ntscsim_set_rng_pos", "ntscsim_field", "ntscsim_frames_host",
    "ntscsim_fields_device", "ntscsim_mixed_fields_device", "ntscsim_mixed_fields422_device",
    "ntscsim_batch_create", "ntscsim_batch_run", "ntscsim_batch_destroy",
    "ntscsim_sync", "ntscsim_set_profiling", "ntscsim_get_timings_ms", "ntscsim_set_launch_form",
    "ntscsim_set_mixed_forms", "ntscsim_debug_mixed_form_of",
    "ntscsim_debug_read_composite", "ntscsim_debug_set_warmup",
    "ntscsim_debug_force_generic", "ntscsim_debug_no_fast_decode", "ntscsim_debug_last_kernels", "ntscsim_debug_last_decoder_lds", "ntscsim_debug_fast_plane_ok", "ntscsim_debug_field_stats", "ntscsim_debug_mixed_tables",
    "ntscsim_params_init_to_composite", "ntscsim_params_parse_argv_to_composite",
    "ntscsim_fields422_device", "ntscsim_output422_device", "ntscsim_bgra_to_yuv_device", "ntscsim_rng_calls_per_field_422",
    "ntscsim_scale_to_bgra_device", "ntscsim_frames_host_scaled",
    "ntscsim_batch422_create", "ntscsim_batch422_run", "ntscsim_batch422_destroy",
    "ntscsim_raw28_opts_init", "ntscsim_raw28_parse_argv", "ntscsim_raw28_geometry", "ntscsim_raw28_create",
    "ntscsim_raw28_destroy", "ntscsim_raw28_last_error", "ntscsim_raw28_decode", "ntscsim_raw28_decode_device",
    "ntscsim_raw28_stream_reset", "ntscsim_raw28_stream_push",
    "ntscsim_raw28_get_levels", "ntscsim_raw28_debug_set_speculation", "ntscsim_raw28_debug_stats", "ntscsim_raw28_debug_pick_chunk",
    "ntscsim_raw28_debug_read_front",
    "ntscsim_submit_opts_init", "ntscsim_submit_configure", "ntscsim_submit", "ntscsim_flush", "ntscsim_wait",
    "ntscsim_host_unpin", "ntscsim_submit_stats",
    "ntscsim_host_pin", "ntscsim_host_alloc", "ntscsim_host_free", "ntscsim_host_frame_alloc", "ntscsim_set_pin_policy",
    "ntscsim_field422", "ntscsim_submit422", "ntscsim_submit422_configure", "ntscsim_submit422_stats",
    "ntscsim_pool_create", "ntscsim_pool_destroy", "ntscsim_pool_size", "ntscsim_pool_ctx", "ntscsim_pool_set_block",
    "ntscsim_pool_get_rng_pos", "ntscsim_pool_set_rng_pos", "ntscsim_pool_last_error", "ntscsim_pool_frames_host",
    "ntscsim_blend_params_init", "ntscsim_blend_parse_argv", "ntscsim_blend_frame_time",
    "ntscsim_blend_plan_create", "ntscsim_blend_plan_push", "ntscsim_blend_plan_next", "ntscsim_blend_plan_reset",
    "ntscsim_blend_plan_destroy", "ntscsim_blend_clip_periods", "ntscsim_blend_tables", "ntscsim_blend_bind",
    "ntscsim_blend_frames_device", "ntscsim_blend_clip_device", "ntscsim_blend_frames_host",
    "ntscsim_key_params_init", "ntscsim_key_params_free", "ntscsim_key_params_add_layer", "ntscsim_key_parse_argv",
    "ntscsim_key_rand_advance", "ntscsim_key_bind", "ntscsim_key_frames_device", "ntscsim_key_clip_device",
    "ntscsim_key_frames_host", "ntscsim_key_debug_lane_state", "ntscsim_key_debug_set_bits_limit",
    "ntscsim_avg_params_init", "ntscsim_avg_params_free", "ntscsim_avg_params_add_layer", "ntscsim_avg_parse_argv",
    "ntscsim_avg_bind", "ntscsim_avg_frames_device", "ntscsim_avg_clip_device", "ntscsim_avg_frames_host",
    "ntscsim_scan_params_init", "ntscsim_scan_parse_argv", "ntscsim_scan_effect", "ntscsim_scan_field_of",
    "ntscsim_scan_bind", "ntscsim_scan_frames_device", "ntscsim_scan_clip_device", "ntscsim_scan_frames_host",
    "ntscsim_scan_debug_keep_raster", "ntscsim_scan_debug_raster", "ntscsim_scan_debug_set_window_rows",
    "ntscsim_scan_debug_spill",
    "ntscsim_led_params_init", "ntscsim_led_parse_argv", "ntscsim_led_bind", "ntscsim_led_frames_device",
    "ntscsim_led_frames_host", "ntscsim_led_debug_keep_edges", "ntscsim_led_debug_edges",
    "ntscsim_filmac_params_init", "ntscsim_filmac_parse_argv", "ntscsim_filmac_bind", "ntscsim_filmac_frames_device",
    "ntscsim_filmac_frames_host", "ntscsim_filmac_reset", "ntscsim_filmac_get_state", "ntscsim_filmac_set_state",
    "ntscsim_filmac_debug_levels", "ntscsim_filmac_debug_time_kernels", "ntscsim_filmac_debug_kernel_ms",
    "ntscsim_pixmap_params_init", "ntscsim_pixmap_params_free", "ntscsim_pixmap_parse_argv",
    "ntscsim_post_params_init", "ntscsim_post_params_free", "ntscsim_post_parse_argv", "ntscsim_post_bind",
    "ntscsim_post_frames_device", "ntscsim_post_frames_host",
    "ntscsim_cmap_params_init", "ntscsim_cmap_params_free", "ntscsim_cmap_parse_argv", "ntscsim_cmap_bind",
    "ntscsim_cmap_frames_device", "ntscsim_cmap_frames_host", "ntscsim_cmap_reset", "ntscsim_cmap_get_table",
    "ntscsim_cmap_set_table",
    "ntscsim_audio_params_from_cli", "ntscsim_audio_bind", "ntscsim_audio_device", "ntscsim_audio_host", "ntscsim_audio_reset",
    "ntscsim_audio_get_state", "ntscsim_audio_set_state", "ntscsim_audio_debug_set_plan", "ntscsim_audio_debug_stats",
    "ntscsim_audio_debug_pulses", "ntscsim_audio_debug_time_kernels", "ntscsim_audio_debug_kernel_ms",
    "ntscsim_audio_tracks_device", "ntscsim_audio_debug_track_stats",
    "ntscsim_audio_mixed_tracks_device", "ntscsim_audio_mixed_tracks_host",
    "ntscsim_cass_params_init", "ntscsim_cass_parse_argv", "ntscsim_cass_params_derive", "ntscsim_cass_bind", "ntscsim_cass_device",
    "ntscsim_cass_host", "ntscsim_cass_reset", "ntscsim_cass_get_state", "ntscsim_cass_set_state", "ntscsim_cass_debug_set_plan",
    "ntscsim_cass_debug_stats", "ntscsim_cass_debug_time_kernels", "ntscsim_cass_debug_kernel_ms",
    "ntscsim_cass_tracks_device", "ntscsim_cass_debug_track_stats", "ntscsim_cass_debug_tilt_frames",
    "ntscsim_cass_mixed_tracks_device", "ntscsim_cass_mixed_tracks_host",
)


class SubmitOpts(C.Structure):
    """struct ntscsim_submit_opts -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("struct_size", C.c_uint32), ("depth", C.c_int32), ("slots", C.c_int32), ("lanes", C.c_int32),
                ("pin_caller_buffers", C.c_int32), ("_pad", C.c_int32), ("min_pin_bytes", C.c_size_t)]


class Frame422(C.Structure):
    """struct ntscsim_frame422 -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("data", C.c_void_p * 3), ("linesize", C.c_int32 * 3), ("_pad", C.c_int32)]


class Loop422(C.Structure):
    """struct ntscsim_loop422 -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("src_height", C.c_int32),
                ("frame", Frame422), ("src", Frame422), ("filter", Frame422), ("out", Frame422),
                ("field", C.c_uint32), ("flags", C.c_uint32), ("out_mode", C.c_uint32), ("out_field", C.c_uint32),
                ("fieldno", C.c_uint64)]


SUBMIT422_DIRTY = 0x40000


class Raw28Opts(C.Structure):
    """struct ntscsim_raw28_opts -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("struct_size", C.c_uint32), ("_pad0", C.c_uint32), ("sample_rate", C.c_double),
                ("mark_sync", C.c_int32), ("disable_sync", C.c_int32), ("disable_wp_equ", C.c_int32),
                ("show_subcarrier", C.c_int32), ("disable_subcarrier", C.c_int32),
                ("disable_equalization", C.c_int32)]


class Params(C.Structure):
    """struct ntscsim_params -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("tv_standard", C.c_int32),
        ("output_width", C.c_int32),
        ("output_height", C.c_int32),
        ("video_scanline_phase_shift", C.c_int32),
        ("video_scanline_phase_shift_offset", C.c_int32),
        ("composite_preemphasis", C.c_double),
        ("composite_preemphasis_cut", C.c_double),
        ("vhs_out_sharpen", C.c_double),
        ("vhs_head_switching", C.c_int32),
        ("_pad0", C.c_int32),
        ("vhs_head_switching_point", C.c_double),
        ("vhs_head_switching_phase", C.c_double),
        ("vhs_head_switching_phase_noise", C.c_double),
        ("composite_in_chroma_lowpass", C.c_int32),
        ("composite_out_chroma_lowpass", C.c_int32),
        ("composite_out_chroma_lowpass_lite", C.c_int32),
        ("video_yc_recombine", C.c_int32),
        ("video_chroma_noise", C.c_int32),
        ("video_chroma_phase_noise", C.c_int32),
        ("video_chroma_loss", C.c_int32),
        ("video_noise", C.c_int32),
        ("subcarrier_amplitude", C.c_int32),
        ("subcarrier_amplitude_back", C.c_int32),
        ("emulating_vhs", C.c_int32),
        ("nocolor_subcarrier", C.c_int32),
        ("nocolor_subcarrier_after_yc_sep", C.c_int32),
        ("vhs_chroma_vert_blend", C.c_int32),
        ("vhs_svideo_out", C.c_int32),
        ("enable_composite_emulation", C.c_int32),
        ("output_vhs_tape_speed", C.c_int32),
        ("black_key_level_feedback", C.c_int32),
        ("vhs_out_sharpen_chroma", C.c_double),
        ("ghost_taps", C.c_int32),
        ("ghost_delay", C.c_int32 * 4),
        ("ghost_gain", C.c_int32 * 4),
        ("_pad1", C.c_int32),
    ]


class FieldDesc(C.Structure):
    """struct ntscsim_field_desc"""
    _fields_ = [
        ("src_dev", C.c_void_p),
        ("dst_dev", C.c_void_p),
        ("src_linesize", C.c_int32),
        ("dst_linesize", C.c_int32),
        ("field", C.c_uint32),
        ("flags", C.c_uint32),
        ("fieldno", C.c_uint64),
        ("rng_pos", C.c_uint64),
    ]


class MixedFieldDesc(C.Structure):
    """struct ntscsim_mixed_field_desc"""
    _fields_ = [
        ("d", FieldDesc),
        ("set", C.c_int32),
        ("_pad", C.c_int32),
    ]


class Field422Desc(C.Structure):
    """struct ntscsim_field422_desc"""
    _fields_ = [
        ("dst_dev", C.c_void_p * 3),
        ("src_dev", C.c_void_p * 3),
        ("flt_dev", C.c_void_p * 3),
        ("dst_linesize", C.c_int32 * 3),
        ("src_linesize", C.c_int32 * 3),
        ("flt_linesize", C.c_int32 * 3),
        ("src_height", C.c_int32),
        ("field", C.c_uint32),
        ("flags", C.c_uint32),
        ("_pad", C.c_uint32),
        ("fieldno", C.c_uint64),
        ("rng_pos", C.c_uint64),
    ]


class MixedField422Desc(C.Structure):
    """struct ntscsim_mixed_field422_desc"""
    _fields_ = [
        ("d", Field422Desc),
        ("set", C.c_int32),
        ("_pad", C.c_int32),
    ]


F422_INTERLACED, F422_TFF, F422_SRC420, F422_SECOND, F422_NOCOMP = 1, 2, 4, 8, 16


class Out422Desc(C.Structure):
    """struct ntscsim_out422_desc"""
    _fields_ = [
        ("frame_dev", C.c_void_p * 3),
        ("bob_dev", C.c_void_p * 3),
        ("frame_linesize", C.c_int32 * 3),
        ("bob_linesize", C.c_int32 * 3),
        ("field", C.c_uint32),
        ("mode", C.c_uint32),
    ]


OUT422_BOB422, OUT422_BOB420, OUT422_INTERLACED420, OUT422_FRAME = 0, 1, 2, 3


class YuvDesc(C.Structure):
    """struct ntscsim_yuv_desc"""
    _fields_ = [
        ("bgra_dev", C.c_void_p),
        ("yuv_dev", C.c_void_p * 3),
        ("bgra_linesize", C.c_int32),
        ("yuv_linesize", C.c_int32 * 3),
    ]


PIX_YUV420P, PIX_YUV422P = 0, 1
HOST_YUV420P, HOST_YUV422P = 0x1000, 0x2000
SRC_BGRA, SRC_YUV420P, SRC_YUV422P = 0, 1, 2


class ScaleDesc(C.Structure):
    """struct ntscsim_scale_desc"""
    _fields_ = [
        ("src_dev", C.c_void_p * 3),
        ("bgra_dev", C.c_void_p),
        ("src_linesize", C.c_int32 * 3),
        ("bgra_linesize", C.c_int32),
        ("src_width", C.c_int32),
        ("src_height", C.c_int32),
        ("src_format", C.c_int32),
        ("_pad", C.c_int32),
    ]


class HostSource(C.Structure):
    """struct ntscsim_host_source"""
    _fields_ = [
        ("format", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("linesize", C.c_int32 * 3),
        ("plane_offset", C.c_size_t * 3),
        ("frame_bytes", C.c_size_t),
    ]


class BlendParams(C.Structure):
    """struct ntscsim_blend_params -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("struct_size", C.c_uint32), ("rate_num", C.c_int32), ("rate_den", C.c_int32),
                ("output_width", C.c_int32), ("output_height", C.c_int32), ("squelch_near_match", C.c_int32),
                ("fullframealt", C.c_int32), ("framealt", C.c_int32), ("gamma_correction", C.c_double),
                ("underscan", C.c_int32), ("use_422_colorspace", C.c_int32), ("n_inputs", C.c_int32), ("_pad", C.c_int32),
                ("input_path", C.c_char_p), ("output_path", C.c_char_p)]


class BlendTap(C.Structure):
    """struct ntscsim_blend_tap"""
    _fields_ = [("src_dev", C.c_void_p), ("src_linesize", C.c_int32), ("weight16", C.c_uint32)]


class BlendDesc(C.Structure):
    """struct ntscsim_blend_desc"""
    _fields_ = [("dst_dev", C.c_void_p), ("dst_linesize", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("n_taps", C.c_int32), ("taps", C.POINTER(BlendTap))]


BLEND_FAST_TAPS = 4


class KeyLayer(C.Structure):
    """struct ntscsim_key_layer -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("color", C.c_uint32), ("threshhold", C.c_int32), ("fade", C.c_uint32), ("xdivr", C.c_uint32),
                ("invert", C.c_int32), ("noisekey", C.c_uint32), ("path", C.c_char_p)]


class KeyParams(C.Structure):
    """struct ntscsim_key_params"""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("tv_standard", C.c_int32),
                ("delay", C.c_int32), ("use_422_colorspace", C.c_int32), ("n_layers", C.c_int32), ("layers_cap", C.c_int32),
                ("layers", C.POINTER(KeyLayer)), ("output_path", C.c_char_p)]

    def __del__(self):                      # the layer list is a heap block of the library's
        try:
            if _lib is not None and self.layers:
                _lib.ntscsim_key_params_free(C.byref(self))
        except Exception:
            pass


class KeySrc(C.Structure):
    """struct ntscsim_key_src"""
    _fields_ = [("src_dev", C.c_void_p), ("src_linesize", C.c_int32), ("_pad", C.c_int32)]


class KeyDesc(C.Structure):
    """struct ntscsim_key_desc"""
    _fields_ = [("dst_dev", C.c_void_p), ("dst_linesize", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("n_layers", C.c_int32), ("layers", C.POINTER(KeySrc)), ("rand_pos", C.c_uint64)]


KEY_FAST_LAYERS = 4


class AvgLayer(C.Structure):
    """struct ntscsim_avg_layer -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("newlevel", C.c_int32), ("path", C.c_char_p)]


class AvgParams(C.Structure):
    """struct ntscsim_avg_params"""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("tv_standard", C.c_int32),
                ("delay", C.c_int32), ("use_422_colorspace", C.c_int32), ("n_layers", C.c_int32), ("layers_cap", C.c_int32),
                ("layers", C.POINTER(AvgLayer)), ("output_path", C.c_char_p)]

    def __del__(self):                      # the layer list is a heap block of the library's
        try:
            if _lib is not None and self.layers:
                _lib.ntscsim_avg_params_free(C.byref(self))
        except Exception:
            pass


class AvgSrc(C.Structure):
    """struct ntscsim_avg_src"""
    _fields_ = [("src_dev", C.c_void_p), ("src_linesize", C.c_int32), ("_pad", C.c_int32)]


class AvgDesc(C.Structure):
    """struct ntscsim_avg_desc"""
    _fields_ = [("dst_dev", C.c_void_p), ("dst_linesize", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("n_layers", C.c_int32), ("layers", C.POINTER(AvgSrc)), ("field", C.c_uint64)]


AVG_FAST_LAYERS = 4


class ScanParams(C.Structure):
    """struct ntscsim_scan_params -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("struct_size", C.c_uint32), ("output_width", C.c_int32), ("output_height", C.c_int32),
                ("tv_standard", C.c_int32), ("field_rate_num", C.c_int32), ("field_rate_den", C.c_int32),
                ("input_ntsc", C.c_int32), ("output_pal", C.c_int32), ("use_422_colorspace", C.c_int32),
                ("n_inputs", C.c_int32), ("src_width", C.c_int32), ("src_height", C.c_int32), ("_pad", C.c_int32),
                ("last_input_path", C.c_char_p), ("output_path", C.c_char_p)]


class ScanDesc(C.Structure):
    """struct ntscsim_scan_desc"""
    _fields_ = [("dst_dev", C.c_void_p), ("dst_linesize", C.c_int32), ("src_linesize", C.c_int32),
                ("src_dev", C.c_void_p), ("src_width", C.c_int32), ("src_height", C.c_int32), ("fieldno", C.c_uint64)]


class LedParams(C.Structure):
    """struct ntscsim_led_params -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("underscan", C.c_int32),
                ("use_422_colorspace", C.c_int32), ("field_rate_num", C.c_int32), ("field_rate_den", C.c_int32),
                ("_pad", C.c_int32), ("gamma_correction", C.c_double), ("input_path", C.c_char_p),
                ("output_path", C.c_char_p)]


class LedDesc(C.Structure):
    """struct ntscsim_led_desc"""
    _fields_ = [("src_dev", C.c_void_p), ("src_linesize", C.c_int32), ("dst_linesize", C.c_int32),
                ("dst_dev", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


FilmacParams = LedParams                   # typedef ntscsim_led_params ntscsim_filmac_params


class FilmacDesc(C.Structure):
    """struct ntscsim_filmac_desc"""
    _fields_ = [("src", C.c_void_p), ("src_linesize", C.c_int32), ("_pad0", C.c_int32),
                ("dst", C.c_void_p), ("dst_linesize", C.c_int32), ("_pad1", C.c_int32)]


class FilmacState(C.Structure):
    """struct ntscsim_filmac_state"""
    _fields_ = [("init", C.c_int32), ("_pad", C.c_int32), ("final_minv", C.c_int64), ("final_maxv", C.c_int64)]


class PixmapLayer(C.Structure):
    """struct ntscsim_pixmap_layer"""
    _fields_ = [("path", C.c_char_p), ("threshhold", C.c_int32), ("_pad", C.c_int32)]


class PixmapParams(C.Structure):
    """struct ntscsim_pixmap_params: the switches of ffmpeg_posterize and of ffmpeg_colormap"""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("use_422_colorspace", C.c_int32),
                ("field_rate_num", C.c_int32), ("field_rate_den", C.c_int32), ("output_pal", C.c_int32),
                ("n_layers", C.c_int32), ("layers_cap", C.c_int32), ("_pad", C.c_int32),
                ("layers", C.POINTER(PixmapLayer)), ("output_path", C.c_char_p)]

    def __del__(self):                      # the input list is a heap block of the library's
        try:
            if _lib is not None and self.layers:
                _lib.ntscsim_pixmap_params_free(C.byref(self))
        except Exception:
            pass


PostParams = PixmapParams                  # typedef ntscsim_pixmap_params ntscsim_post_params
CmapParams = PixmapParams                  # typedef ntscsim_pixmap_params ntscsim_cmap_params


class PostDesc(C.Structure):
    """struct ntscsim_post_desc"""
    _fields_ = [("src", C.c_void_p), ("src_linesize", C.c_int32), ("_pad0", C.c_int32),
                ("dst", C.c_void_p), ("dst_linesize", C.c_int32), ("layer", C.c_int32)]


class CmapDesc(C.Structure):
    """struct ntscsim_cmap_desc"""
    _fields_ = [("src", C.c_void_p), ("src_linesize", C.c_int32), ("_pad0", C.c_int32),
                ("dst", C.c_void_p), ("dst_linesize", C.c_int32), ("_pad1", C.c_int32),
                ("map", C.c_void_p), ("map_linesize", C.c_int32), ("_pad2", C.c_int32)]


class Cli(C.Structure):
    """struct ntscsim_cli -- keep in lock-step with include/ntscsim.h."""
    _fields_ = [("input_paths", C.c_char_p * 16), ("n_inputs", C.c_int32), ("frame_delay", C.c_int32),
                ("output_path", C.c_char_p), ("use_422_colorspace", C.c_int32),
                ("emulating_preemphasis", C.c_int32), ("emulating_deemphasis", C.c_int32), ("output_vhs_hifi", C.c_int32),
                ("output_audio_hiss_db", C.c_double), ("output_audio_linear_buzz", C.c_double),
                ("vhs_linear_high_boost", C.c_double), ("output_video_as_interlaced", C.c_int32), ("_pad", C.c_int32)]


class AudioParams(C.Structure):
    """struct ntscsim_audio_params"""
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_int32), ("channels", C.c_int32), ("rate", C.c_int32),
                ("passes", C.c_int32), ("hifi", C.c_int32), ("preemphasis", C.c_int32), ("deemphasis", C.c_int32),
                ("hiss_level", C.c_int32), ("tv_standard", C.c_int32), ("vsync_lines", C.c_int32), ("vpulse_end", C.c_int32),
                ("lowpass_hz", C.c_double), ("highpass_hz", C.c_double), ("emphasis_hz", C.c_double), ("boost_hz", C.c_double),
                ("hsync_hz", C.c_double), ("hpulse_end", C.c_double), ("buzz", C.c_double), ("boost_gain", C.c_double),
                ("alpha_lowpass", C.c_double), ("alpha_highpass", C.c_double), ("alpha_pre", C.c_double),
                ("alpha_post", C.c_double), ("alpha_boost", C.c_double)]


class AudioState(C.Structure):
    """struct ntscsim_audio_state"""
    _fields_ = [("bandpass", (C.c_double * 12) * 2), ("pre", C.c_double * 2), ("post", C.c_double * 2),
                ("boost", C.c_double * 2), ("count", C.c_uint64)]


class AudioDesc(C.Structure):
    """struct ntscsim_audio_desc"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("samples", C.c_uint32), ("_pad", C.c_uint32),
                ("rng_pos", C.c_uint64)]


class AudioStats(C.Structure):
    """struct ntscsim_audio_stats"""
    _fields_ = [("segments", C.c_uint64), ("repaired", C.c_uint64)]


class AudioTrack(C.Structure):
    """struct ntscsim_audio_track"""
    _fields_ = [("blocks", C.POINTER(AudioDesc)), ("n_blocks", C.c_int32), ("_pad", C.c_int32), ("state", C.c_void_p)]


class AudioMixedTrack(C.Structure):
    """struct ntscsim_audio_mixed_track"""
    _fields_ = [("blocks", C.POINTER(AudioDesc)), ("n_blocks", C.c_int32), ("set", C.c_int32), ("state", C.c_void_p)]


CASS_MAX_TAPS = 512


class CassParams(C.Structure):
    """struct ntscsim_cass_params"""
    _fields_ = [("struct_size", C.c_uint32), ("channels", C.c_int32), ("rate", C.c_int32), ("passes", C.c_int32),
                ("preemphasis", C.c_int32), ("deemphasis", C.c_int32), ("mono", C.c_int32), ("hiss_level", C.c_int32),
                ("taps", C.c_int32), ("audio_stream_index", C.c_int32),
                ("hiss_db", C.c_double), ("lowpass_hz", C.c_double), ("highpass_hz", C.c_double), ("emphasis_hz", C.c_double),
                ("head_tilt", C.c_double), ("head_tilt_waver", C.c_double),
                ("transcode_start", C.c_double), ("transcode_end", C.c_double), ("transcode_dur", C.c_double),
                ("alpha_lowpass", C.c_double), ("alpha_highpass", C.c_double), ("alpha_pre", C.c_double), ("alpha_post", C.c_double),
                ("input_path", C.c_char_p), ("output_path", C.c_char_p)]


class CassState(C.Structure):
    """struct ntscsim_cass_state"""
    _fields_ = [("bandpass", (C.c_double * 12) * 2), ("pre", C.c_double * 2), ("count", C.c_uint64), ("post", C.c_double * 2),
                ("taps", C.c_uint32), ("_pad", C.c_uint32), ("history", (C.c_double * 2) * (CASS_MAX_TAPS - 1))]


class CassDesc(C.Structure):
    """struct ntscsim_cass_desc"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("samples", C.c_uint32), ("_pad", C.c_uint32),
                ("rng_pos", C.c_uint64)]


class CassStats(C.Structure):
    """struct ntscsim_cass_stats"""
    _fields_ = [("segments", C.c_uint64), ("repaired_front", C.c_uint64), ("repaired_back", C.c_uint64)]


class CassTrack(C.Structure):
    """struct ntscsim_cass_track"""
    _fields_ = [("blocks", C.POINTER(CassDesc)), ("n_blocks", C.c_int32), ("_pad", C.c_int32), ("count", C.c_uint64),
                ("state", C.c_void_p)]


class CassMixedTrack(C.Structure):
    """struct ntscsim_cass_mixed_track"""
    _fields_ = [("blocks", C.POINTER(CassDesc)), ("n_blocks", C.c_int32), ("set", C.c_int32), ("count", C.c_uint64),
                ("state", C.c_void_p)]


_u8p = C.POINTER(C.c_uint8)
_lib = None


def lib():
    """Load libntscsim.so; fail loudly if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(PRODUCT_SO):
        raise RuntimeError(
            "%s is missing -- build it with `python -c \"import __graft_entry__ as g; g.build()\"` "
            "(or `make -C composite-video-simulator_amd/csrc`)" % PRODUCT_SO)
    # Load order: torch carries its own copy of the HIP runtime; imported AFTER libntscsim.so (which links /opt/rocm's)
    # it finds no device.  The package's __init__ (the half that hands torch tensors to this library) therefore imports
    # torch before anything here runs; a program that uses _capi alone and torch later must import torch first itself.
    L = C.CDLL(PRODUCT_SO)
    L.ntscsim_params_init.argtypes = [C.POINTER(Params)]
    L.ntscsim_params_init.restype = None
    L.ntscsim_cli_init.argtypes = [C.c_void_p]
    L.ntscsim_cli_init.restype = None
    L.ntscsim_params_parse_argv.argtypes = [C.POINTER(Params), C.c_void_p, C.c_int,
                                            C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_params_parse_argv.restype = C.c_int
    L.ntscsim_params_validate.argtypes = [C.POINTER(Params)]
    L.ntscsim_params_validate.restype = C.c_int
    L.ntscsim_rng_calls_per_field.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_uint]
    L.ntscsim_rng_calls_per_field.restype = C.c_uint64
    L.ntscsim_rng_draw.argtypes = [C.c_uint64, C.c_size_t, C.POINTER(C.c_uint32)]
    L.ntscsim_rng_draw.restype = None
    L.ntscsim_create.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]
    L.ntscsim_create.restype = C.c_int
    L.ntscsim_destroy.argtypes = [C.c_void_p]
    L.ntscsim_destroy.restype = None
    L.ntscsim_strerror.argtypes = [C.c_int]
    L.ntscsim_strerror.restype = C.c_char_p
    L.ntscsim_last_error.argtypes = [C.c_void_p]
    L.ntscsim_last_error.restype = C.c_char_p
    L.ntscsim_set_mode.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_set_mode.restype = C.c_int
    L.ntscsim_get_rng_pos.argtypes = [C.c_void_p]
    L.ntscsim_get_rng_pos.restype = C.c_uint64
    L.ntscsim_set_rng_pos.argtypes = [C.c_void_p, C.c_uint64]
    L.ntscsim_set_rng_pos.restype = None
    L.ntscsim_field.argtypes = [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, _u8p, C.c_int,
                                C.c_int, C.c_int, C.c_uint, C.c_uint64]
    L.ntscsim_field.restype = C.c_int
    L.ntscsim_frames_host.argtypes = [C.c_void_p, _u8p, C.c_size_t, C.c_int, C.c_int, _u8p,
                                      C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32,
                                      C.c_int]
    L.ntscsim_frames_host.restype = C.c_int
    L.ntscsim_fields_device.argtypes = [C.c_void_p, C.POINTER(FieldDesc), C.c_int, C.c_int,
                                        C.c_int, C.c_void_p]
    L.ntscsim_fields_device.restype = C.c_int
    L.ntscsim_mixed_fields_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int, C.POINTER(MixedFieldDesc), C.c_int,
                                              C.c_int, C.c_int, C.c_void_p]
    L.ntscsim_mixed_fields_device.restype = C.c_int
    L.ntscsim_mixed_fields422_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int, C.POINTER(MixedField422Desc),
                                                 C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ntscsim_mixed_fields422_device.restype = C.c_int
    L.ntscsim_batch_create.argtypes = [C.c_void_p, C.POINTER(FieldDesc), C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p)]
    L.ntscsim_batch_create.restype = C.c_int
    L.ntscsim_batch_run.argtypes = [C.c_void_p, C.c_void_p]
    L.ntscsim_batch_run.restype = C.c_int
    L.ntscsim_batch_destroy.argtypes = [C.c_void_p]
    L.ntscsim_batch_destroy.restype = None
    L.ntscsim_sync.argtypes = [C.c_void_p]
    L.ntscsim_sync.restype = C.c_int
    L.ntscsim_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_set_profiling.restype = None
    L.ntscsim_set_launch_form.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_set_launch_form.restype = C.c_int
    L.ntscsim_set_mixed_forms.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_set_mixed_forms.restype = C.c_int
    L.ntscsim_debug_mixed_form_of.argtypes = [C.POINTER(Params)] + [C.c_int] * 5 + [C.POINTER(C.c_int)] * 2
    L.ntscsim_debug_mixed_form_of.restype = C.c_int
    L.ntscsim_get_timings_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.ntscsim_get_timings_ms.restype = C.c_int
    L.ntscsim_debug_read_composite.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_size_t]
    L.ntscsim_debug_read_composite.restype = C.c_int
    L.ntscsim_debug_set_warmup.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ntscsim_debug_set_warmup.restype = None
    L.ntscsim_params_init_to_composite.argtypes = [C.POINTER(Params)]
    L.ntscsim_params_init_to_composite.restype = None
    L.ntscsim_params_parse_argv_to_composite.argtypes = [C.POINTER(Params), C.c_void_p, C.c_int,
                                                         C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_params_parse_argv_to_composite.restype = C.c_int
    L.ntscsim_fields422_device.argtypes = [C.c_void_p, C.POINTER(Field422Desc), C.c_int, C.c_int,
                                           C.c_int, C.c_void_p]
    L.ntscsim_fields422_device.restype = C.c_int
    L.ntscsim_output422_device.argtypes = [C.c_void_p, C.POINTER(Out422Desc), C.c_int, C.c_int,
                                           C.c_int, C.c_void_p]
    L.ntscsim_output422_device.restype = C.c_int
    L.ntscsim_bgra_to_yuv_device.argtypes = [C.c_void_p, C.POINTER(YuvDesc), C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_void_p]
    L.ntscsim_bgra_to_yuv_device.restype = C.c_int
    L.ntscsim_scale_to_bgra_device.argtypes = [C.c_void_p, C.POINTER(ScaleDesc), C.c_int, C.c_int, C.c_int,
                                               C.c_void_p]
    L.ntscsim_scale_to_bgra_device.restype = C.c_int
    L.ntscsim_frames_host_scaled.argtypes = [C.c_void_p, C.POINTER(HostSource), C.POINTER(C.c_uint8), C.c_size_t,
                                             C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.c_int, C.c_int, C.c_int,
                                             C.c_uint64, C.c_uint32, C.c_int]
    L.ntscsim_frames_host_scaled.restype = C.c_int
    L.ntscsim_rng_calls_per_field_422.argtypes = [C.POINTER(Params), C.c_int, C.c_int, C.c_uint]
    L.ntscsim_rng_calls_per_field_422.restype = C.c_uint64
    L.ntscsim_debug_force_generic.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_debug_force_generic.restype = None
    L.ntscsim_debug_no_fast_decode.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_debug_no_fast_decode.restype = None
    L.ntscsim_debug_last_kernels.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.ntscsim_debug_last_kernels.restype = C.c_int
    L.ntscsim_debug_last_decoder_lds.argtypes = [C.c_void_p]
    L.ntscsim_debug_last_decoder_lds.restype = C.c_int
    L.ntscsim_debug_fast_plane_ok.argtypes = [C.c_int] * 4
    L.ntscsim_debug_fast_plane_ok.restype = C.c_int
    L.ntscsim_debug_field_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.ntscsim_debug_field_stats.restype = None
    L.ntscsim_debug_mixed_tables.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.ntscsim_debug_mixed_tables.restype = None
    L.ntscsim_batch422_create.argtypes = [C.c_void_p, C.POINTER(Field422Desc), C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_void_p)]
    L.ntscsim_batch422_create.restype = C.c_int
    L.ntscsim_batch422_run.argtypes = [C.c_void_p, C.c_void_p]
    L.ntscsim_batch422_run.restype = C.c_int
    L.ntscsim_batch422_destroy.argtypes = [C.c_void_p]
    L.ntscsim_batch422_destroy.restype = None
    L.ntscsim_raw28_opts_init.argtypes = [C.POINTER(Raw28Opts)]
    L.ntscsim_raw28_opts_init.restype = None
    L.ntscsim_raw28_parse_argv.argtypes = [C.POINTER(Raw28Opts), C.c_int, C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_raw28_parse_argv.restype = C.c_int
    L.ntscsim_raw28_geometry.argtypes = [C.POINTER(Raw28Opts)] + [C.POINTER(C.c_int)] * 3
    L.ntscsim_raw28_geometry.restype = C.c_int
    L.ntscsim_raw28_create.argtypes = [C.POINTER(Raw28Opts), C.c_int, C.POINTER(C.c_void_p)]
    L.ntscsim_raw28_create.restype = C.c_int
    L.ntscsim_raw28_destroy.argtypes = [C.c_void_p]
    L.ntscsim_raw28_destroy.restype = None
    L.ntscsim_raw28_last_error.argtypes = [C.c_void_p]
    L.ntscsim_raw28_last_error.restype = C.c_char_p
    for fn in (L.ntscsim_raw28_decode, L.ntscsim_raw28_decode_device):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]
        fn.restype = C.c_int
    L.ntscsim_raw28_stream_reset.argtypes = [C.c_void_p]
    L.ntscsim_raw28_stream_reset.restype = C.c_int
    L.ntscsim_raw28_stream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                            C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.ntscsim_raw28_stream_push.restype = C.c_int
    L.ntscsim_raw28_get_levels.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.ntscsim_raw28_get_levels.restype = C.c_int
    L.ntscsim_raw28_debug_set_speculation.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ntscsim_raw28_debug_set_speculation.restype = None
    L.ntscsim_raw28_debug_pick_chunk.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ntscsim_raw28_debug_pick_chunk.restype = None
    L.ntscsim_raw28_debug_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.ntscsim_raw28_debug_stats.restype = None
    L.ntscsim_raw28_debug_read_front.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.ntscsim_raw28_debug_read_front.restype = C.c_int
    L.ntscsim_submit_opts_init.argtypes = [C.POINTER(SubmitOpts)]
    L.ntscsim_submit_opts_init.restype = None
    L.ntscsim_submit_configure.argtypes = [C.c_void_p, C.POINTER(SubmitOpts)]
    L.ntscsim_submit_configure.restype = C.c_int
    L.ntscsim_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                 C.c_int, C.c_int, C.c_uint, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.ntscsim_submit.restype = C.c_int
    L.ntscsim_flush.argtypes = [C.c_void_p]
    L.ntscsim_flush.restype = C.c_int
    L.ntscsim_wait.argtypes = [C.c_void_p, C.c_uint64]
    L.ntscsim_wait.restype = C.c_int
    L.ntscsim_host_unpin.argtypes = [C.c_void_p, C.c_void_p]
    L.ntscsim_host_unpin.restype = C.c_int
    L.ntscsim_submit_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.ntscsim_submit_stats.restype = None
    L.ntscsim_host_pin.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.ntscsim_host_pin.restype = C.c_int
    L.ntscsim_host_alloc.argtypes = [C.c_size_t]
    L.ntscsim_host_alloc.restype = C.c_void_p
    L.ntscsim_host_free.argtypes = [C.c_void_p]
    L.ntscsim_host_free.restype = None
    L.ntscsim_host_frame_alloc.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.ntscsim_host_frame_alloc.restype = C.c_int
    L.ntscsim_set_pin_policy.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_set_pin_policy.restype = C.c_int
    L.ntscsim_field422.argtypes = [C.c_void_p, C.POINTER(Loop422)]
    L.ntscsim_field422.restype = C.c_int
    L.ntscsim_submit422.argtypes = [C.c_void_p, C.POINTER(Loop422), C.c_uint32, C.POINTER(C.c_uint64)]
    L.ntscsim_submit422.restype = C.c_int
    L.ntscsim_submit422_configure.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ntscsim_submit422_configure.restype = C.c_int
    L.ntscsim_submit422_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.ntscsim_submit422_stats.restype = None
    L.ntscsim_pool_create.argtypes = [C.POINTER(Params), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
    L.ntscsim_pool_create.restype = C.c_int
    L.ntscsim_pool_destroy.argtypes = [C.c_void_p]
    L.ntscsim_pool_destroy.restype = None
    L.ntscsim_pool_size.argtypes = [C.c_void_p]
    L.ntscsim_pool_size.restype = C.c_int
    L.ntscsim_pool_ctx.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_pool_ctx.restype = C.c_void_p
    L.ntscsim_pool_set_block.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_pool_set_block.restype = C.c_int
    L.ntscsim_pool_get_rng_pos.argtypes = [C.c_void_p]
    L.ntscsim_pool_get_rng_pos.restype = C.c_uint64
    L.ntscsim_pool_set_rng_pos.argtypes = [C.c_void_p, C.c_uint64]
    L.ntscsim_pool_set_rng_pos.restype = None
    L.ntscsim_pool_last_error.argtypes = [C.c_void_p]
    L.ntscsim_pool_last_error.restype = C.c_char_p
    L.ntscsim_pool_frames_host.argtypes = [C.c_void_p, _u8p, C.c_size_t, C.c_int, C.c_int, _u8p, C.c_size_t, C.c_int,
                                           C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_int]
    L.ntscsim_pool_frames_host.restype = C.c_int
    L.ntscsim_blend_params_init.argtypes = [C.POINTER(BlendParams)]
    L.ntscsim_blend_params_init.restype = None
    L.ntscsim_blend_parse_argv.argtypes = [C.POINTER(BlendParams), C.c_int, C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_blend_parse_argv.restype = C.c_int
    L.ntscsim_blend_frame_time.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(BlendParams)]
    L.ntscsim_blend_frame_time.restype = C.c_double
    L.ntscsim_blend_plan_create.argtypes = [C.POINTER(BlendParams), C.POINTER(C.c_void_p)]
    L.ntscsim_blend_plan_create.restype = C.c_int
    L.ntscsim_blend_plan_push.argtypes = [C.c_void_p, C.c_double]
    L.ntscsim_blend_plan_push.restype = C.c_int64
    L.ntscsim_blend_plan_next.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.c_int,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.ntscsim_blend_plan_next.restype = C.c_int
    L.ntscsim_blend_plan_reset.argtypes = [C.c_void_p]
    L.ntscsim_blend_plan_reset.restype = None
    L.ntscsim_blend_plan_destroy.argtypes = [C.c_void_p]
    L.ntscsim_blend_plan_destroy.restype = None
    L.ntscsim_blend_clip_periods.argtypes = [C.c_double]
    L.ntscsim_blend_clip_periods.restype = C.c_int64
    L.ntscsim_blend_tables.argtypes = [C.c_double, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)]
    L.ntscsim_blend_tables.restype = C.c_int
    L.ntscsim_blend_bind.argtypes = [C.c_void_p, C.POINTER(BlendParams)]
    L.ntscsim_blend_bind.restype = C.c_int
    L.ntscsim_blend_frames_device.argtypes = [C.c_void_p, C.POINTER(BlendDesc), C.c_int, C.c_void_p]
    L.ntscsim_blend_frames_device.restype = C.c_int
    L.ntscsim_blend_clip_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_double), C.c_int,
                                            C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                            C.c_void_p]
    L.ntscsim_blend_clip_device.restype = C.c_int
    L.ntscsim_blend_frames_host.argtypes = [C.c_void_p, C.POINTER(BlendDesc), C.c_int]
    L.ntscsim_blend_frames_host.restype = C.c_int
    L.ntscsim_key_params_init.argtypes = [C.POINTER(KeyParams)]
    L.ntscsim_key_params_init.restype = None
    L.ntscsim_key_params_free.argtypes = [C.POINTER(KeyParams)]
    L.ntscsim_key_params_free.restype = None
    L.ntscsim_key_params_add_layer.argtypes = [C.POINTER(KeyParams), C.c_char_p]
    L.ntscsim_key_params_add_layer.restype = C.c_int
    L.ntscsim_key_parse_argv.argtypes = [C.POINTER(KeyParams), C.c_int, C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_key_parse_argv.restype = C.c_int
    L.ntscsim_key_rand_advance.argtypes = [C.POINTER(KeyParams), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]
    L.ntscsim_key_rand_advance.restype = C.c_int
    L.ntscsim_key_bind.argtypes = [C.c_void_p, C.POINTER(KeyParams)]
    L.ntscsim_key_bind.restype = C.c_int
    L.ntscsim_key_frames_device.argtypes = [C.c_void_p, C.POINTER(KeyDesc), C.c_int, C.c_void_p]
    L.ntscsim_key_frames_device.restype = C.c_int
    L.ntscsim_key_clip_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.c_int,
                                          C.c_int, C.POINTER(C.c_uint64), C.c_void_p]
    L.ntscsim_key_clip_device.restype = C.c_int
    L.ntscsim_key_frames_host.argtypes = [C.c_void_p, C.POINTER(KeyDesc), C.c_int]
    L.ntscsim_key_frames_host.restype = C.c_int
    L.ntscsim_key_debug_lane_state.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]
    L.ntscsim_key_debug_lane_state.restype = C.c_int
    L.ntscsim_key_debug_set_bits_limit.argtypes = [C.c_void_p, C.c_size_t]
    L.ntscsim_key_debug_set_bits_limit.restype = C.c_int
    L.ntscsim_avg_params_init.argtypes = [C.POINTER(AvgParams)]
    L.ntscsim_avg_params_init.restype = None
    L.ntscsim_avg_params_free.argtypes = [C.POINTER(AvgParams)]
    L.ntscsim_avg_params_free.restype = None
    L.ntscsim_avg_params_add_layer.argtypes = [C.POINTER(AvgParams), C.c_char_p]
    L.ntscsim_avg_params_add_layer.restype = C.c_int
    L.ntscsim_avg_parse_argv.argtypes = [C.POINTER(AvgParams), C.c_int, C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_avg_parse_argv.restype = C.c_int
    L.ntscsim_avg_bind.argtypes = [C.c_void_p, C.POINTER(AvgParams)]
    L.ntscsim_avg_bind.restype = C.c_int
    L.ntscsim_avg_frames_device.argtypes = [C.c_void_p, C.POINTER(AvgDesc), C.c_int, C.c_void_p]
    L.ntscsim_avg_frames_device.restype = C.c_int
    L.ntscsim_avg_clip_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.c_int,
                                          C.c_int, C.POINTER(C.c_uint64), C.c_void_p]
    L.ntscsim_avg_clip_device.restype = C.c_int
    L.ntscsim_avg_frames_host.argtypes = [C.c_void_p, C.POINTER(AvgDesc), C.c_int]
    L.ntscsim_avg_frames_host.restype = C.c_int
    L.ntscsim_scan_params_init.argtypes = [C.POINTER(ScanParams)]
    L.ntscsim_scan_params_init.restype = None
    L.ntscsim_scan_parse_argv.argtypes = [C.POINTER(ScanParams), C.c_int, C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_scan_parse_argv.restype = C.c_int
    L.ntscsim_scan_effect.argtypes = [C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.ntscsim_scan_effect.restype = None
    L.ntscsim_scan_field_of.argtypes = [C.c_uint64]
    L.ntscsim_scan_field_of.restype = C.c_uint32
    L.ntscsim_scan_bind.argtypes = [C.c_void_p, C.POINTER(ScanParams)]
    L.ntscsim_scan_bind.restype = C.c_int
    L.ntscsim_scan_frames_device.argtypes = [C.c_void_p, C.POINTER(ScanDesc), C.c_int, C.c_void_p]
    L.ntscsim_scan_frames_device.restype = C.c_int
    L.ntscsim_scan_clip_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                           C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_void_p]
    L.ntscsim_scan_clip_device.restype = C.c_int
    L.ntscsim_scan_frames_host.argtypes = [C.c_void_p, C.POINTER(ScanDesc), C.c_int]
    L.ntscsim_scan_frames_host.restype = C.c_int
    L.ntscsim_scan_debug_keep_raster.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_scan_debug_keep_raster.restype = C.c_int
    L.ntscsim_scan_debug_raster.argtypes = [C.c_void_p, C.c_void_p]
    L.ntscsim_scan_debug_raster.restype = C.c_int
    L.ntscsim_scan_debug_set_window_rows.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_scan_debug_set_window_rows.restype = C.c_int
    L.ntscsim_scan_debug_spill.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ntscsim_scan_debug_spill.restype = C.c_int
    L.ntscsim_led_params_init.argtypes = [C.POINTER(LedParams)]
    L.ntscsim_led_params_init.restype = None
    L.ntscsim_led_parse_argv.argtypes = [C.POINTER(LedParams), C.c_int, C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_led_parse_argv.restype = C.c_int
    L.ntscsim_led_bind.argtypes = [C.c_void_p, C.POINTER(LedParams)]
    L.ntscsim_led_bind.restype = C.c_int
    L.ntscsim_led_frames_device.argtypes = [C.c_void_p, C.POINTER(LedDesc), C.c_int, C.c_void_p]
    L.ntscsim_led_frames_device.restype = C.c_int
    L.ntscsim_led_frames_host.argtypes = [C.c_void_p, C.POINTER(LedDesc), C.c_int]
    L.ntscsim_led_frames_host.restype = C.c_int
    L.ntscsim_led_debug_keep_edges.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_led_debug_keep_edges.restype = C.c_int
    L.ntscsim_led_debug_edges.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.ntscsim_led_debug_edges.restype = C.c_int
    L.ntscsim_filmac_params_init.argtypes = [C.POINTER(FilmacParams)]
    L.ntscsim_filmac_params_init.restype = None
    L.ntscsim_filmac_parse_argv.argtypes = [C.POINTER(FilmacParams), C.c_int, C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_filmac_parse_argv.restype = C.c_int
    L.ntscsim_filmac_bind.argtypes = [C.c_void_p, C.POINTER(FilmacParams)]
    L.ntscsim_filmac_bind.restype = C.c_int
    L.ntscsim_filmac_frames_device.argtypes = [C.c_void_p, C.POINTER(FilmacDesc), C.c_int, C.c_void_p]
    L.ntscsim_filmac_frames_device.restype = C.c_int
    L.ntscsim_filmac_frames_host.argtypes = [C.c_void_p, C.POINTER(FilmacDesc), C.c_int]
    L.ntscsim_filmac_frames_host.restype = C.c_int
    L.ntscsim_filmac_reset.argtypes = [C.c_void_p]
    L.ntscsim_filmac_reset.restype = C.c_int
    L.ntscsim_filmac_get_state.argtypes = [C.c_void_p, C.POINTER(FilmacState)]
    L.ntscsim_filmac_get_state.restype = C.c_int
    L.ntscsim_filmac_set_state.argtypes = [C.c_void_p, C.POINTER(FilmacState)]
    L.ntscsim_filmac_set_state.restype = C.c_int
    L.ntscsim_filmac_debug_levels.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.ntscsim_filmac_debug_levels.restype = C.c_int
    L.ntscsim_filmac_debug_time_kernels.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_filmac_debug_time_kernels.restype = C.c_int
    L.ntscsim_filmac_debug_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.ntscsim_filmac_debug_kernel_ms.restype = C.c_int
    L.ntscsim_audio_params_from_cli.argtypes = [C.POINTER(AudioParams), C.POINTER(Params), C.POINTER(Cli)]
    L.ntscsim_audio_params_from_cli.restype = C.c_int
    L.ntscsim_audio_bind.argtypes = [C.c_void_p, C.POINTER(AudioParams)]
    L.ntscsim_audio_bind.restype = C.c_int
    L.ntscsim_audio_device.argtypes = [C.c_void_p, C.POINTER(AudioDesc), C.c_int, C.c_void_p]
    L.ntscsim_audio_device.restype = C.c_int
    L.ntscsim_audio_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.ntscsim_audio_host.restype = C.c_int
    L.ntscsim_audio_reset.argtypes = [C.c_void_p]
    L.ntscsim_audio_reset.restype = C.c_int
    L.ntscsim_audio_get_state.argtypes = [C.c_void_p, C.POINTER(AudioState)]
    L.ntscsim_audio_get_state.restype = C.c_int
    L.ntscsim_audio_set_state.argtypes = [C.c_void_p, C.POINTER(AudioState)]
    L.ntscsim_audio_set_state.restype = C.c_int
    L.ntscsim_audio_debug_set_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.ntscsim_audio_debug_set_plan.restype = C.c_int
    L.ntscsim_audio_debug_stats.argtypes = [C.c_void_p, C.POINTER(AudioStats)]
    L.ntscsim_audio_debug_stats.restype = C.c_int
    L.ntscsim_audio_debug_pulses.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    L.ntscsim_audio_debug_pulses.restype = C.c_int
    L.ntscsim_audio_debug_time_kernels.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_audio_debug_time_kernels.restype = C.c_int
    L.ntscsim_audio_debug_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.ntscsim_audio_debug_kernel_ms.restype = C.c_int
    L.ntscsim_audio_tracks_device.argtypes = [C.c_void_p, C.POINTER(AudioTrack), C.c_int, C.c_void_p]
    L.ntscsim_audio_tracks_device.restype = C.c_int
    L.ntscsim_audio_mixed_tracks_device.argtypes = [C.c_void_p, C.POINTER(AudioParams), C.c_int, C.POINTER(AudioMixedTrack), C.c_int, C.c_void_p]
    L.ntscsim_audio_mixed_tracks_device.restype = C.c_int
    L.ntscsim_audio_mixed_tracks_host.argtypes = [C.c_void_p, C.POINTER(AudioParams), C.c_int, C.POINTER(AudioMixedTrack), C.c_int]
    L.ntscsim_audio_mixed_tracks_host.restype = C.c_int
    L.ntscsim_audio_debug_track_stats.argtypes = [C.c_void_p, C.POINTER(AudioStats), C.c_int]
    L.ntscsim_audio_debug_track_stats.restype = C.c_int
    L.ntscsim_cass_params_init.argtypes = [C.POINTER(CassParams)]
    L.ntscsim_cass_params_init.restype = None
    L.ntscsim_cass_parse_argv.argtypes = [C.POINTER(CassParams), C.c_int, C.POINTER(C.c_char_p), C.c_int]
    L.ntscsim_cass_parse_argv.restype = C.c_int
    L.ntscsim_cass_params_derive.argtypes = [C.POINTER(CassParams)]
    L.ntscsim_cass_params_derive.restype = C.c_int
    L.ntscsim_cass_bind.argtypes = [C.c_void_p, C.POINTER(CassParams)]
    L.ntscsim_cass_bind.restype = C.c_int
    L.ntscsim_cass_device.argtypes = [C.c_void_p, C.POINTER(CassDesc), C.c_int, C.c_void_p]
    L.ntscsim_cass_device.restype = C.c_int
    L.ntscsim_cass_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.ntscsim_cass_host.restype = C.c_int
    L.ntscsim_cass_reset.argtypes = [C.c_void_p]
    L.ntscsim_cass_reset.restype = C.c_int
    L.ntscsim_cass_get_state.argtypes = [C.c_void_p, C.POINTER(CassState)]
    L.ntscsim_cass_get_state.restype = C.c_int
    L.ntscsim_cass_set_state.argtypes = [C.c_void_p, C.POINTER(CassState)]
    L.ntscsim_cass_set_state.restype = C.c_int
    L.ntscsim_cass_debug_set_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.ntscsim_cass_debug_set_plan.restype = C.c_int
    L.ntscsim_cass_debug_stats.argtypes = [C.c_void_p, C.POINTER(CassStats)]
    L.ntscsim_cass_debug_stats.restype = C.c_int
    L.ntscsim_cass_debug_time_kernels.argtypes = [C.c_void_p, C.c_int]
    L.ntscsim_cass_debug_time_kernels.restype = C.c_int
    L.ntscsim_cass_debug_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.ntscsim_cass_debug_kernel_ms.restype = C.c_int
    L.ntscsim_cass_tracks_device.argtypes = [C.c_void_p, C.POINTER(CassTrack), C.c_int, C.c_void_p]
    L.ntscsim_cass_tracks_device.restype = C.c_int
    L.ntscsim_cass_mixed_tracks_device.argtypes = [C.c_void_p, C.POINTER(CassParams), C.c_int, C.POINTER(CassMixedTrack), C.c_int, C.c_void_p]
    L.ntscsim_cass_mixed_tracks_device.restype = C.c_int
    L.ntscsim_cass_mixed_tracks_host.argtypes = [C.c_void_p, C.POINTER(CassParams), C.c_int, C.POINTER(CassMixedTrack), C.c_int]
    L.ntscsim_cass_mixed_tracks_host.restype = C.c_int
    L.ntscsim_cass_debug_track_stats.argtypes = [C.c_void_p, C.POINTER(CassStats), C.c_int]
    L.ntscsim_cass_debug_track_stats.restype = C.c_int
    L.ntscsim_cass_debug_tilt_frames.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.ntscsim_cass_debug_tilt_frames.restype = C.c_int
    L.ntscsim_pixmap_params_init.argtypes = [C.POINTER(PixmapParams)]
    L.ntscsim_pixmap_params_init.restype = None
    L.ntscsim_pixmap_params_free.argtypes = [C.POINTER(PixmapParams)]
    L.ntscsim_pixmap_params_free.restype = None
    L.ntscsim_pixmap_parse_argv.argtypes = [C.POINTER(PixmapParams), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int]
    L.ntscsim_pixmap_parse_argv.restype = C.c_int
    for stage, desc in (("post", PostDesc), ("cmap", CmapDesc)):
        fn = lambda what: getattr(L, "ntscsim_%s_%s" % (stage, what))
        fn("params_init").argtypes = [C.POINTER(PixmapParams)]
        fn("params_init").restype = None
        fn("params_free").argtypes = [C.POINTER(PixmapParams)]
        fn("params_free").restype = None
        fn("parse_argv").argtypes = [C.POINTER(PixmapParams), C.c_int, C.POINTER(C.c_char_p), C.c_int]
        fn("parse_argv").restype = C.c_int
        fn("bind").argtypes = [C.c_void_p, C.POINTER(PixmapParams)]
        fn("bind").restype = C.c_int
        fn("frames_device").argtypes = [C.c_void_p, C.POINTER(desc), C.c_int, C.c_void_p]
        fn("frames_device").restype = C.c_int
        fn("frames_host").argtypes = [C.c_void_p, C.POINTER(desc), C.c_int]
        fn("frames_host").restype = C.c_int
    L.ntscsim_cmap_reset.argtypes = [C.c_void_p]
    L.ntscsim_cmap_reset.restype = C.c_int
    L.ntscsim_cmap_get_table.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.ntscsim_cmap_get_table.restype = C.c_int
    L.ntscsim_cmap_set_table.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.ntscsim_cmap_set_table.restype = C.c_int
    _lib = L
    return L


class NtscsimError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = lib().ntscsim_strerror(code).decode()
        super().__init__("ntscsim error %d: %s%s" % (code, msg, (" -- " + detail) if detail else ""))


def make_params_to_composite(flags=(), **overrides):
    """ntscsim_params from ffmpeg_to_composite's switches (ffmpeg_to_composite.cpp :1325)."""
    L = lib()
    p = Params()
    L.ntscsim_params_init_to_composite(C.byref(p))
    argv = [b"ffmpeg_to_composite"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    rc = L.ntscsim_params_parse_argv_to_composite(C.byref(p), None, len(argv), arr, 0)
    if rc != OK:
        raise NtscsimError(rc, "parse_argv_to_composite(%r)" % (list(flags),))
    for k, v in overrides.items():
        if k not in dict(Params._fields_):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def make_params(flags=(), **overrides):
    """ntscsim_params from the reference's CLI switches (ffmpeg_ntsc.cpp parse_argv :972)."""
    L = lib()
    p = Params()
    L.ntscsim_params_init(C.byref(p))
    argv = [b"ffmpeg_ntsc"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    rc = L.ntscsim_params_parse_argv(C.byref(p), None, len(argv), arr, 0)
    if rc != OK:
        raise NtscsimError(rc, "parse_argv(%r)" % (list(flags),))
    for k, v in overrides.items():
        if k not in dict(Params._fields_):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def make_audio_params(flags=(), tool="ntsc"):
    """(ntscsim_audio_params, ntscsim_params) from the switches of ffmpeg_ntsc (tool="ntsc") or ffmpeg_to_composite
    (tool="to_composite"): the parser's record, then ntscsim_audio_params_from_cli()."""
    L = lib()
    p, cli, ap = Params(), Cli(), AudioParams()
    L.ntscsim_cli_init(C.byref(cli))
    sibling = tool == "to_composite"
    (L.ntscsim_params_init_to_composite if sibling else L.ntscsim_params_init)(C.byref(p))
    argv = [b"ffmpeg_to_composite" if sibling else b"ffmpeg_ntsc"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    parse = L.ntscsim_params_parse_argv_to_composite if sibling else L.ntscsim_params_parse_argv
    rc = parse(C.byref(p), C.cast(C.byref(cli), C.c_void_p), len(argv), arr, 0)
    if rc != OK:
        raise NtscsimError(rc, "parse_argv(%r)" % (list(flags),))
    rc = L.ntscsim_audio_params_from_cli(C.byref(ap), C.byref(p), C.byref(cli))
    if rc != OK:
        raise NtscsimError(rc, "ntscsim_audio_params_from_cli")
    return ap, p


def make_cass_params(flags=(), require_io=False):
    """ntscsim_cass_params from ffmpeg_cassette's switches (ffmpeg_cassette.cpp parse_argv :441-590), derived settings
    included.  The switch strings are kept alive on the result (input_path / output_path point into them)."""
    L = lib()
    cp = CassParams()
    argv = [b"ffmpeg_cassette"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    rc = L.ntscsim_cass_parse_argv(C.byref(cp), len(argv), arr, 1 if require_io else 0)
    if rc != OK:
        raise NtscsimError(rc, "ntscsim_cass_parse_argv(%r)" % (list(flags),))
    cp._argv = arr
    return cp


def make_raw28_opts(flags=()):
    """ntscsim_raw28_opts from ffmpeg_raw28ntsc's switches (ffmpeg_raw28ntsc.cpp parse_argv :442)."""
    L = lib()
    o = Raw28Opts()
    L.ntscsim_raw28_opts_init(C.byref(o))
    argv = [b"ffmpeg_raw28ntsc"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    rc = L.ntscsim_raw28_parse_argv(C.byref(o), len(argv), arr, 1)
    if rc != OK:
        raise NtscsimError(rc, "raw28 parse_argv(%r)" % (list(flags),))
    return o


def make_blend_params(flags=(), require_io=False):
    """ntscsim_blend_params from frameblend's switches (frameblend.cpp parse_argv :512).  The returned struct keeps
    the argv strings alive (input_path / output_path point into them)."""
    L = lib()
    p = BlendParams()
    L.ntscsim_blend_params_init(C.byref(p))
    argv = [b"frameblend"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    rc = L.ntscsim_blend_parse_argv(C.byref(p), len(argv), arr, int(bool(require_io)))
    if rc != OK:
        raise NtscsimError(rc, "blend parse_argv(%r)" % (list(flags),))
    p._argv = arr
    return p


def make_key_params(flags=(), require_io=False, width=None, height=None):
    """ntscsim_key_params from ffmpeg_colorkey's switches (ffmpeg_colorkey.cpp parse_argv :629).  width / height
    override the frame size after parsing (the tool has no -height).  The returned struct keeps the argv strings
    alive (the layers' paths and output_path point into them) and frees its layer list when it is collected."""
    L = lib()
    p = KeyParams()
    L.ntscsim_key_params_init(C.byref(p))
    argv = [b"ffmpeg_colorkey"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    p._argv = arr
    rc = L.ntscsim_key_parse_argv(C.byref(p), len(argv), arr, int(bool(require_io)))
    if rc != OK:
        raise NtscsimError(rc, "key parse_argv(%r)" % (list(flags),))
    if width is not None:
        p.width = int(width)
    if height is not None:
        p.height = int(height)
    return p


def make_avg_params(flags=(), require_io=False, width=None, height=None):
    """ntscsim_avg_params from ffmpeg_average_delay's switches (ffmpeg_average_delay.cpp parse_argv :623).  width /
    height override the frame size after parsing (the tool has no -height).  The returned struct keeps the argv strings
    alive (the layers' paths and output_path point into them) and frees its layer list when it is collected."""
    L = lib()
    p = AvgParams()
    L.ntscsim_avg_params_init(C.byref(p))
    argv = [b"ffmpeg_average_delay"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    p._argv = arr
    rc = L.ntscsim_avg_parse_argv(C.byref(p), len(argv), arr, int(bool(require_io)))
    if rc != OK:
        raise NtscsimError(rc, "avg parse_argv(%r)" % (list(flags),))
    if width is not None:
        p.width = int(width)
    if height is not None:
        p.height = int(height)
    return p


def make_scan_params(flags=(), require_io=False, width=None, height=None):
    """ntscsim_scan_params from ffmpeg_scanimate's switches (ffmpeg_scanimate.cpp parse_argv :643).  width / height
    override the output size after parsing (the tool has no -height).  The returned struct keeps the argv strings alive
    (last_input_path / output_path point into them)."""
    L = lib()
    p = ScanParams()
    L.ntscsim_scan_params_init(C.byref(p))
    argv = [b"ffmpeg_scanimate"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    p._argv = arr
    rc = L.ntscsim_scan_parse_argv(C.byref(p), len(argv), arr, int(bool(require_io)))
    if rc != OK:
        raise NtscsimError(rc, "scan parse_argv(%r)" % (list(flags),))
    if width is not None:
        p.output_width = int(width)
    if height is not None:
        p.output_height = int(height)
    return p


def make_led_params(flags=(), require_io=False, width=None, height=None):
    """ntscsim_led_params from ffmpeg_vhsled's switches (ffmpeg_vhsled.cpp parse_argv :476).  width / height override
    the frame size after parsing (the tool takes it from its input when the switches are absent).  The returned struct
    keeps the argv strings alive (input_path / output_path point into them)."""
    L = lib()
    p = LedParams()
    L.ntscsim_led_params_init(C.byref(p))
    argv = [b"ffmpeg_vhsled"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    p._argv = arr
    rc = L.ntscsim_led_parse_argv(C.byref(p), len(argv), arr, int(bool(require_io)))
    if rc != OK:
        raise NtscsimError(rc, "led parse_argv(%r)" % (list(flags),))
    if width is not None:
        p.width = int(width)
    if height is not None:
        p.height = int(height)
    return p


def make_filmac_params(flags=(), require_io=False, width=None, height=None):
    """ntscsim_filmac_params from filmac's switches (filmac.cpp parse_argv :476, the same text as ffmpeg_vhsled's).
    width / height override the frame size after parsing.  The returned struct keeps the argv strings alive."""
    L = lib()
    p = FilmacParams()
    L.ntscsim_filmac_params_init(C.byref(p))
    argv = [b"filmac"] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    p._argv = arr
    rc = L.ntscsim_filmac_parse_argv(C.byref(p), len(argv), arr, int(bool(require_io)))
    if rc != OK:
        raise NtscsimError(rc, "filmac parse_argv(%r)" % (list(flags),))
    if width is not None:
        p.width = int(width)
    if height is not None:
        p.height = int(height)
    return p


def make_pixmap_params(stage, flags=(), require_io=False, width=None, height=None):
    """ntscsim_post_params (stage "post": ffmpeg_posterize.cpp parse_argv :620) or ntscsim_cmap_params (stage "cmap":
    ffmpeg_colormap.cpp parse_argv :622) from the tool's switches.  width / height override the frame size after parsing
    (the tools have no -height).  The returned struct keeps the argv strings alive (the inputs' paths and output_path
    point into them) and frees its input list when it is collected."""
    L = lib()
    p = PixmapParams()
    getattr(L, "ntscsim_%s_params_init" % stage)(C.byref(p))
    argv = [stage.encode()] + [str(f).encode() for f in flags]
    arr = (C.c_char_p * len(argv))(*argv)
    p._argv = arr
    rc = getattr(L, "ntscsim_%s_parse_argv" % stage)(C.byref(p), len(argv), arr, int(bool(require_io)))
    if rc != OK:
        raise NtscsimError(rc, "%s parse_argv(%r)" % (stage, list(flags)))
    if width is not None:
        p.width = int(width)
    if height is not None:
        p.height = int(height)
    return p
