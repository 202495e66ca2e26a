"""ntscsim -- host-side Python mirror of the reference's per-field interface
(composite_layer(), ffmpeg_ntsc.cpp:1570, and the field loop around it, :2202-2282), calling the
hand-written HIP kernels through the C-ABI of include/ntscsim.h.

torch is used only for device memory, streams and torch.distributed plumbing.
"""
import ctypes as C

try:                # before libntscsim.so is loaded: one HIP runtime for torch and the library (_capi.lib)
    import torch  # noqa: F401
except ImportError:
    pass

from . import _capi
from ._capi import (DESC_BOB, DESC_INTERLACED, DESC_TFF, RNG_AUTO, Field422Desc, FieldDesc, MixedFieldDesc,
                    NtscsimError, Out422Desc, YuvDesc, ScaleDesc, HostSource, Params, lib, make_params,
                    make_params_to_composite)

__all__ = ["FieldSimulator", "FrameBlender", "ColorKeyer", "FrameAverager", "Scanimator", "EdgeAligner", "AutoContrast", "AudioChain", "Cassette", "Posterizer", "ColorMapper", "blend_plan", "blend_frame_times", "Pool", "Params", "FieldDesc", "make_params", "NtscsimError", "lib",
           "field_rows", "calls_per_field", "field_schedule"]


def field_rows(height, field):
    """Rows composite_layer touches: y = field, field+2, ... < height."""
    return (height - field + 1) // 2 if height > field else 0


def calls_per_field(params, width, height, field):
    return int(lib().ntscsim_rng_calls_per_field(C.byref(params), width, height, field))


def field_schedule(n_fields, first=0):
    """The reference's field loop (ffmpeg_ntsc.cpp:2202-2229): output field `current` uses
    field parity (current & 1) ^ 1 and fieldno = current."""
    return [((cur & 1) ^ 1, cur) for cur in range(first, first + n_fields)]


class FieldSimulator:
    """One GPU context.  `flags` are the reference's CLI switches, e.g. ("-vhs",)."""

    def __init__(self, flags=(), device=0, params=None):
        self.params = params if params is not None else make_params(flags)
        self._lib = lib()
        h = C.c_void_p()
        rc = self._lib.ntscsim_create(C.byref(self.params), int(device), C.byref(h))
        if rc != _capi.OK:
            raise NtscsimError(rc, "ntscsim_create(device=%d)" % device)
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ntscsim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != _capi.OK:
            raise NtscsimError(rc, "%s: %s" % (what, self._lib.ntscsim_last_error(self._h).decode()))

    def set_mode(self, mode):
        """_capi.MODE_EXACT (default, bit-identical to the reference), _capi.MODE_FAST32 or _capi.MODE_FLOAT."""
        self._chk(self._lib.ntscsim_set_mode(self._h, int(mode)), "ntscsim_set_mode")

    # ---- rand() stream position -----------------------------------------------------------
    @property
    def rng_pos(self):
        return int(self._lib.ntscsim_get_rng_pos(self._h))

    @rng_pos.setter
    def rng_pos(self, pos):
        self._lib.ntscsim_set_rng_pos(self._h, int(pos))

    # ---- drop-in for composite_layer(): host (numpy) frames ---------------------------------
    def field_host(self, dst, src, field, fieldno, interlaced=0, tff=0):
        """dst, src: numpy uint8 [H, W, 4] BGRA (C-contiguous).  Writes rows field, field+2, ..."""
        h, w = src.shape[:2]
        assert src.shape == dst.shape and src.shape[2] == 4
        u8p = C.POINTER(C.c_uint8)
        rc = self._lib.ntscsim_field(self._h, src.ctypes.data_as(u8p), src.strides[0],
                                     int(interlaced), int(tff), dst.ctypes.data_as(u8p),
                                     dst.strides[0], w, h, int(field), int(fieldno))
        self._chk(rc, "ntscsim_field")

    # ---- the asynchronous form of the same drop-in: ntscsim_submit() / ntscsim_wait() ------
    def submit_configure(self, depth=32, slots=0, lanes=3, pin=True, min_pin_bytes=256 << 10):
        o = _capi.SubmitOpts()
        self._lib.ntscsim_submit_opts_init(C.byref(o))
        o.depth, o.slots, o.lanes = int(depth), int(slots), int(lanes)
        o.pin_caller_buffers, o.min_pin_bytes = int(bool(pin)), int(min_pin_bytes)
        self._chk(self._lib.ntscsim_submit_configure(self._h, C.byref(o)), "ntscsim_submit_configure")

    def submit(self, dst, src, field, fieldno, interlaced=0, tff=0, bob=False, same_src=False,
               src_stable=False):
        """As field_host(), asynchronously: returns a ticket; dst is complete after wait(ticket).
        dst, src: numpy uint8 [H, W, 4] (rows contiguous; any row stride)."""
        h, w = src.shape[:2]
        assert src.shape == dst.shape and src.shape[2] == 4 and src.strides[1] == 4 and dst.strides[1] == 4
        flags = (DESC_BOB if bob else 0) | (_capi.SUBMIT_SAME_SRC if same_src else 0) | \
                (_capi.SUBMIT_SRC_STABLE if src_stable else 0)
        t = C.c_uint64(0)
        rc = self._lib.ntscsim_submit(self._h, src.ctypes.data, src.strides[0], int(interlaced), int(tff),
                                      dst.ctypes.data, dst.strides[0], w, h, int(field), int(fieldno),
                                      flags, C.byref(t))
        self._chk(rc, "ntscsim_submit")
        return int(t.value)

    def wait(self, ticket=None):
        self._chk(self._lib.ntscsim_wait(self._h, _capi.TICKET_ALL if ticket is None else int(ticket)),
                  "ntscsim_wait")

    def flush(self):
        self._chk(self._lib.ntscsim_flush(self._h), "ntscsim_flush")

    def host_unpin(self, array=None):
        self._chk(self._lib.ntscsim_host_unpin(self._h, None if array is None else array.ctypes.data),
                  "ntscsim_host_unpin")

    def host_pin(self, array):
        """ntscsim_host_pin(): declare a numpy array's memory as the caller's own to pin."""
        self._chk(self._lib.ntscsim_host_pin(self._h, array.ctypes.data, array.nbytes), "ntscsim_host_pin")

    def set_pin_policy(self, policy):
        self._chk(self._lib.ntscsim_set_pin_policy(self._h, int(policy)), "ntscsim_set_pin_policy")

    def submit_stats(self):
        out = (C.c_uint64 * 8)()
        self._lib.ntscsim_submit_stats(self._h, out)
        keys = ("submitted", "launches", "uploads", "uploads_staged", "delivered_direct", "delivered_staged",
                "registrations", "ring_full_waits")
        return dict(zip(keys, [int(v) for v in out]))

    def frames_host(self, dst, src, first_fieldno=0, bob=True, chunk_frames=0, yuv=None):
        """The field loop over host frames: src numpy uint8 [N, H, W, 4], dst [2N, H, W, 4].
        yuv = "420" / "422": dst is uint8 [2N, frame_bytes], each frame Y|U|V planes packed at
        linesize W (chroma W/2)."""
        n, h, w = src.shape[:3]
        assert src.flags.c_contiguous and dst.flags.c_contiguous
        u8p = C.POINTER(C.c_uint8)
        flags = DESC_BOB if bob else 0
        if yuv is None:
            assert dst.shape == (2 * n, h, w, 4)
            dls = dst.strides[1]
        else:
            flags |= _capi.HOST_YUV420P if yuv == "420" else _capi.HOST_YUV422P
            assert dst.ndim == 2 and dst.shape[0] == 2 * n
            dls = w
        rc = self._lib.ntscsim_frames_host(self._h, src.ctypes.data_as(u8p), src.strides[0],
                                           src.strides[1], n, dst.ctypes.data_as(u8p),
                                           dst.strides[0], dls, w, h, int(first_fieldno),
                                           flags, int(chunk_frames))
        self._chk(rc, "ntscsim_frames_host")

    def bgra_to_yuv(self, jobs, width, height, pix_fmt, stream=None):
        """jobs: list of (bgra CUDA uint8 tensor [H, ls], (y, u, v) CUDA uint8 tensors [rows, ls])."""
        arr = (YuvDesc * len(jobs))()
        for d, (bgra, planes) in zip(arr, jobs):
            d.bgra_dev = bgra.data_ptr()
            d.bgra_linesize = bgra.stride(0)
            for k in range(3):
                d.yuv_dev[k] = planes[k].data_ptr()
                d.yuv_linesize[k] = planes[k].stride(0)
        if stream is None:
            stream = self._torch_stream()
        rc = self._lib.ntscsim_bgra_to_yuv_device(self._h, arr, len(jobs), int(width), int(height),
                                                  int(pix_fmt), C.c_void_p(stream))
        self._chk(rc, "ntscsim_bgra_to_yuv_device")

    def scale_to_bgra(self, jobs, width, height, stream=None):
        """jobs: list of (src planes: 1 (BGRA) or 3 (Y, U, V) CUDA uint8 tensors [rows, ls], src_width,
        src_height, format _capi.SRC_*, dst BGRA CUDA uint8 tensor [height, ls])."""
        arr = (ScaleDesc * len(jobs))()
        for d, (planes, sw, sh, fmt, dst) in zip(arr, jobs):
            for k, pl in enumerate(planes):
                d.src_dev[k] = pl.data_ptr()
                d.src_linesize[k] = pl.stride(0)
            d.bgra_dev = dst.data_ptr()
            d.bgra_linesize = dst.stride(0)
            d.src_width, d.src_height, d.src_format = int(sw), int(sh), int(fmt)
        if stream is None:
            stream = self._torch_stream()
        rc = self._lib.ntscsim_scale_to_bgra_device(self._h, arr, len(jobs), int(width), int(height),
                                                    C.c_void_p(stream))
        self._chk(rc, "ntscsim_scale_to_bgra_device")

    def frames_host_scaled(self, dst, src, source, width, height, first_fieldno=0, bob=True, chunk_frames=0, yuv=None):
        """src: numpy uint8 [N, frame_bytes] (frames in the layout `source`, a HostSource);
        dst: numpy uint8 [2N, height, width, 4], or with yuv = "420" / "422" uint8 [2N, frame_bytes]
        (Y|U|V planes packed at linesize width, chroma width/2)."""
        n = src.shape[0]
        # (frames may be strided: only each frame's own bytes must be contiguous)
        assert src.ndim == 2 and src.strides[1] == 1 and dst.flags.c_contiguous
        flags = DESC_BOB if bob else 0
        if yuv is None:
            assert dst.shape == (2 * n, height, width, 4)
            dls = dst.strides[1]
        else:
            flags |= _capi.HOST_YUV420P if yuv == "420" else _capi.HOST_YUV422P
            assert dst.ndim == 2 and dst.shape[0] == 2 * n
            dls = width
        u8p = C.POINTER(C.c_uint8)
        rc = self._lib.ntscsim_frames_host_scaled(self._h, C.byref(source), src.ctypes.data_as(u8p), src.strides[0], n,
                                                  dst.ctypes.data_as(u8p), dst.strides[0], dls,
                                                  int(width), int(height), int(first_fieldno),
                                                  flags, int(chunk_frames))
        self._chk(rc, "ntscsim_frames_host_scaled")

    # ---- batched, device-resident -----------------------------------------------------------
    def build_descs(self, src, dst, jobs, bob=False, interlaced=0, tff=0, rng_pos=None):
        """src, dst: torch uint8 CUDA tensors [N, H, W, 4].  jobs: iterable of
        (src_index, dst_index, field, fieldno).  rng_pos: None (sequential from the ctx
        position) or a list of absolute rand() stream positions."""
        assert src.is_cuda and dst.is_cuda and src.dim() == 4 and dst.dim() == 4
        assert src.stride(2) == 4 and src.stride(3) == 1 and dst.stride(2) == 4 and dst.stride(3) == 1
        jobs = list(jobs)
        arr = (FieldDesc * len(jobs))()
        sbase, dbase = src.data_ptr(), dst.data_ptr()
        sfs, dfs = src.stride(0), dst.stride(0)
        flags = (DESC_INTERLACED if interlaced else 0) | (DESC_TFF if tff else 0) | \
                (DESC_BOB if bob else 0)
        for i, (si, di, field, fieldno) in enumerate(jobs):
            d = arr[i]
            d.src_dev = sbase + si * sfs
            d.dst_dev = dbase + di * dfs
            d.src_linesize = src.stride(1)
            d.dst_linesize = dst.stride(1)
            d.field = field
            d.flags = flags
            d.fieldno = fieldno
            d.rng_pos = RNG_AUTO if rng_pos is None else int(rng_pos[i])
        return arr

    def run_descs(self, descs, width, height, stream=None):
        """Enqueue; does not synchronise."""
        if stream is None:
            stream = self._torch_stream()
        rc = self._lib.ntscsim_fields_device(self._h, descs, len(descs), int(width), int(height),
                                             C.c_void_p(stream))
        self._chk(rc, "ntscsim_fields_device")

    def prepare(self, descs, width, height):
        """Prepared batch (ntscsim_batch_create): returns a handle for run_prepared()."""
        h = C.c_void_p()
        rc = self._lib.ntscsim_batch_create(self._h, descs, len(descs), int(width), int(height),
                                            C.byref(h))
        self._chk(rc, "ntscsim_batch_create")
        return h

    def run_prepared(self, batch, stream=None):
        if stream is None:
            stream = self._torch_stream()
        self._chk(self._lib.ntscsim_batch_run(batch, C.c_void_p(stream)), "ntscsim_batch_run")

    def free_prepared(self, batch):
        self._lib.ntscsim_batch_destroy(batch)

    def fields(self, src, dst, jobs, **kw):
        descs = self.build_descs(src, dst, jobs, **kw)
        self.run_descs(descs, src.shape[2], src.shape[1])
        return descs

    # ---- the same with parameters per field (ntscsim_mixed_fields_device) -------------------
    @staticmethod
    def build_sets(sets):
        """sets: list of Params or flag lists -> ntscsim_params array (None for an empty list)."""
        if not sets:
            return None
        arr = (Params * len(sets))()
        for i, s in enumerate(sets):
            arr[i] = s if isinstance(s, Params) else make_params(s)
        return arr

    def build_mixed_descs(self, set_of, src, dst, jobs, bob=False, interlaced=0, tff=0, rng_pos=None):
        """As build_descs(); set_of[i] is the set of job i (-1: this simulator's own parameters).  bob, interlaced and
        tff may be one value for the call or a list with one value per job."""
        jobs = list(jobs)
        assert len(set_of) == len(jobs)

        def per_job(v, i):
            return v[i] if isinstance(v, (list, tuple)) else v
        arr = (MixedFieldDesc * len(jobs))()
        for i, job in enumerate(jobs):
            one = self.build_descs(src, dst, [job], bob=per_job(bob, i), interlaced=per_job(interlaced, i),
                                   tff=per_job(tff, i), rng_pos=None if rng_pos is None else [rng_pos[i]])
            arr[i].d = one[0]
            arr[i].set = int(set_of[i])
        return arr

    def run_mixed_descs(self, sets, descs, width, height, stream=None):
        """Enqueue; does not synchronise.  sets: what build_sets() returns (or a list it accepts)."""
        if isinstance(sets, (list, tuple)):
            sets = self.build_sets(sets)
        if stream is None:
            stream = self._torch_stream()
        rc = self._lib.ntscsim_mixed_fields_device(self._h, sets, 0 if sets is None else len(sets), descs, len(descs),
                                                   int(width), int(height), C.c_void_p(stream))
        self._chk(rc, "ntscsim_mixed_fields_device")

    def mixed_fields(self, sets, set_of, src, dst, jobs, **kw):
        """fields() with the parameters of sets[set_of[i]] for job i: one launch of each kernel for all of them."""
        descs = self.build_mixed_descs(set_of, src, dst, jobs, **kw)
        self.run_mixed_descs(sets, descs, src.shape[2], src.shape[1])
        return descs

    # ---- 8-bit YUV422P sibling (ffmpeg_to_composite) ---------------------------------------
    def build_descs422(self, jobs):
        """jobs: list of dicts with keys dst (3 CUDA uint8 tensors [H, ls]), optional src (3
        tensors) + src_height, optional flt (3 tensors), field, fieldno, flags, rng_pos.
        Returns the ntscsim_field422_desc array (reusable: run_descs422)."""
        arr = (Field422Desc * len(jobs))()
        for d, j in zip(arr, jobs):
            for k in range(3):
                d.dst_dev[k] = j["dst"][k].data_ptr()
                d.dst_linesize[k] = j["dst"][k].stride(0)
                if j.get("src") is not None:
                    d.src_dev[k] = j["src"][k].data_ptr()
                    d.src_linesize[k] = j["src"][k].stride(0)
                if j.get("flt") is not None:
                    d.flt_dev[k] = j["flt"][k].data_ptr()
                    d.flt_linesize[k] = j["flt"][k].stride(0)
            d.src_height = j.get("src_height", 0)
            d.field = j["field"]
            d.flags = j.get("flags", 0)
            d.fieldno = j["fieldno"]
            d.rng_pos = RNG_AUTO if j.get("rng_pos") is None else int(j["rng_pos"])
        return arr

    def run_descs422(self, arr, width, height, stream=None):
        if stream is None:
            stream = self._torch_stream()
        rc = self._lib.ntscsim_fields422_device(self._h, arr, len(arr), int(width), int(height),
                                                C.c_void_p(stream))
        self._chk(rc, "ntscsim_fields422_device")

    def prepare422(self, arr, width, height):
        """ntscsim_batch422_create on a descriptor array (keep `arr` and its tensors alive)."""
        b = C.c_void_p()
        rc = self._lib.ntscsim_batch422_create(self._h, arr, len(arr), int(width), int(height), C.byref(b))
        self._chk(rc, "ntscsim_batch422_create")
        return b

    def run_prepared422(self, batch, stream=None):
        if stream is None:
            stream = self._torch_stream()
        self._chk(self._lib.ntscsim_batch422_run(batch, C.c_void_p(stream)), "ntscsim_batch422_run")

    def free_prepared422(self, batch):
        self._lib.ntscsim_batch422_destroy(batch)

    def fields422(self, jobs, width, height, stream=None):
        """build_descs422 + run_descs422."""
        self.run_descs422(self.build_descs422(jobs), width, height, stream)

    # ---- the same with parameters per field (ntscsim_mixed_fields422_device) ----------------
    def build_mixed_descs422(self, sets_idx, jobs, rng_pos=None):
        """As build_descs422(); sets_idx[i] is the set of job i (-1: this simulator's own parameters).  rng_pos: None
        (every job's own "rng_pos" key, as in build_descs422) or a list with one absolute position or None per job."""
        jobs = list(jobs)
        assert len(sets_idx) == len(jobs)
        if rng_pos is not None:
            assert len(rng_pos) == len(jobs)
            jobs = [dict(j, rng_pos=rp) for j, rp in zip(jobs, rng_pos)]
        plain = self.build_descs422(jobs)
        arr = (_capi.MixedField422Desc * len(jobs))()
        for i in range(len(jobs)):
            arr[i].d = plain[i]
            arr[i].set = int(sets_idx[i])
        return arr

    @staticmethod
    def build_sets422(sets):
        """sets: list of Params or ffmpeg_to_composite flag lists -> ntscsim_params array (None for an empty list)."""
        if not sets:
            return None
        arr = (Params * len(sets))()
        for i, s in enumerate(sets):
            arr[i] = s if isinstance(s, Params) else make_params_to_composite(s)
        return arr

    def run_mixed_descs422(self, sets, arr, width, height, stream=None):
        """Enqueue; does not synchronise.  sets: what build_sets422() returns, or a list it accepts (Params or
        ffmpeg_to_composite flag lists)."""
        if isinstance(sets, (list, tuple)):
            sets = self.build_sets422(sets)
        if stream is None:
            stream = self._torch_stream()
        rc = self._lib.ntscsim_mixed_fields422_device(self._h, sets, 0 if sets is None else len(sets), arr, len(arr),
                                                      int(width), int(height), C.c_void_p(stream))
        self._chk(rc, "ntscsim_mixed_fields422_device")

    def output422(self, jobs, width, height, stream=None):
        """jobs: list of dicts {frame: 3 CUDA uint8 tensors, bob: 3 tensors, field, mode}."""
        arr = (Out422Desc * len(jobs))()
        for d, j in zip(arr, jobs):
            for k in range(3):
                d.frame_dev[k] = j["frame"][k].data_ptr()
                d.frame_linesize[k] = j["frame"][k].stride(0)
                d.bob_dev[k] = j["bob"][k].data_ptr()
                d.bob_linesize[k] = j["bob"][k].stride(0)
            d.field = j["field"]
            d.mode = j["mode"]
        if stream is None:
            stream = self._torch_stream()
        rc = self._lib.ntscsim_output422_device(self._h, arr, len(jobs), int(width), int(height),
                                                C.c_void_p(stream))
        self._chk(rc, "ntscsim_output422_device")

    def _torch_stream(self):
        """Handle of torch's current stream.  The legacy default stream has handle 0, which the C
        ABI reads as "the context's own (non-blocking) stream": nothing would order the kernels
        behind torch work still queued on the default stream, so that work is waited for here."""
        import torch
        st = torch.cuda.current_stream(self.device)
        if st.cuda_stream == 0:
            st.synchronize()
        return st.cuda_stream

    def sync(self):
        self._chk(self._lib.ntscsim_sync(self._h), "ntscsim_sync")

    def debug_field_stats(self):
        """[calls of ntscsim_field, sources read in place, destinations written in place, early setup kernels used]"""
        a = (C.c_uint64 * 4)()
        self._lib.ntscsim_debug_field_stats(self._h, a)
        return list(a)

    def set_launch_form(self, latency=True):
        """Device-resident launches of up to 64 fields as wavefront roles (ntscsim_set_launch_form: NTSCSIM_FORM_LATENCY)."""
        self._chk(self._lib.ntscsim_set_launch_form(self._h, 1 if latency else 0), "ntscsim_set_launch_form")

    def set_mixed_forms(self, tuned=True):
        """Later mixed_fields() calls run sets of the default / -vhs preset families on the hand-tuned kernels
        (ntscsim_set_mixed_forms: NTSCSIM_MIXED_TUNED); every other set keeps the generic mixed kernels.  Same bytes."""
        self._chk(self._lib.ntscsim_set_mixed_forms(self._h, 1 if tuned else 0), "ntscsim_set_mixed_forms")

    def set_profiling(self, on=True):
        self._lib.ntscsim_set_profiling(self._h, 1 if on else 0)

    def timings_ms(self):
        """Summed hipEvent timings (ms) of the calls made since the last query."""
        out = (C.c_float * 4)()
        n = C.c_int(0)
        self._chk(self._lib.ntscsim_get_timings_ms(self._h, out, C.byref(n)),
                  "ntscsim_get_timings_ms")
        return {"setup": out[0], "encode": out[1], "decode": out[2], "total": out[3],
                "calls": n.value}

    def debug_mixed_tables(self):
        """[jump-table sets cached, cos/sin tables cached, times the caches were dropped] of mixed_fields()"""
        a = (C.c_uint64 * 3)()
        self._lib.ntscsim_debug_mixed_tables(self._h, a)
        return [int(x) for x in a]

    def debug_force_generic(self, on=True):
        self._lib.ntscsim_debug_force_generic(self._h, 1 if on else 0)

    def debug_no_fast_decode(self, on=True):
        """on: True/1 = template PRESET kernels, 2 = two-launch (VCR half / TV half) VHS decoder."""
        self._lib.ntscsim_debug_no_fast_decode(self._h, int(on))

    def last_kernels(self):
        """Names of the kernel forms the last fields / fields422 / batch call enqueued, in order."""
        buf = C.create_string_buffer(1024)
        n = self._lib.ntscsim_debug_last_kernels(self._h, buf, len(buf))
        if n < 0:
            raise RuntimeError("ntscsim_debug_last_kernels: %d" % n)
        return [k for k in buf.value.decode().split(";") if k]

    def last_decoder_lds(self):
        """Bytes of dynamic LDS of the last decoder launch: the luma delay ring (4096), or 0 where the luma path re-reads."""
        n = self._lib.ntscsim_debug_last_decoder_lds(self._h)
        if n < 0:
            raise RuntimeError("ntscsim_debug_last_decoder_lds: %d" % n)
        return n

    def debug_set_warmup(self, luma_draws, chroma_draws):
        self._lib.ntscsim_debug_set_warmup(self._h, int(luma_draws), int(chroma_draws))

    def debug_composite(self, n_fields, width, height):
        import numpy as np
        lslot = (height + 1) // 2
        a = np.zeros((n_fields, lslot, width), dtype=np.int32)
        rc = self._lib.ntscsim_debug_read_composite(
            self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size)
        self._chk(rc, "ntscsim_debug_read_composite")
        return a


def blend_frame_times(params, n_frames, rate_num, rate_den=1):
    """Times, in output periods, of the frames of a constant-rate clip: pts = frame number, time base =
    rate_den / rate_num (ntscsim_blend_frame_time, frameblend.cpp:100-110)."""
    L = lib()
    return [float(L.ntscsim_blend_frame_time(k, int(rate_den), int(rate_num), C.byref(params))) for k in range(n_frames)]


def blend_plan(params, times, first=0, last=None):
    """The planner (ntscsim_blend_plan_*, frameblend.cpp:929-1028) over a whole clip, with the tool's read-ahead of
    30 periods (:910): a list, one entry per output period in [first, last), of (ids, weight16) -- ids are indices
    into `times`.  last = None: the tool's own end of the clip (ntscsim_blend_clip_periods).  Host only: no GPU."""
    L = lib()
    times = [float(t) for t in times]
    if last is None:
        last = int(L.ntscsim_blend_clip_periods(times[-1]))
    h = C.c_void_p()
    rc = L.ntscsim_blend_plan_create(C.byref(params), C.byref(h))
    if rc != _capi.OK:
        raise NtscsimError(rc, "ntscsim_blend_plan_create")
    out = []
    try:
        cap = 64
        ids, w16 = (C.c_int64 * cap)(), (C.c_uint32 * cap)()
        n = C.c_int(0)
        pushed = 1
        L.ntscsim_blend_plan_push(h, times[0])
        for current in range(int(last)):
            while pushed < len(times) and times[pushed - 1] < current + 30:
                L.ntscsim_blend_plan_push(h, times[pushed])
                pushed += 1
            rc = L.ntscsim_blend_plan_next(h, current, ids, w16, cap, C.byref(n), None)
            if rc == _capi.E_SIZE:
                cap = n.value
                ids, w16 = (C.c_int64 * cap)(), (C.c_uint32 * cap)()
                rc = L.ntscsim_blend_plan_next(h, current, ids, w16, cap, C.byref(n), None)
            if rc != _capi.OK:
                raise NtscsimError(rc, "ntscsim_blend_plan_next(%d)" % current)
            if current >= first:
                out.append(([int(ids[k]) for k in range(n.value)], [int(w16[k]) for k in range(n.value)]))
    finally:
        L.ntscsim_blend_plan_destroy(h)
    return out


class FrameBlender:
    """The frameblend stage (ntscsim_blend_*): resamples a clip to the output rate by blending the source frames
    that overlap each output period.  `flags` are frameblend's switches, e.g. ("-gamma", "ntsc").  sim: share the
    context of a FieldSimulator (the outputs can then be handed to sim.fields() on the same stream); otherwise a
    context of its own is created.  torch is used only for device memory and streams."""

    def __init__(self, flags=(), device=0, params=None, sim=None):
        self.params = params if params is not None else _capi.make_blend_params(flags)
        self._own = sim is None
        self.sim = sim if sim is not None else FieldSimulator(device=device)
        self._lib = self.sim._lib
        self.sim._chk(self._lib.ntscsim_blend_bind(self.sim._h, C.byref(self.params)), "ntscsim_blend_bind")

    def close(self):
        if self._own and self.sim is not None:
            self.sim.close()
        self.sim = None

    def frame_times(self, n_frames, rate_num, rate_den=1):
        return blend_frame_times(self.params, n_frames, rate_num, rate_den)

    def plan(self, times, first=0, last=None):
        return blend_plan(self.params, times, first, last)

    def n_out(self, times):
        """Output periods the tool renders for a clip with these frame times (frameblend.cpp:924-927)."""
        return int(self._lib.ntscsim_blend_clip_periods(float(times[-1])))

    @staticmethod
    def _descs(jobs, ptr, linesize):
        """jobs: list of (dst, [(src, weight16), ...]), frames [H, W, 4] uint8 with contiguous pixels."""
        arr = (_capi.BlendDesc * len(jobs))()
        keep = []
        for d, (dst, taps) in zip(arr, jobs):
            h, w = dst.shape[0], dst.shape[1]
            t = (_capi.BlendTap * max(1, len(taps)))()
            for k, (src, w16) in enumerate(taps):
                assert tuple(src.shape) == (h, w, 4)
                t[k].src_dev, t[k].src_linesize, t[k].weight16 = ptr(src), linesize(src), int(w16)
            keep.append(t)
            d.dst_dev, d.dst_linesize, d.width, d.height, d.n_taps, d.taps = ptr(dst), linesize(dst), w, h, len(taps), t
        return arr, keep

    def blend_frames(self, jobs, stream=None):
        """ntscsim_blend_frames_device: jobs = [(dst, [(src, weight16), ...]), ...] of torch uint8 CUDA tensors
        [H, W, 4] (any row stride).  Enqueues; does not synchronise."""
        arr, keep = self._descs(jobs, lambda t: t.data_ptr(), lambda t: t.stride(0))
        if stream is None:
            stream = self.sim._torch_stream()
        rc = self._lib.ntscsim_blend_frames_device(self.sim._h, arr, len(jobs), C.c_void_p(stream))
        self.sim._chk(rc, "ntscsim_blend_frames_device")

    def blend_frames_host(self, jobs):
        """ntscsim_blend_frames_host: the same on numpy uint8 arrays [H, W, 4].  Synchronous."""
        arr, keep = self._descs(jobs, lambda a: a.ctypes.data, lambda a: a.strides[0])
        self.sim._chk(self._lib.ntscsim_blend_frames_host(self.sim._h, arr, len(jobs)), "ntscsim_blend_frames_host")

    def blend(self, src, times, out, first=0, last=None, stream=None):
        """ntscsim_blend_clip_device: src torch uint8 CUDA [N, H, W, 4] with frame times `times` (output periods),
        out [last - first, H, W, 4]; output period k lands in out[k - first].  Enqueues; does not synchronise."""
        n, h, w = src.shape[0], src.shape[1], src.shape[2]
        if last is None:
            last = first + out.shape[0]
        assert src.is_cuda and out.is_cuda and len(times) == n and out.shape[0] >= last - first
        assert tuple(out.shape[1:]) == (h, w, 4) and src.stride(2) == 4 and out.stride(2) == 4
        sp = (C.c_void_p * n)(*[src.data_ptr() + j * src.stride(0) for j in range(n)])
        dp = (C.c_void_p * max(1, last - first))(*[out.data_ptr() + k * out.stride(0) for k in range(last - first)])
        tt = (C.c_double * n)(*[float(t) for t in times])
        if stream is None:
            stream = self.sim._torch_stream()
        rc = self._lib.ntscsim_blend_clip_device(self.sim._h, sp, src.stride(1), tt, n, dp, out.stride(1), w, h,
                                                 int(first), int(last), C.c_void_p(stream))
        self.sim._chk(rc, "ntscsim_blend_clip_device")

    def last_kernels(self):
        return self.sim.last_kernels()

    def sync(self):
        self.sim.sync()


class _LayerStage:
    """What ColorKeyer and FrameAverager share: a stage bound on a shared or owned FieldSimulator context whose frames are
    a destination and a list of layers.  A subclass names its C entry points (_NAME: ntscsim_<_NAME>_*), its ctypes
    descriptor and source types, and the uint64 field that tags a descriptor (_TAG)."""
    _NAME = _DESC = _SRC = _TAG = None

    def __init__(self, params, device, sim):
        self.params = params
        self._own = sim is None
        self.sim = sim if sim is not None else FieldSimulator(device=device)
        self._lib = self.sim._lib
        self._call("bind", C.byref(self.params))

    def _call(self, what, *args):
        name = "ntscsim_%s_%s" % (self._NAME, what)
        self.sim._chk(getattr(self._lib, name)(self.sim._h, *args), name)

    def close(self):
        if self._own and self.sim is not None:
            self.sim.close()
        self.sim = None

    @property
    def n_layers(self):
        return int(self.params.n_layers)

    @property
    def delay(self):
        return int(self.params.delay)

    def _descs(self, jobs, ptr, linesize):
        """jobs: list of (dst, [src or None per layer], tag), frames [H, W, 4] uint8 with contiguous pixels."""
        arr = (self._DESC * max(1, len(jobs)))()
        keep = []
        for d, (dst, srcs, tag) in zip(arr, jobs):
            h, w = dst.shape[0], dst.shape[1]
            t = (self._SRC * max(1, len(srcs)))()
            for k, src in enumerate(srcs):
                if src is not None:
                    assert tuple(src.shape) == (h, w, 4)
                    t[k].src_dev, t[k].src_linesize = ptr(src), linesize(src)
            keep.append(t)
            d.dst_dev, d.dst_linesize, d.width, d.height, d.n_layers, d.layers = ptr(dst), linesize(dst), w, h, len(srcs), t
            setattr(d, self._TAG, int(tag))
        return arr, keep

    def _frames_device(self, jobs, stream):
        arr, keep = self._descs(jobs, lambda t: t.data_ptr(), lambda t: t.stride(0))
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("frames_device", arr, len(jobs), C.c_void_p(stream))

    def _frames_host(self, jobs):
        arr, keep = self._descs(jobs, lambda a: a.ctypes.data, lambda a: a.strides[0])
        self._call("frames_host", arr, len(jobs))

    def _clip(self, ring, layers, out, ring_index, tag, stream):
        """The *_clip_device call; returns (ring_index, tag) behind the last frame."""
        T, nl = len(out), self.n_layers
        assert len(ring) == self.delay and len(layers) == nl and all(len(lay) == T for lay in layers)
        rp = (C.c_void_p * max(1, len(ring)))(*[r.data_ptr() for r in ring])
        sp = (C.c_void_p * max(1, nl * T))(*[(f.data_ptr() if f is not None else None) for lay in layers for f in lay])
        ls = (C.c_int32 * max(1, nl))()
        for k, lay in enumerate(layers):
            strides = set(f.stride(0) for f in lay if f is not None)
            assert len(strides) <= 1
            ls[k] = strides.pop() if strides else 4 * int(self.params.width)
        op = (C.c_void_p * max(1, T))(*[o.data_ptr() for o in out])
        ri, tg = C.c_int32(int(ring_index)), C.c_uint64(int(tag))
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("clip_device", rp, ring[0].stride(0) if len(ring) else 0, C.byref(ri), sp, ls, op,
                   out[0].stride(0) if T else 4 * int(self.params.width), T, C.byref(tg), C.c_void_p(stream))
        return int(ri.value), int(tg.value)

    def last_kernels(self):
        return self.sim.last_kernels()

    def sync(self):
        self.sim.sync()


class ColorKeyer(_LayerStage):
    """The colorkey stage (ntscsim_key_*): keys layers over a destination that is never cleared, as ffmpeg_colorkey
    does.  `argv` are the tool's switches, e.g. ("-d", "2", "-i", "bg", "-i", "fg", "-color", "0x00FF00", "-threshhold",
    "96"): every -i opens a layer (the name is only recorded) and the per-layer switches behind it apply to it.
    width / height: the frame size (the tool has no -height).  sim: share the context of a FieldSimulator (its outputs
    can then be keyed on the same stream without leaving device memory); otherwise a context of its own is created.
    torch is used only for device memory and streams."""
    _NAME, _DESC, _SRC, _TAG = "key", _capi.KeyDesc, _capi.KeySrc, "rand_pos"

    def __init__(self, argv=(), width=None, height=None, device=0, params=None, sim=None):
        super().__init__(params if params is not None else _capi.make_key_params(argv, width=width, height=height), device, sim)

    def rand_advance(self, pos, present=None):
        """ntscsim_key_rand_advance: the position of the rand() stream behind one output frame that starts at `pos`;
        present[l] false marks layer l as absent in that frame (default: all present)."""
        v = C.c_uint64(int(pos))
        pm = None
        if present is not None:
            assert len(present) == self.n_layers
            pm = (C.c_uint8 * max(1, self.n_layers))(*[1 if x else 0 for x in present])
        rc = self._lib.ntscsim_key_rand_advance(C.byref(self.params), pm, C.byref(v))
        if rc != _capi.OK:
            raise NtscsimError(rc, "ntscsim_key_rand_advance")
        return int(v.value)

    def key_frames(self, jobs, stream=None):
        """ntscsim_key_frames_device: jobs = [(dst, [src or None per layer], rand_pos), ...] of torch uint8 CUDA tensors
        [H, W, 4] (any row stride); dst is keyed in place.  Enqueues; does not synchronise."""
        self._frames_device(jobs, stream)

    def key_frames_host(self, jobs):
        """ntscsim_key_frames_host: the same on numpy uint8 arrays [H, W, 4].  Synchronous."""
        self._frames_host(jobs)

    def key_clip(self, ring, layers, out, ring_index=0, rand_pos=0, stream=None):
        """ntscsim_key_clip_device: ring = list of `delay` torch uint8 CUDA frames [H, W, 4] (the destination ring, kept
        between calls), layers = per layer a list of T frames (None: absent in that frame), out = list of T frames.
        Frames of one list share a row stride.  Returns (ring_index, rand_pos) behind the last frame, to be handed to
        the next call.  Enqueues; does not synchronise."""
        return self._clip(ring, layers, out, ring_index, rand_pos, stream)

    def debug_set_bits_limit(self, nbytes):
        """ntscsim_key_debug_set_bits_limit: bound on the hit bits of one launch (0: the default)."""
        self._call("debug_set_bits_limit", int(nbytes))


class FrameAverager(_LayerStage):
    """The average_delay stage (ntscsim_avg_*): averages layers into a destination that is never cleared, as
    ffmpeg_average_delay does.  `argv` are the tool's switches, e.g. ("-d", "2", "-i", "a", "-n", "64"): every -i opens a
    layer (the name is only recorded) and -n behind it sets its level (256 = all new, 0 = all old).  width / height:
    the frame size (the tool has no -height).  sim: share the context of a FieldSimulator (its outputs can then be
    averaged on the same stream without leaving device memory); otherwise a context of its own is created.  torch is
    used only for device memory and streams."""
    _NAME, _DESC, _SRC, _TAG = "avg", _capi.AvgDesc, _capi.AvgSrc, "field"

    def __init__(self, argv=(), width=None, height=None, device=0, params=None, sim=None):
        super().__init__(params if params is not None else _capi.make_avg_params(argv, width=width, height=height), device, sim)

    def average_frames(self, jobs, stream=None):
        """ntscsim_avg_frames_device: jobs = [(dst, [src or None per layer], field), ...] of torch uint8 CUDA tensors
        [H, W, 4] (any row stride); dst is averaged in place.  Enqueues; does not synchronise."""
        self._frames_device(jobs, stream)

    def average_frames_host(self, jobs):
        """ntscsim_avg_frames_host: the same on numpy uint8 arrays [H, W, 4].  Synchronous."""
        self._frames_host(jobs)

    def average_clip(self, ring, layers, out, ring_index=0, field=0, stream=None):
        """ntscsim_avg_clip_device: ring = list of `delay` torch uint8 CUDA frames [H, W, 4] (the destination ring, kept
        between calls), layers = per layer a list of T frames (None: absent in that frame), out = list of T frames.
        Frames of one list share a row stride.  Returns (ring_index, field) behind the last frame, to be handed to the
        next call.  Enqueues; does not synchronise."""
        return self._clip(ring, layers, out, ring_index, field, stream)


class Scanimator:
    """The scanimate stage (ntscsim_scan_*): the CRT raster re-scan effect of ffmpeg_scanimate.  `flags` are the tool's
    switches, e.g. ("-inntsc", "-tvstd", "pal"); width / height: the output size (the tool has no -height).  A source
    frame may have any size: the tool's (params.src_width x src_height) is only what its own input scaler produces.
    sim: share the context of a FieldSimulator; otherwise a context of its own is created.  torch is used only for
    device memory and streams.  Frames are uint8 [H, W, 4] with contiguous pixels and any row stride."""

    def __init__(self, flags=(), width=None, height=None, sim=None, device=0, params=None):
        self.params = params if params is not None else _capi.make_scan_params(flags, width=width, height=height)
        self._own = sim is None
        self.sim = sim if sim is not None else FieldSimulator(device=device)
        self._lib = self.sim._lib
        self._call("bind", C.byref(self.params))

    def _call(self, what, *args):
        name = "ntscsim_scan_%s" % what
        self.sim._chk(getattr(self._lib, name)(self.sim._h, *args), name)

    def close(self):
        if self._own and self.sim is not None:
            self.sim.close()
        self.sim = None

    def _descs(self, jobs, ptr, linesize):
        w, h = int(self.params.output_width), int(self.params.output_height)
        arr = (_capi.ScanDesc * max(1, len(jobs)))()
        for d, (dst, src, fieldno) in zip(arr, jobs):
            if tuple(dst.shape) != (h, w, 4):           # the descriptor carries no destination size: the bound one is meant
                raise NtscsimError(_capi.E_SIZE, "scan: destination %r is not the bound %dx%d" % (tuple(dst.shape), w, h))
            assert len(src.shape) == 3 and src.shape[2] == 4
            d.dst_dev, d.dst_linesize = ptr(dst), linesize(dst)
            d.src_dev, d.src_linesize, d.src_width, d.src_height = ptr(src), linesize(src), src.shape[1], src.shape[0]
            d.fieldno = int(fieldno)
        return arr

    def scan_frames(self, jobs, stream=None):
        """ntscsim_scan_frames_device: jobs = [(dst, src, fieldno), ...] of torch uint8 CUDA tensors.  Rows field ..
        of dst are written, field = (fieldno & 1) ^ 1.  Enqueues; does not synchronise."""
        arr = self._descs(jobs, lambda t: t.data_ptr(), lambda t: t.stride(0))
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("frames_device", arr, len(jobs), C.c_void_p(stream))

    def scan_frames_host(self, jobs):
        """ntscsim_scan_frames_host: the same on numpy uint8 arrays.  Synchronous."""
        arr = self._descs(jobs, lambda a: a.ctypes.data, lambda a: a.strides[0])
        self._call("frames_host", arr, len(jobs))

    def scan_clip(self, srcs, out, fieldno=0, stream=None):
        """ntscsim_scan_clip_device: srcs / out = lists of T torch uint8 CUDA frames (one source size and one row stride
        per list); out[t] becomes the field of fieldno + t, row 0 of the field == 1 outputs zeroed.  Returns the
        field number behind the last one.  Enqueues; does not synchronise."""
        T = len(out)
        assert len(srcs) == T
        w, h = int(self.params.output_width), int(self.params.output_height)
        for o in out:
            if tuple(o.shape) != (h, w, 4):
                raise NtscsimError(_capi.E_SIZE, "scan: output %r is not the bound %dx%d" % (tuple(o.shape), w, h))
        assert len(set((tuple(f.shape), f.stride(0)) for f in srcs)) <= 1 and len(set(o.stride(0) for o in out)) <= 1
        sp = (C.c_void_p * max(1, T))(*[f.data_ptr() for f in srcs])
        op = (C.c_void_p * max(1, T))(*[o.data_ptr() for o in out])
        fn = C.c_uint64(int(fieldno))
        if stream is None:
            stream = self.sim._torch_stream()
        sh, sw = (srcs[0].shape[0], srcs[0].shape[1]) if T else (1, 1)
        self._call("clip_device", sp, srcs[0].stride(0) if T else 4, sw, sh, op, out[0].stride(0) if T else 4 * w, T,
                   C.byref(fn), C.c_void_p(stream))
        return int(fn.value)

    def last_kernels(self):
        """Synchronises: whether k_scan_splat spilled is read from a device counter."""
        return self.sim.last_kernels()

    def sync(self):
        self.sim.sync()

    def debug_keep_raster(self, on=True):
        self._call("debug_keep_raster", 1 if on else 0)

    def debug_raster(self):
        """The accumulator plane of the last descriptor of the last call (numpy uint32 [H, W]), before the >> 1 and
        the clamp; debug_keep_raster() first."""
        import numpy as np
        out = np.empty((int(self.params.output_height), int(self.params.output_width)), np.uint32)
        self._call("debug_raster", C.c_void_p(out.ctypes.data))
        return out

    def debug_set_window_rows(self, rows):
        """Caps the rows of the splat kernel's on-chip window (0: everything spills; negative: the default)."""
        self._call("debug_set_window_rows", int(rows))

    def debug_spill(self):
        """(workgroups of the last call that drew a dot, those of them that spilled)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._call("debug_spill", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)


class EdgeAligner:
    """The vhsled stage (ntscsim_led_*): lines up the left edge of the picture of every scanline, as ffmpeg_vhsled does.
    `flags` are the tool's switches (none of them changes a pixel); width / height: the frame size, 16 .. 3640 by
    16 .. 65536.  sim: share the context of a FieldSimulator (its outputs can then be aligned on the same stream
    without leaving device memory); otherwise a context of its own is created.  torch is used only for device memory
    and streams.  Frames are uint8 [H, W, 4] with contiguous pixels and any row stride."""

    def __init__(self, flags=(), width=None, height=None, sim=None, device=0, params=None):
        self.params = params if params is not None else _capi.make_led_params(flags, width=width, height=height)
        self._own = sim is None
        self.sim = sim if sim is not None else FieldSimulator(device=device)
        self._lib = self.sim._lib
        try:
            self._call("bind", C.byref(self.params))
        except Exception:
            self.close()
            raise

    def _call(self, what, *args):
        name = "ntscsim_led_%s" % what
        self.sim._chk(getattr(self._lib, name)(self.sim._h, *args), name)

    def close(self):
        if self._own and self.sim is not None:
            self.sim.close()
        self.sim = None

    @staticmethod
    def _descs(jobs, ptr, linesize):
        arr = (_capi.LedDesc * max(1, len(jobs)))()
        for d, (dst, src) in zip(arr, jobs):
            assert len(dst.shape) == 3 and dst.shape[2] == 4 and tuple(src.shape) == tuple(dst.shape)
            d.src_dev, d.src_linesize, d.dst_dev, d.dst_linesize = ptr(src), linesize(src), ptr(dst), linesize(dst)
            d.width, d.height = dst.shape[1], dst.shape[0]
        return arr

    def align_frames(self, jobs, stream=None):
        """ntscsim_led_frames_device: jobs = [(dst, src), ...] of torch uint8 CUDA tensors [H, W, 4]; dst becomes src
        with every row moved left by its smoothed edge.  One launch for all jobs that do not depend on each other.
        Enqueues; does not synchronise."""
        arr = self._descs(jobs, lambda t: t.data_ptr(), lambda t: t.stride(0))
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("frames_device", arr, len(jobs), C.c_void_p(stream))

    def align_frames_host(self, jobs):
        """ntscsim_led_frames_host: the same on numpy uint8 arrays.  Synchronous."""
        arr = self._descs(jobs, lambda a: a.ctypes.data, lambda a: a.strides[0])
        self._call("frames_host", arr, len(jobs))

    def debug_keep_edges(self, on=True):
        self._call("debug_keep_edges", 1 if on else 0)

    def edges(self, frame=0):
        """(e, x): per row the edge the scan found and the shift after smoothing (numpy int32 [H]) of frame `frame` of
        the last align_frames call; debug_keep_edges() first.  Synchronises."""
        import numpy as np
        h = int(self.params.height)
        e, x = np.empty(h, np.int32), np.empty(h, np.int32)
        self._call("debug_edges", int(frame), C.c_void_p(e.ctypes.data), C.c_void_p(x.ctypes.data))
        return e, x

    def last_kernels(self):
        return self.sim.last_kernels()

    def sync(self):
        self.sim.sync()


class AutoContrast:
    """The filmac stage (ntscsim_filmac_*): stretches the levels of every frame to full range, following the darkest
    block mean and the brightest pixel from frame to frame, as filmac does.  `flags` are the tool's switches; -gamma
    is the one that changes a byte (levels are then measured and stretched in linear light).  width / height: the
    frame size, 16 .. 16384 each.  sim: share the context of a FieldSimulator; otherwise a context of its own is
    created.  The level state lives on the device and carries from frame to frame and from call to call; calls must
    be ordered by the caller (one stream).  Frames are uint8 [H, W, 4] with contiguous pixels and any row stride."""

    def __init__(self, flags=(), width=None, height=None, sim=None, device=0, params=None):
        self.params = params if params is not None else _capi.make_filmac_params(flags, width=width, height=height)
        self._own = sim is None
        self.sim = sim if sim is not None else FieldSimulator(device=device)
        self._lib = self.sim._lib
        try:
            self._call("bind", C.byref(self.params))
        except Exception:
            self.close()
            raise

    def _call(self, what, *args):
        name = "ntscsim_filmac_%s" % what
        self.sim._chk(getattr(self._lib, name)(self.sim._h, *args), name)

    def close(self):
        if self._own and self.sim is not None:
            self.sim.close()
        self.sim = None

    @staticmethod
    def _descs(jobs, ptr, linesize):
        arr = (_capi.FilmacDesc * max(1, len(jobs)))()
        for d, (dst, src) in zip(arr, jobs):
            assert len(dst.shape) == 3 and dst.shape[2] == 4 and tuple(src.shape) == tuple(dst.shape)
            d.src, d.src_linesize, d.dst, d.dst_linesize = ptr(src), linesize(src), ptr(dst), linesize(dst)
        return arr

    def _check_size(self, jobs):
        for dst, _ in jobs:
            if (dst.shape[0], dst.shape[1]) != (self.params.height, self.params.width):
                raise NtscsimError(_capi.E_SIZE, "a frame of %dx%d on a stage bound to %dx%d"
                                   % (dst.shape[1], dst.shape[0], self.params.width, self.params.height))

    def stretch_frames(self, jobs, stream=None):
        """ntscsim_filmac_frames_device: jobs = [(dst, src), ...] of torch uint8 CUDA tensors [H, W, 4], in clip order;
        dst may be src.  Five launches for all jobs that do not depend on each other.  Enqueues; does not synchronise."""
        self._check_size(jobs)
        arr = self._descs(jobs, lambda t: t.data_ptr(), lambda t: t.stride(0))
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("frames_device", arr, len(jobs), C.c_void_p(stream))

    def stretch_frames_host(self, jobs):
        """ntscsim_filmac_frames_host: the same on numpy uint8 arrays.  Synchronous."""
        self._check_size(jobs)
        arr = self._descs(jobs, lambda a: a.ctypes.data, lambda a: a.strides[0])
        self._call("frames_host", arr, len(jobs))

    def reset(self):
        """The tool's start: the next frame sets the levels.  Synchronises."""
        self._call("reset")

    @property
    def state(self):
        """(init, final_minv, final_maxv).  Reading and writing synchronise."""
        s = _capi.FilmacState()
        self._call("get_state", C.byref(s))
        return bool(s.init), int(s.final_minv), int(s.final_maxv)

    @state.setter
    def state(self, value):
        s = _capi.FilmacState()
        s.init, s.final_minv, s.final_maxv = int(bool(value[0])), int(value[1]), int(value[2])
        self._call("set_state", C.byref(s))

    def levels(self, frame=0):
        """(minv, maxv, final_minv, final_maxv) of frame `frame` of the last stretch_frames call.  Synchronises."""
        out = (C.c_int64 * 4)()
        self._call("debug_levels", int(frame), out)
        return tuple(int(v) for v in out)

    def debug_time_kernels(self, on=True):
        self._call("debug_time_kernels", 1 if on else 0)

    def kernel_ms(self):
        """(k_filmac_stats, k_filmac_frame_levels, k_filmac_levels, k_filmac_tables, k_filmac_apply) milliseconds of the
        last stretch_frames call; debug_time_kernels() first.  Synchronises."""
        out = (C.c_float * 5)()
        self._call("debug_kernel_ms", out)
        return tuple(float(v) for v in out)

    def last_kernels(self):
        return self.sim.last_kernels()

    def sync(self):
        self.sim.sync()


class AudioChain:
    """The VHS audio chain of ffmpeg_ntsc / ffmpeg_to_composite (ntscsim_audio_*): composite_audio_process() on
    interleaved int16, bit-identical to the tool, the hiss draws included.  params: ntscsim_audio_params
    (_capi.make_audio_params(flags)[0]) or None with `flags` / `tool`.  sim: share the context -- and with it the
    rand() position -- of a FieldSimulator; otherwise a context of its own is created.  The filter states and the
    sample count live on the device and carry from block to block and from call to call; calls must be ordered by the
    caller (one stream)."""

    def __init__(self, params=None, cli=None, device=0, flags=(), tool="ntsc", sim=None):
        if params is None:
            params = _capi.make_audio_params(flags, tool)[0]
        elif not isinstance(params, _capi.AudioParams):                         # (ntscsim_params, ntscsim_cli)
            ap = _capi.AudioParams()
            rc = _capi.lib().ntscsim_audio_params_from_cli(C.byref(ap), C.byref(params), C.byref(cli))
            if rc != _capi.OK:
                raise NtscsimError(rc, "ntscsim_audio_params_from_cli")
            params = ap
        self.params = params
        self.channels = int(params.channels)
        self._own = sim is None
        self.sim = sim if sim is not None else FieldSimulator(device=device)
        self._lib = self.sim._lib
        try:
            self._call("bind", C.byref(self.params))
        except Exception:
            self.close()
            raise

    def _call(self, what, *args):
        name = "ntscsim_audio_%s" % what
        self.sim._chk(getattr(self._lib, name)(self.sim._h, *args), name)

    def close(self):
        if self._own and self.sim is not None:
            self.sim.close()
        self.sim = None

    def process(self, src, dst, blocks=None, stream=None):
        """ntscsim_audio_device: src, dst are torch int16 CUDA tensors [frames, channels] (or flat), contiguous.
        blocks: [(frames, rng_pos or None), ...] cutting them into the call's descriptors in order (None: one block at
        the ctx's rand() position).  Enqueues; does not synchronise."""
        ch = self.channels
        total = src.numel() // ch
        assert src.is_contiguous() and dst.is_contiguous() and dst.numel() == src.numel()
        if blocks is None:
            blocks = [(total, None)]
        assert sum(b[0] for b in blocks) == total
        arr = (_capi.AudioDesc * max(1, len(blocks)))()
        at = 0
        for d, (frames, pos) in zip(arr, blocks):
            d.src = src.data_ptr() + at * ch * 2
            d.dst = dst.data_ptr() + at * ch * 2
            d.samples = int(frames)
            d.rng_pos = RNG_AUTO if pos is None else int(pos)
            at += int(frames)
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("device", arr, len(blocks), C.c_void_p(stream))

    STATE_BYTES = C.sizeof(_capi.AudioState)

    def process_tracks(self, srcs, dsts, states=None, blocks=None, stream=None):
        """ntscsim_audio_tracks_device: srcs, dsts are lists of torch int16 CUDA tensors, contiguous, one pair per
        independent track (lengths may differ).  states: None (every track starts from zeros and its end state is
        dropped) or a contiguous CUDA tensor of len(srcs) * STATE_BYTES bytes (zero_states()), updated in place.
        blocks: None, or per track None or a list shaped like process()'s.  Enqueues; does not synchronise."""
        ch, n = self.channels, len(srcs)
        assert len(dsts) == n and (blocks is None or len(blocks) == n)
        base = 0
        if states is not None:
            assert states.is_cuda and states.is_contiguous() and states.numel() * states.element_size() == n * self.STATE_BYTES
            base = states.data_ptr()
        tracks = (_capi.AudioTrack * max(1, n))()
        keep = []                                                               # the block arrays, alive until the call returns
        for t, (src, dst) in enumerate(zip(srcs, dsts)):
            total = src.numel() // ch
            assert src.is_contiguous() and dst.is_contiguous() and dst.numel() == src.numel()
            cut = blocks[t] if blocks is not None and blocks[t] is not None else [(total, None)]
            assert sum(b[0] for b in cut) == total
            arr = (_capi.AudioDesc * max(1, len(cut)))()
            at = 0
            for d, (frames, pos) in zip(arr, cut):
                d.src = src.data_ptr() + at * ch * 2
                d.dst = dst.data_ptr() + at * ch * 2
                d.samples = int(frames)
                d.rng_pos = RNG_AUTO if pos is None else int(pos)
                at += int(frames)
            keep.append(arr)
            tracks[t].blocks = arr
            tracks[t].n_blocks = len(cut)
            tracks[t].state = base + t * self.STATE_BYTES if states is not None else None
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("tracks_device", tracks, n, C.c_void_p(stream))

    def _mixed_tracks(self, sets, set_of, chunks, state_ptrs, blocks):
        """The argument arrays of a mixed call.  chunks[t]: (src pointer, dst pointer, int16 values) of track t."""
        n = len(chunks)
        assert len(set_of) == n and (blocks is None or len(blocks) == n)
        arr = (_capi.AudioParams * max(1, len(sets)))(*sets)
        tracks = (_capi.AudioMixedTrack * max(1, n))()
        keep = [arr]                                                            # the arrays, alive until the call returns
        for t, (src, dst, numel) in enumerate(chunks):
            ch = int(sets[set_of[t]].channels) if set_of[t] >= 0 else self.channels
            total = numel // ch
            assert total * ch == numel
            cut = blocks[t] if blocks is not None and blocks[t] is not None else [(total, None)]
            assert sum(b[0] for b in cut) == total
            descs = (_capi.AudioDesc * max(1, len(cut)))()
            at = 0
            for d, (frames, pos) in zip(descs, cut):
                d.src = src + at * ch * 2
                d.dst = dst + at * ch * 2
                d.samples = int(frames)
                d.rng_pos = RNG_AUTO if pos is None else int(pos)
                at += int(frames)
            keep.append(descs)
            tracks[t].blocks = descs
            tracks[t].n_blocks = len(cut)
            tracks[t].set = int(set_of[t])
            tracks[t].state = state_ptrs[t]
        return arr, tracks, keep

    def process_mixed_tracks(self, sets, set_of, srcs, dsts, states=None, blocks=None, stream=None):
        """ntscsim_audio_mixed_tracks_device: process_tracks() with parameters per track.  sets: a list of
        ntscsim_audio_params; set_of[t]: the index in it of track t's parameters, or -1 for the chain's own.  A track's
        tensors hold frames of ITS set's channels.  states, blocks: as process_tracks().  Enqueues; does not
        synchronise."""
        n = len(srcs)
        assert len(dsts) == n
        base = 0
        if states is not None:
            assert states.is_cuda and states.is_contiguous() and states.numel() * states.element_size() == n * self.STATE_BYTES
            base = states.data_ptr()
        for src, dst in zip(srcs, dsts):
            assert src.is_contiguous() and dst.is_contiguous() and dst.numel() == src.numel()
        chunks = [(s.data_ptr(), d.data_ptr(), s.numel()) for s, d in zip(srcs, dsts)]
        ptrs = [base + t * self.STATE_BYTES if states is not None else None for t in range(n)]
        arr, tracks, _keep = self._mixed_tracks(sets, set_of, chunks, ptrs, blocks)
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("mixed_tracks_device", arr, len(sets), tracks, n, C.c_void_p(stream))

    def host_mixed_tracks(self, sets, set_of, arrays, states=None, blocks=None):
        """ntscsim_audio_mixed_tracks_host: the mixed call in place on numpy int16 arrays whose samples are contiguous
        (any alignment), one per track.  states: None or a writeable numpy uint8 array of len(arrays) * STATE_BYTES
        bytes, updated in place.  Synchronous."""
        n = len(arrays)
        for a in arrays:
            assert a.dtype.str in ("<i2", "=i2") and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]
        base = 0
        if states is not None:
            assert states.dtype.itemsize == 1 and states.flags["C_CONTIGUOUS"] and states.flags["WRITEABLE"] and states.size == n * self.STATE_BYTES
            base = states.ctypes.data
        chunks = [(a.ctypes.data, a.ctypes.data, a.size) for a in arrays]
        ptrs = [base + t * self.STATE_BYTES if states is not None else None for t in range(n)]
        arr, tracks, _keep = self._mixed_tracks(sets, set_of, chunks, ptrs, blocks)
        self._call("mixed_tracks_host", arr, len(sets), tracks, n)

    def track_stats(self, n):
        """[(segments, repaired segments)] of tracks 0 .. n-1 of the last process_tracks() or process_mixed_tracks().
        Synchronises."""
        s = (_capi.AudioStats * max(1, int(n)))()
        self._call("debug_track_stats", s, int(n))
        return [(int(s[t].segments), int(s[t].repaired)) for t in range(int(n))]

    @classmethod
    def zero_states(cls, n, device="cuda"):
        """A state tensor for process_tracks(): n tracks at the tool's start (zeros, count 0)."""
        import torch
        return torch.zeros(int(n) * cls.STATE_BYTES, dtype=torch.uint8, device=device)

    @classmethod
    def track_state(cls, states, t):
        """(30 filter values as a tuple, sample count) of track t of a state tensor, as the `state` property gives
        the ctx's.  Synchronises (a copy to the host)."""
        import torch
        raw = states.view(torch.uint8).reshape(-1)[t * cls.STATE_BYTES:(t + 1) * cls.STATE_BYTES].cpu().numpy().tobytes()
        s = _capi.AudioState.from_buffer_copy(raw)
        v = [x for c in s.bandpass for x in c] + list(s.pre) + list(s.post) + list(s.boost)
        return tuple(v), int(s.count)

    @classmethod
    def set_track_state(cls, states, t, value):
        """Write (30 filter values, sample count) into track t of a state tensor."""
        import numpy as np
        import torch
        v, count = value
        raw = np.array(v, np.float64).tobytes() + np.array([count], np.uint64).tobytes()
        assert len(raw) == cls.STATE_BYTES
        states.view(torch.uint8).reshape(-1)[t * cls.STATE_BYTES:(t + 1) * cls.STATE_BYTES] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(states.device)

    def host(self, array):
        """ntscsim_audio_host: composite_audio_process(array, frames) in place on a numpy int16 array whose samples
        are contiguous (any alignment).  Synchronous."""
        assert array.dtype.str in ("<i2", "=i2") and array.flags["C_CONTIGUOUS"] and array.flags["WRITEABLE"]
        self._call("host", C.c_void_p(array.ctypes.data), array.size // self.channels)

    def reset(self):
        self._call("reset")

    @property
    def state(self):
        """(30 filter values as a tuple, sample count).  Reading and writing synchronise."""
        s = _capi.AudioState()
        self._call("get_state", C.byref(s))
        v = [x for c in s.bandpass for x in c] + list(s.pre) + list(s.post) + list(s.boost)
        return tuple(v), int(s.count)

    @state.setter
    def state(self, value):
        v, count = value
        s = _capi.AudioState()
        for c in range(2):
            for i in range(12):
                s.bandpass[c][i] = v[c * 12 + i]
        for i in range(2):
            s.pre[i], s.post[i], s.boost[i] = v[24 + i], v[26 + i], v[28 + i]
        s.count = int(count)
        self._call("set_state", C.byref(s))

    def set_plan(self, seg_len=0, warmup=0):
        """ntscsim_audio_debug_set_plan: (0, 0) restores the defaults; otherwise warmup is taken as given."""
        self._call("debug_set_plan", int(seg_len), int(warmup))

    def default_warmup(self):
        """72 tau of the high-pass, up to a multiple of 64 (csrc/audio_chain.hpp: audio_default_warmup)."""
        import math
        tau = self.params.rate / (2 * math.pi * self.params.highpass_hz)
        return (int(72.0 * tau) + 1 + 63) // 64 * 64

    def stats(self):
        """(segments, repaired segments) of the last call.  Synchronises."""
        s = _capi.AudioStats()
        self._call("debug_stats", C.byref(s))
        return int(s.segments), int(s.repaired)

    def pulses(self, count0, n):
        """The device's sync pulse counts of frames count0 .. count0 + n - 1, as a numpy uint8 array."""
        import numpy as np
        out = np.zeros(int(n), np.uint8)
        self._call("debug_pulses", int(count0), int(n), C.c_void_p(out.ctypes.data))
        return out

    def debug_time_kernels(self, on=True):
        self._call("debug_time_kernels", 1 if on else 0)

    def kernel_ms(self):
        """(draws and pulse counts, k_audio_segments, k_audio_verify_repair) milliseconds of the last call."""
        out = (C.c_float * 3)()
        self._call("debug_kernel_ms", out)
        return tuple(float(v) for v in out)

    def sync(self):
        self.sim.sync()


class Cassette:
    """ffmpeg_cassette's tape chain (ntscsim_cass_*): its composite_audio_process() on interleaved int16 stereo,
    bit-identical to the tool on the host that makes the call (the per-frame sin() is the host's libm), the hiss draws
    included.  params: ntscsim_cass_params (_capi.make_cass_params(flags)) or None with `flags`.  sim: share the context
    -- and with it the rand() position -- of a FieldSimulator; otherwise a context of its own is created.  Filter
    states, sample count and the FIR's history live on the device and carry from block to block and from call to call;
    calls must be ordered by the caller (one stream)."""

    channels = 2

    def __init__(self, params=None, device=0, flags=(), sim=None):
        if params is None:
            params = _capi.make_cass_params(flags)
        self.params = params
        self.taps = int(params.taps)
        self._own = sim is None
        self.sim = sim if sim is not None else FieldSimulator(device=device)
        self._lib = self.sim._lib
        try:
            self._call("bind", C.byref(self.params))
        except Exception:
            self.close()
            raise

    def _call(self, what, *args):
        name = "ntscsim_cass_%s" % what
        self.sim._chk(getattr(self._lib, name)(self.sim._h, *args), name)

    def close(self):
        if self._own and self.sim is not None:
            self.sim.close()
        self.sim = None

    def process(self, src, dst, blocks=None, stream=None):
        """ntscsim_cass_device: src, dst are torch int16 CUDA tensors [frames, 2] (or flat), contiguous.  blocks:
        [(frames, rng_pos or None), ...] cutting them into the call's descriptors in order (None: one block at the
        ctx's rand() position).  Enqueues; does not synchronise."""
        total = src.numel() // 2
        assert src.is_contiguous() and dst.is_contiguous() and dst.numel() == src.numel()
        if blocks is None:
            blocks = [(total, None)]
        assert sum(b[0] for b in blocks) == total
        arr = (_capi.CassDesc * max(1, len(blocks)))()
        at = 0
        for d, (frames, pos) in zip(arr, blocks):
            d.src = src.data_ptr() + at * 4
            d.dst = dst.data_ptr() + at * 4
            d.samples = int(frames)
            d.rng_pos = RNG_AUTO if pos is None else int(pos)
            at += int(frames)
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("device", arr, len(blocks), C.c_void_p(stream))

    STATE_BYTES = C.sizeof(_capi.CassState)

    def process_tracks(self, srcs, dsts, counts, states=None, blocks=None, stream=None):
        """ntscsim_cass_tracks_device: srcs, dsts are lists of torch int16 CUDA tensors, contiguous, one pair per
        independent track (lengths may differ).  counts: the sample count of every track's first frame, which the caller
        keeps (the sines are made from it on the host; the count inside a state is not read).  states: None (every
        track starts from zeros and its end state is dropped) or a contiguous CUDA tensor of len(srcs) * STATE_BYTES
        bytes (zero_states()), updated in place.  blocks: None, or per track None or a list shaped like process()'s.
        Enqueues; does not synchronise."""
        n = len(srcs)
        assert len(dsts) == n and len(counts) == n and (blocks is None or len(blocks) == n)
        base = 0
        if states is not None:
            assert states.is_cuda and states.is_contiguous() and states.numel() * states.element_size() == n * self.STATE_BYTES
            base = states.data_ptr()
        tracks = (_capi.CassTrack * max(1, n))()
        keep = []                                                               # the block arrays, alive until the call returns
        for t, (src, dst) in enumerate(zip(srcs, dsts)):
            total = src.numel() // 2
            assert src.is_contiguous() and dst.is_contiguous() and dst.numel() == src.numel()
            cut = blocks[t] if blocks is not None and blocks[t] is not None else [(total, None)]
            assert sum(b[0] for b in cut) == total
            arr = (_capi.CassDesc * max(1, len(cut)))()
            at = 0
            for d, (frames, pos) in zip(arr, cut):
                d.src = src.data_ptr() + at * 4
                d.dst = dst.data_ptr() + at * 4
                d.samples = int(frames)
                d.rng_pos = RNG_AUTO if pos is None else int(pos)
                at += int(frames)
            keep.append(arr)
            tracks[t].blocks = arr
            tracks[t].n_blocks = len(cut)
            tracks[t].count = int(counts[t])
            tracks[t].state = base + t * self.STATE_BYTES if states is not None else None
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("tracks_device", tracks, n, C.c_void_p(stream))

    def _mixed_tracks(self, sets, set_of, chunks, counts, state_ptrs, blocks):
        """The argument arrays of a mixed call.  chunks[t]: (src pointer, dst pointer, int16 values) of track t."""
        n = len(chunks)
        assert len(set_of) == n and len(counts) == n and (blocks is None or len(blocks) == n)
        arr = (_capi.CassParams * max(1, len(sets)))(*sets)
        tracks = (_capi.CassMixedTrack * max(1, n))()
        keep = [arr]                                                            # the arrays, alive until the call returns
        for t, (src, dst, numel) in enumerate(chunks):
            total = numel // 2
            assert total * 2 == numel
            cut = blocks[t] if blocks is not None and blocks[t] is not None else [(total, None)]
            assert sum(b[0] for b in cut) == total
            descs = (_capi.CassDesc * max(1, len(cut)))()
            at = 0
            for d, (frames, pos) in zip(descs, cut):
                d.src = src + at * 4
                d.dst = dst + at * 4
                d.samples = int(frames)
                d.rng_pos = RNG_AUTO if pos is None else int(pos)
                at += int(frames)
            keep.append(descs)
            tracks[t].blocks = descs
            tracks[t].n_blocks = len(cut)
            tracks[t].set = int(set_of[t])
            tracks[t].count = int(counts[t])
            tracks[t].state = state_ptrs[t]
        return arr, tracks, keep

    def process_mixed_tracks(self, sets, set_of, srcs, dsts, counts, states=None, blocks=None, stream=None):
        """ntscsim_cass_mixed_tracks_device: process_tracks() with parameters per track.  sets: a list of
        ntscsim_cass_params; set_of[t]: the index in it of track t's parameters, or -1 for the chain's own.  counts,
        states, blocks: as process_tracks(); the history of a track's state has the length of ITS set's taps - 1.
        Enqueues; does not synchronise."""
        n = len(srcs)
        assert len(dsts) == n
        base = 0
        if states is not None:
            assert states.is_cuda and states.is_contiguous() and states.numel() * states.element_size() == n * self.STATE_BYTES
            base = states.data_ptr()
        for src, dst in zip(srcs, dsts):
            assert src.is_contiguous() and dst.is_contiguous() and dst.numel() == src.numel()
        chunks = [(s.data_ptr(), d.data_ptr(), s.numel()) for s, d in zip(srcs, dsts)]
        ptrs = [base + t * self.STATE_BYTES if states is not None else None for t in range(n)]
        arr, tracks, _keep = self._mixed_tracks(sets, set_of, chunks, counts, ptrs, blocks)
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("mixed_tracks_device", arr, len(sets), tracks, n, C.c_void_p(stream))

    def host_mixed_tracks(self, sets, set_of, arrays, counts, states=None, blocks=None):
        """ntscsim_cass_mixed_tracks_host: the mixed call in place on numpy int16 arrays whose samples are contiguous
        (any alignment), one per track.  states: None or a writeable numpy uint8 array of len(arrays) * STATE_BYTES
        bytes, updated in place.  Synchronous."""
        n = len(arrays)
        for a in arrays:
            assert a.dtype.str in ("<i2", "=i2") and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]
        base = 0
        if states is not None:
            assert states.dtype.itemsize == 1 and states.flags["C_CONTIGUOUS"] and states.flags["WRITEABLE"] and states.size == n * self.STATE_BYTES
            base = states.ctypes.data
        chunks = [(a.ctypes.data, a.ctypes.data, a.size) for a in arrays]
        ptrs = [base + t * self.STATE_BYTES if states is not None else None for t in range(n)]
        arr, tracks, _keep = self._mixed_tracks(sets, set_of, chunks, counts, ptrs, blocks)
        self._call("mixed_tracks_host", arr, len(sets), tracks, n)

    def track_stats(self, n):
        """[(segments, segments the front repaired, segments the back repaired)] of tracks 0 .. n-1 of the last
        process_tracks() or process_mixed_tracks().  Synchronises."""
        s = (_capi.CassStats * max(1, int(n)))()
        self._call("debug_track_stats", s, int(n))
        return [(int(s[t].segments), int(s[t].repaired_front), int(s[t].repaired_back)) for t in range(int(n))]

    def tilt_frames(self):
        """Sines the last call's host fill evaluated: for process_tracks() the union of the tracks' count ranges."""
        out = C.c_uint64(0)
        self._call("debug_tilt_frames", C.byref(out))
        return int(out.value)

    @classmethod
    def zero_states(cls, n, device="cuda"):
        """A state tensor for process_tracks(): n tracks at the tool's start (zeros)."""
        import torch
        return torch.zeros(int(n) * cls.STATE_BYTES, dtype=torch.uint8, device=device)

    def track_state(self, states, t):
        """(28 filter values, sample count, history of taps - 1 pairs) of track t of a state tensor, as the `state`
        property gives the ctx's.  Synchronises (a copy to the host)."""
        import torch
        raw = states.view(torch.uint8).reshape(-1)[t * self.STATE_BYTES:(t + 1) * self.STATE_BYTES].cpu().numpy().tobytes()
        s = _capi.CassState.from_buffer_copy(raw)
        v = [x for c in s.bandpass for x in c] + list(s.pre) + list(s.post)
        return tuple(v), int(s.count), tuple((s.history[k][0], s.history[k][1]) for k in range(self.taps - 1))

    def set_track_state(self, states, t, value):
        """Write (28 filter values, sample count, history pairs) into track t of a state tensor; the rest of the
        history is zeroed and taps is the bound one."""
        import torch
        v, count, hist = value
        s = _capi.CassState()
        for c in range(2):
            for i in range(12):
                s.bandpass[c][i] = v[c * 12 + i]
        for i in range(2):
            s.pre[i], s.post[i] = v[24 + i], v[26 + i]
        s.count = int(count)
        s.taps = self.taps
        for k, (a, b) in enumerate(hist):
            s.history[k][0], s.history[k][1] = a, b
        states.view(torch.uint8).reshape(-1)[t * self.STATE_BYTES:(t + 1) * self.STATE_BYTES] = torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).to(states.device)

    def host(self, array):
        """ntscsim_cass_host: composite_audio_process(array, frames) in place on a numpy int16 array whose samples are
        contiguous (any alignment).  Synchronous."""
        assert array.dtype.str in ("<i2", "=i2") and array.flags["C_CONTIGUOUS"] and array.flags["WRITEABLE"]
        self._call("host", C.c_void_p(array.ctypes.data), array.size // 2)

    def reset(self):
        self._call("reset")

    @property
    def state(self):
        """(28 filter values as a tuple: 24 band-pass, pre[2], post[2]; sample count; the FIR's history as a tuple of
        taps - 1 (left, right) pairs).  Reading and writing synchronise."""
        s = _capi.CassState()
        self._call("get_state", C.byref(s))
        v = [x for c in s.bandpass for x in c] + list(s.pre) + list(s.post)
        return tuple(v), int(s.count), tuple((s.history[k][0], s.history[k][1]) for k in range(self.taps - 1))

    @state.setter
    def state(self, value):
        v, count, hist = value
        s = _capi.CassState()
        for c in range(2):
            for i in range(12):
                s.bandpass[c][i] = v[c * 12 + i]
        for i in range(2):
            s.pre[i], s.post[i] = v[24 + i], v[26 + i]
        s.count = int(count)
        s.taps = self.taps
        for k, (a, b) in enumerate(hist):
            s.history[k][0], s.history[k][1] = a, b
        self._call("set_state", C.byref(s))

    def set_plan(self, seg_len=0, warmup_front=0, warmup_back=0):
        """ntscsim_cass_debug_set_plan: (0, 0, 0) restores the defaults; otherwise the warm-ups are taken as given."""
        self._call("debug_set_plan", int(seg_len), int(warmup_front), int(warmup_back))

    def default_warmups(self):
        """(front: 72 tau of the high-pass, up to a multiple of 64; back: csrc/cass_chain.hpp CASS_DEFAULT_BACK_WARMUP)"""
        import math
        tau = self.params.rate / (2 * math.pi * self.params.highpass_hz)
        return (int(72.0 * tau) + 1 + 63) // 64 * 64, 64

    def stats(self):
        """(segments, segments the front repaired, segments the back repaired) of the last call.  Synchronises."""
        s = _capi.CassStats()
        self._call("debug_stats", C.byref(s))
        return int(s.segments), int(s.repaired_front), int(s.repaired_back)

    def debug_time_kernels(self, on=True):
        self._call("debug_time_kernels", 1 if on else 0)

    def kernel_ms(self):
        """(host sin fill, its upload, k_audio_hiss, k_cass_front, k_cass_front_verify, k_cass_conv, k_cass_back,
        k_cass_back_verify) milliseconds of the last call; after process_tracks() the same slots hold the
        k_cass_track_* kernels'."""
        out = (C.c_float * 8)()
        self._call("debug_kernel_ms", out)
        return tuple(float(v) for v in out)

    def sync(self):
        self.sim.sync()


class _PixelMapStage:
    """What Posterizer and ColorMapper share: the bound context, the descriptor arrays and the two frame calls.
    `flags` are the tool's switches.  width / height: the frame size, 1 .. 16384 each (the tools have no -height).
    sim: share the context of a FieldSimulator; otherwise a context of its own is created.  Frames are uint8
    [H, W, 4] with contiguous pixels and any row stride; a job is a tuple of frames in the order of _FRAMES."""
    _STAGE = None                           # "post" / "cmap": ntscsim_<stage>_*
    _DESC = None
    _FRAMES = ("dst", "src")

    def __init__(self, flags=(), width=None, height=None, sim=None, device=0, params=None):
        self.params = params if params is not None else _capi.make_pixmap_params(self._STAGE, flags, width=width, height=height)
        self._own = sim is None
        self.sim = sim if sim is not None else FieldSimulator(device=device)
        self._lib = self.sim._lib
        try:
            self._call("bind", C.byref(self.params))
        except Exception:
            self.close()
            raise

    def _call(self, what, *args):
        name = "ntscsim_%s_%s" % (self._STAGE, what)
        self.sim._chk(getattr(self._lib, name)(self.sim._h, *args), name)

    def close(self):
        if self._own and self.sim is not None:
            self.sim.close()
        self.sim = None

    def _fill(self, d, job, ptr, linesize):
        """one descriptor from one job; the frames named in _FRAMES are set here, a stage adds the rest"""
        for name, t in zip(self._FRAMES, job):
            if t is None:
                continue
            if len(t.shape) != 3 or t.shape[2] != 4 or (t.shape[0], t.shape[1]) != (self.params.height, self.params.width):
                raise NtscsimError(_capi.E_SIZE, "a frame of shape %r on a stage bound to %dx%d"
                                   % (tuple(t.shape), self.params.width, self.params.height))
            setattr(d, name, ptr(t))
            setattr(d, name + "_linesize", linesize(t))

    def _descs(self, jobs, ptr, linesize):
        arr = (self._DESC * max(1, len(jobs)))()
        for d, job in zip(arr, jobs):
            self._fill(d, job, ptr, linesize)
        return arr

    def frames(self, jobs, stream=None):
        """ntscsim_<stage>_frames_device on torch uint8 CUDA tensors, in order; dst may be src.  One launch group for
        all jobs that do not depend on each other.  Enqueues; does not synchronise."""
        arr = self._descs(jobs, lambda t: t.data_ptr(), lambda t: t.stride(0))
        if stream is None:
            stream = self.sim._torch_stream()
        self._call("frames_device", arr, len(jobs), C.c_void_p(stream))

    def frames_host(self, jobs):
        """ntscsim_<stage>_frames_host: the same on numpy uint8 arrays.  Synchronous."""
        arr = self._descs(jobs, lambda a: a.ctypes.data, lambda a: a.strides[0])
        self._call("frames_host", arr, len(jobs))

    def last_kernels(self):
        return self.sim.last_kernels()

    def sync(self):
        self.sim.sync()


class Posterizer(_PixelMapStage):
    """The posterize stage (ntscsim_post_*): every byte of a pixel, alpha included, keeps the `-threshhold` high bits
    of the input it came from, as ffmpeg_posterize does.  jobs = [(dst, src, layer), ...] or [(dst, src), ...]; layer
    is an index into the -i list of `flags` (default: the last input, whose frame is the tool's output)."""
    _STAGE = "post"
    _DESC = _capi.PostDesc

    def _fill(self, d, job, ptr, linesize):
        super()._fill(d, job, ptr, linesize)
        d.layer = int(job[2]) if len(job) > 2 else self.params.n_layers - 1


class ColorMapper(_PixelMapStage):
    """The colormap stage (ntscsim_cmap_*): the green byte of a pixel selects the output pixel from a 256-entry table,
    which is taken from the middle row of a map frame, as ffmpeg_colormap does with its second input.  jobs =
    [(dst, src, map), ...] in clip order; map None: there is no second input, the table stays as it is.  The table
    lives on the device and carries from job to job and from call to call; calls must be ordered by the caller (one
    stream)."""
    _STAGE = "cmap"
    _DESC = _capi.CmapDesc
    _FRAMES = ("dst", "src", "map")

    def reset(self):
        """The tool's start: table[i] = i * 0x01010101.  Synchronises."""
        self._call("reset")

    @property
    def table(self):
        """The 256 pixels of the table as a numpy uint32 array.  Reading and writing synchronise."""
        import numpy as np
        out = (C.c_uint32 * 256)()
        self._call("get_table", out)
        return np.frombuffer(out, dtype=np.uint32).copy()

    @table.setter
    def table(self, value):
        vals = [int(x) for x in value]
        if len(vals) != 256:
            raise NtscsimError(_capi.E_ARG, "a table of %d entries" % len(vals))
        self._call("set_table", (C.c_uint32 * 256)(*vals))


class Pool:
    """ntscsim_pool_*: one context per GPU (an ordinal may repeat), a run of host frames dealt block-cyclically
    over them -- byte-identical to one FieldSimulator.frames_host() over the whole run."""

    def __init__(self, flags=(), devices=(0,), params=None, block_frames=None):
        self.params = params if params is not None else make_params(flags)
        self._lib = lib()
        h = C.c_void_p()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        rc = self._lib.ntscsim_pool_create(C.byref(self.params), devs, len(devices), C.byref(h))
        if rc != _capi.OK:
            raise NtscsimError(rc, "ntscsim_pool_create(%r)" % (list(devices),))
        self._h = h
        if block_frames is not None:
            rc = self._lib.ntscsim_pool_set_block(self._h, int(block_frames))
            if rc != _capi.OK:
                raise NtscsimError(rc, "ntscsim_pool_set_block")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ntscsim_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return int(self._lib.ntscsim_pool_size(self._h))

    @property
    def rng_pos(self):
        return int(self._lib.ntscsim_pool_get_rng_pos(self._h))

    @rng_pos.setter
    def rng_pos(self, pos):
        self._lib.ntscsim_pool_set_rng_pos(self._h, int(pos))

    def frames_host(self, dst, src, first_fieldno=0, bob=True, chunk_frames=0):
        """src numpy uint8 [N, H, W, 4], dst [2N, H, W, 4] (as FieldSimulator.frames_host)."""
        n, h, w = src.shape[:3]
        assert src.flags.c_contiguous and dst.flags.c_contiguous and dst.shape == (2 * n, h, w, 4)
        u8p = C.POINTER(C.c_uint8)
        rc = self._lib.ntscsim_pool_frames_host(self._h, src.ctypes.data_as(u8p), src.strides[0], src.strides[1], n,
                                                dst.ctypes.data_as(u8p), dst.strides[0], dst.strides[1], w, h,
                                                int(first_fieldno), DESC_BOB if bob else 0, int(chunk_frames))
        if rc != _capi.OK:
            raise NtscsimError(rc, "ntscsim_pool_frames_host: %s" % self._lib.ntscsim_pool_last_error(self._h).decode())


class Raw28Decoder:
    """The raw-composite decoder (ffmpeg_raw28ntsc): one decode() = one run of the tool on a capture."""

    def __init__(self, flags=(), device=0, opts=None):
        self._lib = lib()
        self.opts = opts if opts is not None else _capi.make_raw28_opts(flags)
        w, h, sl = C.c_int(), C.c_int(), C.c_int()
        rc = self._lib.ntscsim_raw28_geometry(C.byref(self.opts), C.byref(w), C.byref(h), C.byref(sl))
        if rc != _capi.OK:
            raise NtscsimError(rc, "ntscsim_raw28_geometry")
        self.width, self.height, self.scanline = w.value, h.value, sl.value
        hnd = C.c_void_p()
        rc = self._lib.ntscsim_raw28_create(C.byref(self.opts), int(device), C.byref(hnd))
        if rc != _capi.OK:
            raise NtscsimError(rc, "ntscsim_raw28_create")
        self._h = hnd

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ntscsim_raw28_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode(self, capture, frames, max_fields=None):
        """capture: numpy uint8 (host) or CUDA uint8 tensor; frames: CUDA uint8 tensor
        [F, height, >= 4*width].  Returns the number of fields decoded."""
        n = C.c_int()
        mf = int(frames.shape[0] if max_fields is None else max_fields)
        if hasattr(capture, "data_ptr"):
            fn, ptr, ns = self._lib.ntscsim_raw28_decode_device, capture.data_ptr(), capture.numel()
        else:
            fn, ptr, ns = self._lib.ntscsim_raw28_decode, capture.ctypes.data, capture.size
        rc = fn(self._h, C.c_void_p(ptr), ns, C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1),
                mf, C.byref(n))
        if rc != _capi.OK:
            raise NtscsimError(rc, self._lib.ntscsim_raw28_last_error(self._h).decode())
        return n.value

    def stream_reset(self):
        rc = self._lib.ntscsim_raw28_stream_reset(self._h)
        if rc != _capi.OK:
            raise NtscsimError(rc, "ntscsim_raw28_stream_reset")

    def stream_push(self, samples, frames, final=False, max_fields=None):
        """samples: numpy uint8 (host), a CUDA uint8 tensor, or None / empty; frames: CUDA uint8 tensor
        [F, height, >= 4*width].  Returns the number of fields this push wrote to frames[0:]."""
        n = C.c_int()
        mf = int(frames.shape[0] if max_fields is None else max_fields)
        if samples is None:
            ptr, ns, dev = None, 0, 0
        elif hasattr(samples, "data_ptr"):
            import torch
            if samples.dtype != torch.uint8 or not samples.is_contiguous():
                raise TypeError("stream_push: a CUDA tensor of samples must be contiguous uint8 (one byte per sample)")
            ptr, ns, dev = samples.data_ptr(), samples.numel(), 1
        else:
            import numpy as np
            keep = np.ascontiguousarray(samples)      # (a strided view would push the bytes in between)
            if keep.dtype != np.uint8:
                raise TypeError("stream_push: samples must be uint8 (one byte per sample), got %s" % keep.dtype)
            ptr, ns, dev = keep.ctypes.data, keep.size, 0
        rc = self._lib.ntscsim_raw28_stream_push(self._h, C.c_void_p(ptr), ns, dev, 1 if final else 0,
                                                 C.c_void_p(frames.data_ptr()), frames.stride(0), frames.stride(1),
                                                 mf, C.byref(n))
        if rc != _capi.OK:
            raise NtscsimError(rc, self._lib.ntscsim_raw28_last_error(self._h).decode())
        return n.value

    def levels(self):
        b, w, p = C.c_double(), C.c_double(), C.c_uint64()
        self._lib.ntscsim_raw28_get_levels(self._h, C.byref(b), C.byref(w), C.byref(p))
        return b.value, w.value, p.value

    def set_speculation(self, warm_lines=-1, chunk_samples=0):
        self._lib.ntscsim_raw28_debug_set_speculation(self._h, int(warm_lines), int(chunk_samples))

    def stats(self):
        a = (C.c_int64 * 16)()
        self._lib.ntscsim_raw28_debug_stats(self._h, a)
        return dict(zip(("front_rounds", "chunks_repaired", "tail_rounds", "sync_runs", "scanlines", "cal_pulses",
                         "us_front", "us_runs", "us_walk", "us_queue", "us_wait", "us_redo",
                         "pulses_past_stream", "zero_records", "compactions", "max_samples_held"), list(a)))

    def read_front(self, n):
        import numpy as np
        out = np.empty(n, np.uint8)
        rc = self._lib.ntscsim_raw28_debug_read_front(self._h, C.c_void_p(out.ctypes.data), n)
        if rc != _capi.OK:
            raise NtscsimError(rc, "ntscsim_raw28_debug_read_front")
        return out


_host_blocks = {}


def host_alloc_array(shape, align_offset=0):
    """A uint8 array of `shape` in pinned memory from ntscsim_host_alloc(), starting `align_offset` bytes into the
    block (tests: frames that do not start on a page boundary).  Free with host_free_array()."""
    import numpy as np
    n = int(np.prod(shape))
    p = lib().ntscsim_host_alloc(n + int(align_offset))
    if not p:
        raise MemoryError("ntscsim_host_alloc(%d)" % n)
    buf = (C.c_uint8 * (n + int(align_offset))).from_address(p)
    a = np.frombuffer(buf, dtype=np.uint8)[int(align_offset):].reshape(shape)
    _host_blocks[a.ctypes.data] = p
    return a


def host_free_array(a):
    p = _host_blocks.pop(a.ctypes.data, None)
    if p:
        lib().ntscsim_host_free(p)
