/*
 * ntscsim.h -- C ABI of the MI355X-native NTSC composite / VHS field simulator.
 *
 * This is the drop-in boundary for ONE hot path of joncampbell123/composite-video-simulator:
 * the per-field function
 *
 *     void composite_layer(AVFrame *dst, AVFrame *src, InputFile&, unsigned field,
 *                          unsigned long long fieldno)          ffmpeg_ntsc.cpp:1570-1921
 *
 * called once per output field from the field loop at ffmpeg_ntsc.cpp:2229, together with the
 * ~35 process-wide globals it reads (ffmpeg_ntsc.cpp:205-214, :756-809) and the libc rand()
 * stream it consumes.  Everything here is plain C: pointers, sizes, PODs.  No torch / HIP types
 * appear in any signature; a HIP stream is passed as an opaque void*.
 *
 * The reference has no plugin API -- the "interface" is the function signature above plus the
 * globals -- so the mapping is:
 *
 *   reference                                   | this header
 *   --------------------------------------------+------------------------------------------
 *   globals set by parse_argv() :972-1282       | struct ntscsim_params + ntscsim_params_parse_argv()
 *   preset_NTSC()/preset_PAL() :815-831         | ntscsim_params_init() / "-tvstd" flag
 *   composite_layer(dst,src,_,field,fieldno)    | ntscsim_field()            (host AVFrame planes)
 *   N calls of composite_layer in the loop :2202 | ntscsim_fields_device()   (batched, HBM resident)
 *   process-wide rand() state (never seeded)    | explicit 64-bit stream position per field
 *   bob line doubling :2233-2257                | NTSCSIM_DESC_BOB flag of ntscsim_field_desc
 *   silent `return` on bad frames :1578-1583    | negative error codes
 */
#ifndef NTSCSIM_H
#define NTSCSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTSCSIM_ABI_VERSION 1

/* ---- error codes (the reference returns silently, ffmpeg_ntsc.cpp:1578-1583) ---- */
enum {
    NTSCSIM_OK          = 0,
    NTSCSIM_E_ARG       = -1,  /* NULL pointer / bad argument                              */
    NTSCSIM_E_SIZE      = -2,  /* linesize < 4*width, size mismatch, width/height too small */
    NTSCSIM_E_NODEV     = -3,  /* no HIP device / HIP runtime unavailable                   */
    NTSCSIM_E_HIP       = -4,  /* a HIP call failed (see ntscsim_last_error)                */
    NTSCSIM_E_NOMEM     = -5,
    NTSCSIM_E_PARAM     = -6,  /* params outside the supported domain                       */
    NTSCSIM_E_FLAG      = -7,  /* unknown switch / bad value (reference: "return 1")        */
    NTSCSIM_E_HELP      = -8,  /* -h / -help was given                                      */
    NTSCSIM_E_INTERNAL  = -9
};

enum { NTSCSIM_TV_NTSC = 0, NTSCSIM_TV_PAL = 1 };
enum { NTSCSIM_VHS_SP = 0, NTSCSIM_VHS_LP = 1, NTSCSIM_VHS_EP = 2 }; /* ffmpeg_ntsc.cpp:801-805 */

/*
 * Immutable snapshot of the globals composite_layer() reads.  Field names follow the
 * reference's global names; the comment gives file:line of the global and its default.
 */
typedef struct ntscsim_params {
    uint32_t struct_size;                 /* = sizeof(ntscsim_params); versions the struct      */
    int32_t  tv_standard;                 /* output_ntsc/output_pal :209-210; NTSCSIM_TV_NTSC    */
    int32_t  output_width;                /* :207  720                                          */
    int32_t  output_height;               /* :208  480 (576 PAL)                                */
    int32_t  video_scanline_phase_shift;        /* :213  180 (0|90|180|270)                     */
    int32_t  video_scanline_phase_shift_offset; /* :214  0                                      */
    double   composite_preemphasis;       /* :756  0                                            */
    double   composite_preemphasis_cut;   /* :757  1000000                                      */
    double   vhs_out_sharpen;             /* :759  1.5                                          */
    int32_t  vhs_head_switching;          /* :761  false (true with -vhs)                       */
    int32_t  _pad0;
    double   vhs_head_switching_point;    /* :762  1 - 4.51/262.5                               */
    double   vhs_head_switching_phase;    /* :763  0.99/262.5                                   */
    double   vhs_head_switching_phase_noise; /* :764 (1/500)/262.5                              */
    int32_t  composite_in_chroma_lowpass;       /* :766  true                                   */
    int32_t  composite_out_chroma_lowpass;      /* :767  true                                   */
    int32_t  composite_out_chroma_lowpass_lite; /* :768  true                                   */
    int32_t  video_yc_recombine;          /* :770  0  (parsed, unused by ffmpeg_ntsc L1)        */
    int32_t  video_chroma_noise;          /* :772  0                                            */
    int32_t  video_chroma_phase_noise;    /* :773  0                                            */
    int32_t  video_chroma_loss;           /* :774  0                                            */
    int32_t  video_noise;                 /* :775  2                                            */
    int32_t  subcarrier_amplitude;        /* :776  50                                           */
    int32_t  subcarrier_amplitude_back;   /* :777  50                                           */
    int32_t  emulating_vhs;               /* :791  false                                        */
    int32_t  nocolor_subcarrier;          /* :794  false                                        */
    int32_t  nocolor_subcarrier_after_yc_sep; /* :795 false (parsed, unused by ffmpeg_ntsc L1)  */
    int32_t  vhs_chroma_vert_blend;       /* :796  true                                         */
    int32_t  vhs_svideo_out;              /* :797  false                                        */
    int32_t  enable_composite_emulation;  /* :798  true (-nocomp clears it; L1 never tests it)  */
    int32_t  output_vhs_tape_speed;       /* :809  NTSCSIM_VHS_SP                               */
    int32_t  black_key_level_feedback;    /* ffmpeg_to_composite.cpp:322  -1 (variant only)      */
    double   vhs_out_sharpen_chroma;      /* ffmpeg_to_composite.cpp:271  0.85 (variant only)    */
    /* EXTENSION, not in the reference (SURVEY 0.3 / 8(f) "ext"): multipath ghosting on the
     * composite signal, between the luma-noise stage (:1644) and head switching (:1647):
     *   Y'[x] = Y[x] + ( sum_k ghost_gain[k] * Y[x - ghost_delay[k]] ) / 256      (Y[<0] = 0)
     * taps read the un-ghosted signal (FIR), C integer arithmetic.  ghost_taps = 0 (default)
     * disables it and leaves the output bit-identical to the reference.  BGRA path only.
     * (Speed: while every delay is at most 63 samples the taps are folded into the encoder
     * kernel; a longer delay costs a pass over the composite plane) */
    int32_t  ghost_taps;                  /* 0..NTSCSIM_MAX_GHOST_TAPS                           */
    int32_t  ghost_delay[4];              /* samples, 1..4096                                    */
    int32_t  ghost_gain[4];               /* 1/256 units, -256..256                              */
    int32_t  _pad1;
} ntscsim_params;
#define NTSCSIM_MAX_GHOST_TAPS 4

/* Host-side (L4/L2) settings parse_argv() also fills; not read by the field DSP. */
#define NTSCSIM_MAX_INPUTS 16
typedef struct ntscsim_cli {
    const char *input_paths[NTSCSIM_MAX_INPUTS]; /* -i (repeatable) :1012                       */
    int32_t     n_inputs;
    int32_t     frame_delay;                     /* -d :1003, 1..256, default 1                 */
    const char *output_path;                     /* -o :1017                                    */
    int32_t     use_422_colorspace;              /* -422 / -420 :1022-1027                      */
    /* audio-only flags are accepted for CLI compatibility and recorded, never used here */
    int32_t     emulating_preemphasis, emulating_deemphasis, output_vhs_hifi;
    double      output_audio_hiss_db, output_audio_linear_buzz, vhs_linear_high_boost;
    int32_t     output_video_as_interlaced;      /* ffmpeg_to_composite -vi / -vp :1399-1404 (default 0: bob) */
    int32_t     _pad;
} ntscsim_cli;

/* preset_NTSC() + the global initialisers (ffmpeg_ntsc.cpp:205-214, :756-809, :824-831). */
void ntscsim_params_init(ntscsim_params *p);
void ntscsim_cli_init(ntscsim_cli *c);

/*
 * Mirror of parse_argv() (ffmpeg_ntsc.cpp:972-1282): same switch names (any number of leading
 * '-'), same defaults, same preset side effects (-vhs :1141, -vhs-speed :1160, -comp-catv* :1077)
 * and the same post-parse derivation of subcarrier_amplitude_back (:1264-1265).
 * argv[0] is the program name, as in main().  `cli` may be NULL.  If `require_io` is non-zero the
 * "No output file / No input files specified" checks (:1271-1278) apply.
 * Returns NTSCSIM_OK, NTSCSIM_E_HELP (-h), or NTSCSIM_E_FLAG (reference: return 1).
 */
int ntscsim_params_parse_argv(ntscsim_params *p, ntscsim_cli *cli, int argc,
                              const char *const *argv, int require_io);

/*
 * The 8-bit YUV422P sibling tool, ffmpeg_to_composite.cpp: its global initialisers (:267-333 --
 * note the different head-switch defaults: one `phase` parameter = 1-4.51/262.5, noise 1/300 line)
 * and its parse_argv() (:1325-1639: no -d / -comp-catv4 / -vhs-head-switching-phase; adds
 * -bkey-feedback, -ss/-se/-t, -a/-v/-an/-vn, -vi/-vp; -vhs-head-switching-point sets the phase;
 * -comp-catv* = 1.5/2.5/4 at fsc/2; amplitude_back += 50*pre/4 (:1627)).
 */
void ntscsim_params_init_to_composite(ntscsim_params *p);
int  ntscsim_params_parse_argv_to_composite(ntscsim_params *p, ntscsim_cli *cli, int argc,
                                            const char *const *argv, int require_io);

/* Rejects parameter values for which the reference's own behaviour is undefined
 * (negative noise levels, subcarrier amplitude 0 -> division by zero at :1545, ...). */
int ntscsim_params_validate(const ntscsim_params *p);

/*
 * Number of libc rand() draws one composite_layer() call makes:
 *   [W*L if video_noise] + [4 if head switching with phase noise] + [2*W*L if chroma noise]
 *   + [L if chroma phase noise] + [L if chroma loss],   L = rows of this field.
 */
uint64_t ntscsim_rng_calls_per_field(const ntscsim_params *p, int width, int height,
                                     unsigned field);

/* glibc TYPE_3 rand() clone (stdlib/random_r.c, seed 1): draw `n` values starting at stream
 * position `pos` (0 = first rand() of the process) using O(log pos) jump-ahead. */
void ntscsim_rng_draw(uint64_t pos, size_t n, uint32_t *out);

/* ------------------------------------------------------------------------------------------ */

typedef struct ntscsim_ctx ntscsim_ctx;

/* Bind to HIP device `device` (ordinal), snapshot `p`.  Fails with NTSCSIM_E_NODEV when no
 * GPU is present: there is NO CPU fallback in this library.
 * Threading: a ctx (and the batches created from it) is NOT re-entrant -- one thread at a time
 * per ctx, like the reference's globals + process-wide rand(); use one ctx per thread / stream.
 * Work enqueued through one ctx is ordered by the caller's stream; its scratch is reused. */
int  ntscsim_create(const ntscsim_params *p, int device, ntscsim_ctx **out);
void ntscsim_destroy(ntscsim_ctx *ctx);
const char *ntscsim_strerror(int code);
const char *ntscsim_last_error(const ntscsim_ctx *ctx); /* text of the last HIP failure */

/*
 * Arithmetic mode of the BGRA path.
 *   NTSCSIM_MODE_EXACT  (default): fp64 filters in the reference's operation order, no FMA --
 *                       output bit-identical to composite_layer().
 *   NTSCSIM_MODE_FAST32: the same pipeline, integer stages and rand() stream, with the filters,
 *                       the colour matrices and the phase rotation in fp32 (FMA allowed).  Output
 *                       differs from the reference by at most 1 LSB per 8-bit channel on a small
 *                       fraction of pixels (bounds in tests/test_gpu_fast_mode.py).
 *   NTSCSIM_MODE_FLOAT:  the tolerance mode as a pipeline of its own (csrc/ntsc_float.hip): Y / I / Q and the composite
 *                       sample are fp32 from RGB -> YIQ to YIQ -> RGB -- no inter-stage (int), no int <-> float
 *                       conversion of the signal, FMA contraction on -- while the rand() stream, the noise accumulators,
 *                       head-switch geometry, phase-noise table and dropout stay the exact mode's integers.  Same stated
 *                       tolerance as FAST32 (at most 1 LSB per 8-bit channel; bounds and the measured share of exact
 *                       pixels in tests/test_gpu_fast_mode.py).  Default preset and the -vhs family with its standard
 *                       switches; other switch sets -- and the short launches of ntscsim_field() / ntscsim_submit() -- run
 *                       the FAST32 forms in this mode.
 */
enum { NTSCSIM_MODE_EXACT = 0, NTSCSIM_MODE_FAST32 = 1, NTSCSIM_MODE_FLOAT = 2 };
int ntscsim_set_mode(ntscsim_ctx *ctx, int mode);

/* Stream position of the next field processed through ntscsim_field() (starts at 0, advances
 * by ntscsim_rng_calls_per_field per call -- exactly the reference's process-wide rand()). */
uint64_t ntscsim_get_rng_pos(const ntscsim_ctx *ctx);
void     ntscsim_set_rng_pos(ntscsim_ctx *ctx, uint64_t pos);

/*
 * Drop-in for composite_layer() (ffmpeg_ntsc.cpp:1570).  HOST buffers, as an AVFrame holds them:
 *   src_bgra/src_linesize/src_interlaced/src_tff = srcframe->data[0], ->linesize[0],
 *                                                  ->interlaced_frame, ->top_field_first
 *   dst_bgra/dst_linesize/width/height           = dstframe->data[0], ->linesize[0], ->width, ->height
 * Only rows y = field, field+2, ... of dst are written (alpha byte 0, :1914); other rows are
 * untouched.  Synchronous.  Uses and advances the ctx's rand() stream position.
 * A dst frame the GPU can address -- memory declared with ntscsim_host_pin(), or pinned memory (ntscsim_host_frame_alloc /
 * ntscsim_av_frame_get_buffer of ntscsim_avframe.h / hipHostMalloc; the runtime is asked at every call, nothing is
 * registered or remembered) -- whose rows are 16-byte aligned is written by the kernels themselves; any other frame goes
 * through a device copy and a download.  Same bytes either way.  (The call runs encoder and decoder as wavefront ROLES of
 * one workgroup per 63 rows for the -vhs family and the default preset: DESIGN.md 1c; 4.8-5.8k calls per second at 720x486.)
 */
int ntscsim_field(ntscsim_ctx *ctx,
                  const uint8_t *src_bgra, int src_linesize, int src_interlaced, int src_tff,
                  uint8_t *dst_bgra, int dst_linesize,
                  int width, int height, unsigned field, uint64_t fieldno);

/*
 * ASYNCHRONOUS drop-in for composite_layer() (ntscsim_submit / ntscsim_wait).
 *
 * The reference's loop calls composite_layer(ring[idx], in.rgb, in, (current&1)^1, current) at
 * ffmpeg_ntsc.cpp:2229, then line-doubles (:2233-2257), converts (:2266) and encodes the frame before it
 * composites the next field.  One synchronous field per call leaves the GPU 98 % idle (a field is four
 * workgroups of work).  ntscsim_submit() takes the same arguments, returns at once with a ticket, and the
 * ctx coalesces submitted fields into launches of `depth` fields; ntscsim_wait(ticket) returns when that
 * field's rows are in the caller's dst frame.  The caller moves everything it does with the frame after
 * composite_layer() (bob, sws_scale, output_frame :2233-2280) behind a wait issued `depth` fields later
 * (INTEGRATION.md section 1b shows the patch of the loop :2202-2282).
 *
 * Contract (what makes a sequence of submits + waits byte-identical to the same sequence of
 * ntscsim_field() calls on the same pointers, rand() position included):
 *   - src is SNAPSHOTTED by the call: when ntscsim_submit() returns the caller may overwrite src (the
 *     reference rewrites in.rgb with the next decoded frame, InputFile::frame_copy_scale :544-613).
 *     NTSCSIM_SUBMIT_SAME_SRC: src still holds the frame of the previous submit on this ctx (same
 *     pointer, geometry and content -- e.g. the second field of a frame): the device copy is reused and
 *     nothing is uploaded.  NTSCSIM_SUBMIT_SRC_STABLE: the caller promises to leave src alone until the
 *     ticket has been waited for; the call then does not wait for its upload either.
 *   - dst is written some time between submit and the return of ntscsim_wait(ticket): exactly the rows
 *     composite_layer() writes (rows field, field+2, ... :1910-1916; alpha 0), or with NTSCSIM_DESC_BOB
 *     in `flags` additionally the rows the loop's line doubling writes (:2233-2257: every row except, for
 *     field 0 and an even height or field 1 and an odd height, the last one).  Other rows are not touched.
 *     The caller must not read or write dst between submit and wait.  Fields in flight that share a dst
 *     frame are delivered in submit order.
 *   - tickets are issued in increasing order starting at 1; waiting for a ticket also completes every
 *     earlier one.  NTSCSIM_TICKET_ALL waits for everything submitted so far.
 *   - the rand() stream advances at SUBMIT time, in submit order (ntscsim_get_rng_pos() reflects it), so
 *     the noise is the one the synchronous loop draws.  ntscsim_field() / ntscsim_sync() on a ctx with
 *     fields in flight first wait for them; the other entry points must not be mixed in without
 *     ntscsim_wait(ctx, NTSCSIM_TICKET_ALL).
 *   - a launch happens when `depth` fields are pending, on ntscsim_flush(), or when a wait needs it; a
 *     change of width/height flushes first.
 * Host buffers (the same rules for ntscsim_submit() and ntscsim_submit422()): frames in PINNED memory are served
 * without a host memcpy -- DMA uploads, and the GPU writes the field rows straight into the caller's frame.  What
 * counts as pinned is deterministic (pin policy 1, the default):
 *   - memory the caller DECLARED with ntscsim_host_pin(ctx, base, len);
 *   - memory that is pinned already: ntscsim_host_alloc() / ntscsim_host_frame_alloc() (what the
 *     ntscsim_av_frame_get_buffer() helper of ntscsim_avframe.h backs an AVFrame with), hipHostMalloc, or the
 *     caller's own hipHostRegister -- the HIP runtime is asked (hipPointerGetAttributes), nothing is guessed;
 *   - buffers of at least min_pin_bytes (never below 64 KiB) that START ON A PAGE BOUNDARY and lie above the program
 *     break: registered in place on first sight (hipHostRegister, whole pages, cached per ctx).
 * Everything else -- ordinary malloc / av_malloc blocks, whatever the allocator (glibc, jemalloc, tcmalloc, a pool) --
 * goes through pinned staging rings: one memcpy each way, the delivery side on the engine's own copy threads.  Same
 * bytes either way.  Policy 2 (opt-in, glibc only: pin_caller_buffers = 2 / ntscsim_set_pin_policy) additionally
 * registers blocks that carry glibc's header of a chunk with a mapping of its own (IS_MMAPPED and a chunk size that
 * covers the frame) -- what av_frame_get_buffer() planes are while glibc's mmap threshold is below their size; it reads
 * the allocator's private word in front of the pointer and must not be used with another allocator.  Policy 0 stages
 * everything.
 * A pinned buffer must stay allocated until ntscsim_host_unpin() / ntscsim_destroy(): free()ing registered
 * memory while the registration lives is undefined (HIP).
 */
typedef struct ntscsim_submit_opts {
    uint32_t struct_size;          /* sizeof(ntscsim_submit_opts)                                       */
    int32_t  depth;                /* fields per launch, 1..4096; default 32                              */
    int32_t  slots;                /* fields that may be in flight (device frame ring), >= 2*depth;
                                      default 8*depth (0: the same).  ntscsim_submit() blocks (waits for the
                                      oldest launch) when the ring is full.  Waiting 4*depth fields behind
                                      the submits keeps uploads, kernels and deliveries of neighbouring
                                      launches overlapped (2*depth: ~10 % slower)                           */
    int32_t  lanes;                /* launches in flight side by side (own stream + scratch), 1..8; def. 3 */
    int32_t  pin_caller_buffers;   /* pin policy 0 | 1 | 2 (above); default 1                             */
    int32_t  _pad;
    size_t   min_pin_bytes;        /* default 256 KiB                                                     */
} ntscsim_submit_opts;
void ntscsim_submit_opts_init(ntscsim_submit_opts *o);
/* (Re)configure the engine; waits for everything in flight first.  Optional: the defaults apply otherwise. */
int  ntscsim_submit_configure(ntscsim_ctx *ctx, const ntscsim_submit_opts *o);

#define NTSCSIM_SUBMIT_SAME_SRC   0x10000u
#define NTSCSIM_SUBMIT_SRC_STABLE 0x20000u
#define NTSCSIM_TICKET_ALL        UINT64_MAX

/* Arguments as ntscsim_field(); `flags`: NTSCSIM_DESC_BOB | NTSCSIM_SUBMIT_*.  *ticket (may be NULL)
 * receives the ticket.  Errors are those of ntscsim_field(); a field that was refused consumes no ticket
 * and no rand() draws. */
int ntscsim_submit(ntscsim_ctx *ctx,
                   const uint8_t *src_bgra, int src_linesize, int src_interlaced, int src_tff,
                   uint8_t *dst_bgra, int dst_linesize,
                   int width, int height, unsigned field, uint64_t fieldno,
                   uint32_t flags, uint64_t *ticket);
/* Launch what is pending without waiting for it. */
int ntscsim_flush(ntscsim_ctx *ctx);
/* Block until `ticket` (and every earlier one) has been delivered.  Returns the first error of the
 * launches it had to complete (their fields are then lost), NTSCSIM_E_ARG for a ticket never issued. */
int ntscsim_wait(ntscsim_ctx *ctx, uint64_t ticket);
/* Declare [base, base + len) as the caller's own memory to pin: the pages it touches are registered with the GPU now
 * (hipHostRegister; memory that is pinned already is just noted) and every frame inside the range takes the
 * no-copy path from then on, wherever it starts.  The caller vouches that those pages hold nothing that is freed or
 * recycled while the declaration lives (an allocation of its own: a mmap, a large malloc block incl. its header page,
 * a frame pool).  Memory of the brk heap -- small malloc blocks, whose pages the allocator trims and recycles -- is refused
 * (NTSCSIM_E_ARG): a registration there makes the GPU fault sooner or later.
 * NTSCSIM_OK, NTSCSIM_E_ARG, NTSCSIM_E_HIP (registration refused; nothing changed). */
int ntscsim_host_pin(ntscsim_ctx *ctx, const void *base, size_t len);
/* Drop the registration that covers `base` (NULL: all of them) -- declared or made by the engine on its own --
 * after waiting for everything in flight: call before free()ing a frame buffer the engine has seen while the ctx
 * lives on. */
int ntscsim_host_unpin(ntscsim_ctx *ctx, const void *base);
/* Pinned host memory (hipHostMalloc, visible to every GPU of the process), page-aligned; NULL when it cannot be had.
 * No ctx needed: usable as the allocator behind av_buffer_create() (ntscsim_avframe.h). */
void *ntscsim_host_alloc(size_t bytes);
void  ntscsim_host_free(void *p);
/* The planes of one frame, laid out like av_frame_get_buffer(frame, align) does (linesize[k] = row_bytes[k] rounded
 * up to `align`, a power of two; every plane 64-byte aligned with 64 spare bytes), in ONE ntscsim_host_alloc()
 * block: data[k] / linesize[k] receive the planes, *base the block to hand to ntscsim_host_free(), *bytes (may be
 * NULL) its size. */
int   ntscsim_host_frame_alloc(int n_planes, const int *row_bytes, const int *rows, int align,
                               uint8_t **data, int *linesize, void **base, size_t *bytes);
/* Pin policy of this ctx's host-frame engines (0 | 1 | 2, see "Host buffers" above; default 1). */
int   ntscsim_set_pin_policy(ntscsim_ctx *ctx, int policy);
/* Counters since ntscsim_create(): [0] fields submitted, [1] launches, [2] source uploads, [3] uploads that
 * went through the staging ring, [4] fields delivered by the GPU into pinned caller frames, [5] fields
 * delivered through the staging ring, [6] live registrations, [7] submits that blocked on a full ring. */
void ntscsim_submit_stats(const ntscsim_ctx *ctx, uint64_t out[8]);

/*
 * The field loop (ffmpeg_ntsc.cpp:2202-2282) for a run of frames held in HOST memory, pipelined:
 * source frame j (j = 0..n_frames-1, BGRA, at src + j*src_frame_stride) produces output fields
 * first_fieldno + 2j and + 2j+1 (field parity (cur&1)^1, :2229), each into its own host frame at
 * dst + k*dst_frame_stride (k = 0..2*n_frames-1).  Destination frames start zeroed on the device;
 * with NTSCSIM_DESC_BOB in `flags` every row is then written except the one row bob leaves alone
 * (the frame-delay ring's, :2248).  Chunks of `chunk_frames` frames (<= 0: default 32) flow
 * through H2D copy | kernels | D2H copy on three HIP streams; the caller's buffers are pinned for
 * the duration of the call.  Synchronous; continues the ctx's rand() stream.
 */
int ntscsim_frames_host(ntscsim_ctx *ctx, const uint8_t *src, size_t src_frame_stride,
                        int src_linesize, int n_frames, uint8_t *dst, size_t dst_frame_stride,
                        int dst_linesize, int width, int height, uint64_t first_fieldno,
                        uint32_t flags, int chunk_frames);
/* `flags` bits for ntscsim_frames_host() in addition to NTSCSIM_DESC_*: deliver the output frames as
 * planar YUV instead of BGRA (each output frame at dst + k*dst_frame_stride holds the Y plane,
 * height rows of dst_linesize bytes, then U, then V, chroma rows of dst_linesize/2 bytes;
 * dst_linesize >= width, even). */
#define NTSCSIM_HOST_YUV420P 0x1000u
#define NTSCSIM_HOST_YUV422P 0x2000u

/*
 * Source scaling / pixel-format conversion before the field loop: what the tool does with
 * libswscale (sws_getContext(any format, any size -> BGRA W x H, SWS_BILINEAR), ffmpeg_ntsc.cpp
 * :573-583, sws_scale :603; ffmpeg_to_composite.cpp:1773).  libswscale is third-party code that
 * is not part of the reference tree: this is NOT a bit-clone of it (parity unpinned) but the
 * definition in csrc/ntsc_scale.hip -- pixel-centre-aligned bilinear resampling with 8-bit weights,
 * BT.601 limited-range YUV -> RGB, alpha 255 -- which tests/_libs.py restates and the GPU tests
 * compare bit for bit.
 */
#define NTSCSIM_SRC_BGRA    0
#define NTSCSIM_SRC_YUV420P 1
#define NTSCSIM_SRC_YUV422P 2
typedef struct ntscsim_scale_desc {
    const void *src_dev[3];     /* device pointers: BGRA uses [0]; planar YUV: Y, U, V            */
    void       *bgra_dev;       /* device pointer, BGRA frame of the call's width x height        */
    int32_t     src_linesize[3];
    int32_t     bgra_linesize;  /* >= 4*width, multiple of 4                                      */
    int32_t     src_width, src_height;   /* chroma planes: (w+1)/2 wide, (h+1)/2 (4:2:0) or h rows */
    int32_t     src_format;     /* NTSCSIM_SRC_*                                                  */
    int32_t     _pad;
} ntscsim_scale_desc;
int ntscsim_scale_to_bgra_device(ntscsim_ctx *ctx, const ntscsim_scale_desc *descs, int n,
                                 int width, int height, void *hip_stream);

/* Layout of one SOURCE frame in host memory for ntscsim_frames_host_scaled(): plane p starts
 * `plane_offset[p]` bytes into the frame and has rows of `linesize[p]` bytes. */
typedef struct ntscsim_host_source {
    int32_t format;             /* NTSCSIM_SRC_*                                                  */
    int32_t width, height;
    int32_t linesize[3];
    size_t  plane_offset[3];
    size_t  frame_bytes;        /* bytes of one frame that must travel to the device              */
} ntscsim_host_source;
/* ntscsim_frames_host() for sources of any size in BGRA / YUV420P / YUV422P: every chunk is uploaded
 * in its own format, converted to BGRA width x height on the GPU (ntscsim_scale_to_bgra_device) and
 * fed to the field loop; everything else as ntscsim_frames_host(). */
int ntscsim_frames_host_scaled(ntscsim_ctx *ctx, const ntscsim_host_source *source, const uint8_t *src,
                               size_t src_frame_stride, int n_frames, uint8_t *dst,
                               size_t dst_frame_stride, int dst_linesize, int width, int height,
                               uint64_t first_fieldno, uint32_t flags, int chunk_frames);

/* ---- several GPUs: a pool of contexts (BASELINE north_star: "partition the input stream
 * frame-round-robin") ------------------------------------------------------------------------------------
 * The loop :2202-2282 carries nothing from field to field but the position of the process-wide rand() stream,
 * and the draws per composite_layer() call do not depend on the pixels (ntscsim_rng_calls_per_field), so every
 * field's position is a closed form.  ntscsim_pool_frames_host() is ntscsim_frames_host() dealt over N
 * contexts: block b of `block` frames (default 32; ntscsim_pool_set_block) goes to context b mod N, every context
 * runs its own upload | kernels | download pipeline on its blocks from a host thread of its own, no data moves
 * between GPUs, and the frames are byte-identical to one context processing the whole run.  `devices` lists the
 * HIP ordinals, one context each (an ordinal may repeat: several contexts on one GPU -- how the tests run on a
 * one-GPU box); devices = NULL: the first n_devices visible GPUs (n_devices = 0: all of them).  The pool keeps its
 * own rand() position, advanced by every successful call like the ctx's.  One thread at a time per pool. */
typedef struct ntscsim_pool ntscsim_pool;
int  ntscsim_pool_create(const ntscsim_params *p, const int *devices, int n_devices, ntscsim_pool **out);
void ntscsim_pool_destroy(ntscsim_pool *pool);
int  ntscsim_pool_size(const ntscsim_pool *pool);
ntscsim_ctx *ntscsim_pool_ctx(ntscsim_pool *pool, int i);       /* context i, e.g. for ntscsim_set_mode() */
int  ntscsim_pool_set_block(ntscsim_pool *pool, int block_frames);
uint64_t ntscsim_pool_get_rng_pos(const ntscsim_pool *pool);
void ntscsim_pool_set_rng_pos(ntscsim_pool *pool, uint64_t pos);
const char *ntscsim_pool_last_error(const ntscsim_pool *pool);
int  ntscsim_pool_frames_host(ntscsim_pool *pool, const uint8_t *src, size_t src_frame_stride, int src_linesize,
                              int n_frames, uint8_t *dst, size_t dst_frame_stride, int dst_linesize,
                              int width, int height, uint64_t first_fieldno, uint32_t flags, int chunk_frames);

/* ---- batched, device-resident form (what the field loop :2202-2282 becomes) -------------- */

#define NTSCSIM_RNG_AUTO  UINT64_MAX   /* rng_pos: continue after the previous descriptor      */

typedef struct ntscsim_field_desc {
    const void *src_dev;      /* device pointer, BGRA frame, width x height                    */
    void       *dst_dev;      /* device pointer, BGRA frame, width x height                    */
    int32_t     src_linesize; /* bytes, >= 4*width, multiple of 4                              */
    int32_t     dst_linesize;
    uint32_t    field;        /* 0 | 1 : rows field, field+2, ...                              */
    uint32_t    flags;        /* NTSCSIM_DESC_* : bit0 src interlaced_frame, bit1 src
                                 top_field_first, bit8 bob line doubling (:2233-2257)          */
    uint64_t    fieldno;      /* `current` in the reference's loop                             */
    uint64_t    rng_pos;      /* rand() stream position at entry, or NTSCSIM_RNG_AUTO          */
} ntscsim_field_desc;

#define NTSCSIM_DESC_INTERLACED 1u
#define NTSCSIM_DESC_TFF        2u
#define NTSCSIM_DESC_BOB        0x100u   /* bob writes the OTHER field's rows of dst_dev: give every
                                            descriptor of a batch its own destination frame */

/*
 * Process `n` independent fields of one geometry.  All pointers in `descs` are DEVICE pointers
 * on the ctx's device; the descriptor array itself is host memory.  Work is enqueued on
 * `hip_stream` (a hipStream_t passed as void*, NULL = the ctx's own stream) and the call returns
 * without synchronising; scratch owned by the ctx is reused by the next call on the same ctx,
 * which is stream-ordered after this one.  descs[0].rng_pos == NTSCSIM_RNG_AUTO continues from
 * the ctx position; after a successful call the ctx position is the end of the last descriptor
 * (a call that fails leaves it where it was).
 * The descriptors of one call run concurrently: two of them may share a destination frame only as
 * its two fields (different `field`, neither with NTSCSIM_DESC_BOB); any other sharing is refused
 * with NTSCSIM_E_ARG.
 */
int ntscsim_fields_device(ntscsim_ctx *ctx, const ntscsim_field_desc *descs, int n,
                          int width, int height, void *hip_stream);

/*
 * Fields of one geometry, EACH WITH ITS OWN PARAMETERS: a fields call whose descriptors name a set of `sets` (a library
 * of stills, an augmentation run that gives every clip its own noise levels, tape speed, sharpening, head-switch point,
 * S-Video or composite out, pre-emphasis).  The call equals, in destination bytes and in the ctx's rand() position
 * afterwards, this sequence for i = 0 .. n-1 in order: a ctx made with ntscsim_create(&sets[descs[i].set]) has its
 * rand() position set to where descriptor i starts and runs ntscsim_fields_device(&descs[i].d, 1, width, height) -- but
 * the fields run side by side in ONE launch of each kernel however many sets there are (the decoder: one launch per
 * decoder class present -- no VCR, VCR with composite out, VCR with S-Video out), nothing waits for the device, and the
 * ctx's own parameters are neither read (except through set == -1) nor written.
 * rand() positions: NTSCSIM_RNG_AUTO continues after the previous descriptor in the call's order, which advanced by
 * ntscsim_rng_calls_per_field() of ITS set; descs[0] continues from the ctx's position; the position moves only when the
 * call succeeds, to the end of the last descriptor.
 * Destinations: shared across the whole call exactly as in ntscsim_fields_device() -- two descriptors may share a frame
 * only as its two fields, neither with NTSCSIM_DESC_BOB; the two may name different sets.
 * Modes: NTSCSIM_MODE_EXACT is bit-identical to the reference; NTSCSIM_MODE_FAST32 runs the same kernels with float
 * filter states; NTSCSIM_MODE_FLOAT runs the FAST32 forms here.  The call runs the generic kernels (every switch read at
 * run time), not the hand-tuned ones of the presets: a long run of fields on ONE preset is faster through
 * ntscsim_fields_device().  ntscsim_debug_set_warmup is honoured; ntscsim_debug_last_kernels names what
 * ran: k_mixed_setup, k_mixed_encode<RT>, k_mixed_decode<VHS,COMPOUT,RT> per class, k_mixed_bob.
 * ntscsim_set_profiling / ntscsim_get_timings_ms cover the call as they cover ntscsim_fields_device() (setup | encode |
 * decode, the decoder launches of all classes together).  The first call that names a draw layout (which of the noise
 * stages draw) or a chroma phase-noise level the ctx has not seen builds and uploads that table, synchronously; later
 * calls reuse it (ntscsim_debug_mixed_tables).
 * Refused before anything is enqueued or the position moves -- NTSCSIM_E_ARG / NTSCSIM_E_SIZE: everything
 * ntscsim_fields_device() refuses, its size limits taken for the call's scanline space (every set's fields start at a
 * multiple of 64 rows); a `set` outside -1 .. n_sets-1; n_sets < 0; a NULL `sets` that should hold something; a set some
 * descriptor names with a wrong struct_size.  NTSCSIM_E_PARAM: a set some descriptor names that
 * ntscsim_params_validate() refuses, or one with ghost_taps > 0 -- the ghosting extension is a pass over the whole
 * composite plane with call-wide taps and stays with the single-set calls.  Sets that no descriptor names are not looked
 * at.  n == 0 succeeds and does nothing.  `sets` and `descs` are host memory, consumed by the call.
 */
typedef struct ntscsim_mixed_field_desc {
    ntscsim_field_desc d;      /* as in ntscsim_fields_device                                     */
    int32_t            set;    /* index into `sets`; -1: the parameters the ctx was created with  */
    int32_t            _pad;
} ntscsim_mixed_field_desc;

int ntscsim_mixed_fields_device(ntscsim_ctx *ctx, const ntscsim_params *sets, int n_sets,
                                const ntscsim_mixed_field_desc *descs, int n,
                                int width, int height, void *hip_stream);

/*
 * Prepared batch: the same work as ntscsim_fields_device(), split into "validate the descriptors,
 * derive each field's rand() window, upload the records" (once) and "enqueue the kernel chain"
 * (any number of times, e.g. a clip that is re-rendered, or a ring of frame buffers that is
 * refilled in place).  The descriptors' pointers must stay valid.  A batch uses its ctx's scratch:
 * runs on one ctx are stream-ordered by the caller; use one ctx per stream to overlap batches.
 * ntscsim_batch_create() does not move the ctx's rand() position; every successful
 * ntscsim_batch_run() leaves it at the end of the batch's last descriptor.
 */
typedef struct ntscsim_batch ntscsim_batch;
int  ntscsim_batch_create(ntscsim_ctx *ctx, const ntscsim_field_desc *descs, int n,
                          int width, int height, ntscsim_batch **out);
int  ntscsim_batch_run(ntscsim_batch *batch, void *hip_stream);
void ntscsim_batch_destroy(ntscsim_batch *batch);

/* ---- the 8-bit YUV422P sibling: ffmpeg_to_composite.cpp --------------------------------------
 * One descriptor == one iteration of the loop at ffmpeg_to_composite.cpp:1783-1800:
 *   render_field(dst, src, field, ...) :1784   (skipped when src_dev[0] == NULL)
 *   black_key_feedback(dst, flt, ...)  :1787   (when params.black_key_level_feedback >= 0 and
 *                                               flt_dev[0] != NULL)
 *   composite_video_process(dst, field, fieldno) :1790, IN PLACE on the rows of `field` of the
 *                                               YUV422P frame dst (skipped with NTSCSIM_422_NOCOMP,
 *                                               the tool's -nocomp :1789)
 * Create the ctx from ntscsim_params_init_to_composite()/..._parse_argv_to_composite() parameters.
 * The reference's Y/C separator reads two bytes past the end of each luma row (`Y[x+2]`, :496).  This
 * implementation has the same memory semantics: for the last two positions of a row it reads the
 * caller's bytes dst[0][y*linesize + width], [.. + width + 1] when they lie inside the luma plane
 * (height * linesize bytes) -- with linesize < width + 2 those are the first bytes of the NEXT row,
 * which belongs to the other field -- and the value 16 otherwise (the frame's last row).
 * Consequences for batching: (1) fields that share a feedback frame must not be in the same batch
 * (frame-to-frame recurrence); (2) when dst_linesize[0] < width + 2, the two fields of one destination
 * frame must not be in the same batch either: one field's kernel would read bytes the other rewrites
 * in place, whereas the tool processes them one after the other (:1783-1800).  Such a batch is refused
 * with NTSCSIM_E_ARG; submit the fields in separate, stream-ordered calls (or pad the rows).
 */
#define NTSCSIM_422_INTERLACED 1u   /* src->interlaced_frame                                     */
#define NTSCSIM_422_TFF        2u   /* src->top_field_first                                      */
#define NTSCSIM_422_SRC420     4u   /* decoder format is YUV420P (:1005): src chroma is H/2 tall */
#define NTSCSIM_422_SECOND     8u   /* field_number - src_pts >= ticks_per_frame/2 (:1035)       */
#define NTSCSIM_422_NOCOMP     16u  /* -nocomp: render only                                      */

typedef struct ntscsim_field422_desc {
    void       *dst_dev[3];         /* Y, U, V of the YUV422P output frame (device pointers)     */
    const void *src_dev[3];         /* source frame for render_field, or NULL                    */
    void       *flt_dev[3];         /* black-key feedback frame, or NULL                         */
    int32_t     dst_linesize[3], src_linesize[3], flt_linesize[3];
    int32_t     src_height;         /* source frame height (its width is the output width)       */
    uint32_t    field;
    uint32_t    flags;              /* NTSCSIM_422_*                                             */
    uint32_t    _pad;
    uint64_t    fieldno;
    uint64_t    rng_pos;            /* or NTSCSIM_RNG_AUTO                                       */
} ntscsim_field422_desc;

int ntscsim_fields422_device(ntscsim_ctx *ctx, const ntscsim_field422_desc *descs, int n,
                             int width, int height, void *hip_stream);

/*
 * YUV422P fields of one geometry, EACH WITH ITS OWN PARAMETERS: ntscsim_mixed_fields_device() for the 8-bit tool -- a
 * fields422 call whose descriptors name a set of `sets` (a library of stills, an augmentation run that gives every clip
 * its own deck).  The call equals, in every byte of every destination and feedback plane and in the ctx's rand()
 * position afterwards, this sequence for i = 0 .. n-1 in order: a ctx made with ntscsim_create(&sets[descs[i].set]) has
 * its rand() position set to where descriptor i starts and runs ntscsim_fields422_device(&descs[i].d, 1, width, height)
 * -- render_field, black_key_feedback, composite_video_process, each with THAT set's switches
 * (black_key_level_feedback, video_yc_recombine, nocolor_subcarrier_after_yc_sep, tape speed, vhs_out_sharpen_chroma,
 * S-Video or composite out and everything else the 8-bit tool derives from a set) -- but the fields run side by side in
 * ONE launch of each kernel however many sets there are, nothing waits for the device, and the ctx's own parameters are
 * neither read (except through set == -1) nor written.
 * rand() positions: NTSCSIM_RNG_AUTO continues after the previous descriptor in the call's order, which advanced by
 * ntscsim_rng_calls_per_field_422() of ITS set and parity -- by nothing if it carries NTSCSIM_422_NOCOMP; descs[0]
 * continues from the ctx's position; the position moves only when the call succeeds, to the end of the last descriptor.
 * Destinations and the separator's two bytes past each luma row: the rules of ntscsim_fields422_device() hold across
 * the whole call, whatever sets the descriptors name -- the same frame and field twice is refused, both fields of one
 * frame with dst_linesize[0] < width + 2 are refused, overlapping frames that are not side-by-side views are refused.
 * Fields that share a FEEDBACK frame remain the caller's business, as there.
 * Modes and ghosting: the YUV422P path has no float forms (ntscsim_set_mode changes nothing here) and ignores
 * ghost_taps; so does this call.  All sets run the twelve-sweep kernel (every switch read at run time), not the
 * streamed forms of the presets: a long run of fields on ONE preset is faster through ntscsim_fields422_device()
 * (INTEGRATION.md).  ntscsim_debug_set_warmup is honoured; ntscsim_debug_last_kernels names what ran: k_mixed_setup,
 * k422_mixed_render when some descriptor has a source, k422_mixed_bkey when some descriptor keys, k422_mixed_halo when
 * some set's fields fill more than one workgroup of 63 rows, k422_mixed_process.  ntscsim_set_profiling /
 * ntscsim_get_timings_ms cover the call as they cover ntscsim_fields422_device() (setup | (empty) | process).  Tables
 * are cached as for ntscsim_mixed_fields_device(), per tool (ntscsim_debug_mixed_tables counts both tools' entries).
 * Refused before anything is enqueued or the position moves -- NTSCSIM_E_ARG / NTSCSIM_E_SIZE: everything
 * ntscsim_fields422_device() refuses (odd or out-of-range size, field > 1, NULL planes, short linesizes, a short
 * src_height, n > 65535, more than 2^30 rows -- taken for the call's padded scanline space: every set's fields start at
 * a multiple of 64 rows); a `set` outside -1 .. n_sets-1; n_sets < 0; a NULL `sets` that should hold something; a set
 * some descriptor names with a wrong struct_size.  NTSCSIM_E_PARAM: a set some descriptor names that
 * ntscsim_params_validate() refuses, or one with video_yc_recombine outside 0 .. 64.  Sets that no descriptor names are
 * not looked at.  n == 0 succeeds and does nothing.  `sets` and `descs` are host memory, consumed by the call.
 */
typedef struct ntscsim_mixed_field422_desc {
    ntscsim_field422_desc d;   /* as in ntscsim_fields422_device                                  */
    int32_t               set; /* index into `sets`; -1: the parameters the ctx was created with  */
    int32_t               _pad;
} ntscsim_mixed_field422_desc;

int ntscsim_mixed_fields422_device(ntscsim_ctx *ctx, const ntscsim_params *sets, int n_sets,
                                   const ntscsim_mixed_field422_desc *descs, int n,
                                   int width, int height, void *hip_stream);

/* Prepared batch of the same call (like ntscsim_batch_create/run/destroy above): descriptors are
 * validated, their rand() windows derived and everything uploaded once; every ntscsim_batch422_run()
 * is then only the kernel launches.  The descriptors' frame pointers must stay valid; runs on one ctx
 * are stream-ordered by the caller (one ctx per stream to overlap batches). */
typedef struct ntscsim_batch422 ntscsim_batch422;
int  ntscsim_batch422_create(ntscsim_ctx *ctx, const ntscsim_field422_desc *descs, int n,
                             int width, int height, ntscsim_batch422 **out);
int  ntscsim_batch422_run(ntscsim_batch422 *batch, void *hip_stream);
void ntscsim_batch422_destroy(ntscsim_batch422 *batch);

/*
 * The same loop iteration on HOST frames -- the drop-in for the tool's own call sequence
 *     render_field(output_avstream_video_frame, output_avstream_video_input_frame, field, video_field, tgt_pts);  :1784
 *     if (black_key_level_feedback >= 0) black_key_feedback(frame, output_avstream_video_filter_frame, ...);      :1787
 *     if (enable_composite_emulation) composite_video_process(frame, field, video_field);   :1790 (signature :629)
 *     output_frame(frame, video_field, field);          :1793 / :1796 -- its pixel work, the copy loops :1177-1236
 * of ffmpeg_to_composite.cpp:1783-1800, on the planes an AVFrame holds (data[0..2], linesize[0..2]).
 * ntscsim_field422() is synchronous (0.31-0.34 ms per 720x480 iteration: the streamed kernels of the -vhs family run as
 * four wavefront roles of one workgroup per 63 rows for such short launches); ntscsim_submit422() returns at once with a ticket and ntscsim_wait(ctx,
 * ticket) / ntscsim_flush(ctx) (above) complete / launch it -- a ctx serves ONE of the two tools, its tickets
 * come from one sequence.  include/ntscsim_avframe.h wraps both for real AVFrames; INTEGRATION.md section 5
 * has the patch of the loop and host/field_loop422.cpp is that loop in C++.
 *
 * Contract (what makes submits + waits byte-identical to the same sequence of synchronous calls, and those to
 * the tool's own calls on the same buffers; rand() position included):
 *   - `frame` is the tool's ONE persistent YUV422P frame, processed in place: the rows of `field` are written
 *     (render, key, composite emulation), the separator's read of two bytes behind each luma row (:496) sees
 *     the caller's own bytes as in ntscsim_fields422_device().  The engine keeps device copies of the frames it
 *     has seen: between calls the caller must not modify `frame` / `filter` -- or pass NTSCSIM_SUBMIT422_DIRTY
 *     with the next call (everything in flight is then delivered first and the frames are read again).
 *   - `src` (render_field's source: output_width wide, src_height rows, 4:2:2 or with NTSCSIM_422_SRC420 4:2:0)
 *     is SNAPSHOTTED by the call; data[0] == NULL: no render_field (the frame is processed as it stands).
 *     NTSCSIM_SUBMIT_SAME_SRC: src still holds the frame of the previous submit422 (second field of a frame).
 *   - `filter`: the black-key feedback frame, used when params.black_key_level_feedback >= 0 and data[0] != NULL;
 *     its rows of `field` are updated like the tool's.
 *   - `out` (data[0] == NULL: no output_frame call): the frame output_frame() hands to its encoder -- YUV422P
 *     (NTSCSIM_OUT422_BOB422) or YUV420P, chroma planes (height + 1) / 2 rows -- written per `out_mode` from
 *     the rows of `out_field` (the tool passes video_field's parity, or with -vi the previous field's, :1792-1796).
 *     Rows inside the planes only: the interlaced 4:2:0 repack's one chroma row past the plane for a height of
 *     2 mod 4 (:1215-1223, lands in the AVFrame's padding in the tool) is not written.
 *   - results are in the caller's memory when ntscsim_wait(ticket) returns, delivered in submit order; frame,
 *     filter and out must not be touched between submit and wait.  With one persistent `frame` and several
 *     fields in flight the frame holds the LAST delivered version of each row -- consume `out` (a ring of
 *     encoder frames) rather than `frame`, as the tool does.
 *   - iterations that render from a source into rows padded by >= 2 bytes, without black-key feedback, run
 *     `depth` at a time (default 32); everything else (no source, linesize[0] < width + 2, feedback: a
 *     frame-to-frame recurrence, an interlaced repack whose other field was not submitted right before it)
 *     runs one at a time, in order -- exact, and as slow as the synchronous call.
 *   - ntscsim_sync() delivers everything in flight first; the device-pointer entry points
 *     (ntscsim_fields422_device() ...) must not be mixed in without ntscsim_wait(ctx, NTSCSIM_TICKET_ALL).
 *     ntscsim_host_unpin(ctx, base) drops the engine's registration of a frame the caller is about to free.
 * Host buffers: the rules of ntscsim_submit() above ("Host buffers"; the floor for pinning in place is 64 KiB per
 * plane here).  Results are written into pinned planes by the delivery kernels (the source is snapshotted by one memcpy
 * into a pinned ring: cheaper for the calling thread than waiting for a DMA out of its planes); planes that are not
 * pinned are filled from the staging ring by the engine's copy threads before ntscsim_wait() returns.  Same bytes
 * either way.
 * Errors: as ntscsim_fields422_device(); a refused call consumes no ticket and no rand() draws.
 */
typedef struct ntscsim_frame422 {    /* AVFrame::data[0..2] / linesize[0..2] of a planar YUV frame in host memory */
    uint8_t *data[3];
    int32_t  linesize[3];
    int32_t  _pad;
} ntscsim_frame422;

typedef struct ntscsim_loop422 {
    uint32_t struct_size;            /* sizeof(ntscsim_loop422)                                          */
    int32_t  width, height;          /* output_width x output_height: the size of frame, filter, out     */
    int32_t  src_height;             /* rows of src (its width is `width`)                               */
    ntscsim_frame422 frame;          /* output_avstream_video_frame                                      */
    ntscsim_frame422 src;            /* output_avstream_video_input_frame, or data[0] == NULL            */
    ntscsim_frame422 filter;         /* output_avstream_video_filter_frame, or data[0] == NULL           */
    ntscsim_frame422 out;            /* output_avstream_video_bob_frame / the encoder frame, or NULL     */
    uint32_t field;                  /* (video_field & 1) ^ 1                                            */
    uint32_t flags;                  /* NTSCSIM_422_*                                                    */
    uint32_t out_mode;               /* NTSCSIM_OUT422_* (below)                                         */
    uint32_t out_field;              /* output_frame()'s `field` argument                                */
    uint64_t fieldno;                /* video_field                                                      */
} ntscsim_loop422;

#define NTSCSIM_SUBMIT422_DIRTY 0x40000u   /* the caller changed frame / filter since the engine last saw them */

int ntscsim_field422(ntscsim_ctx *ctx, const ntscsim_loop422 *it);
int ntscsim_submit422(ntscsim_ctx *ctx, const ntscsim_loop422 *it, uint32_t submit_flags, uint64_t *ticket);
/* Optional: iterations per launch (1..4096, default 32) and iterations that may be in flight (0: 4 * depth;
 * >= 2 * depth + 2).  Waits for everything in flight first. */
int ntscsim_submit422_configure(ntscsim_ctx *ctx, int depth, int slots);
/* [0] submitted [1] launches [2] source uploads [3] batched iterations [4] one-at-a-time iterations
 * [5] frame (re)uploads [6] iterations delivered by kernels into pinned caller planes [7] submits that blocked on a full ring */
void ntscsim_submit422_stats(const ntscsim_ctx *ctx, uint64_t out[8]);


/*
 * The pixel work of output_frame() ffmpeg_to_composite.cpp:1131, lines :1177-1236: line-double
 * ("bob") the rows of `field` of a processed YUV422P frame into the frame handed to the encoder.
 *   NTSCSIM_OUT422_BOB422         use_422_colorspace, field rate (:1177-1196): bob is YUV422P
 *   NTSCSIM_OUT422_BOB420         4:2:0, field rate (:1197-1236): bob is YUV420P; chroma row y/2 is
 *                                 the frame's chroma row sy(y) for even y (decimation by copy)
 *   NTSCSIM_OUT422_INTERLACED420  4:2:0 with -interlaced (:1202, :1215-1223): luma copied 1:1,
 *                                 chroma rows interleaved per field
 * (4:2:2 interlaced output encodes the frame as is, :1158 -- nothing to do.)  The bob frame's
 * chroma planes need (height+1)/2 rows in the 4:2:0 modes -- and ONE MORE in NTSCSIM_OUT422_INTERLACED420 when
 * height is 2 mod 4: the tool's repack writes chroma row (y & 1) + ((y & ~3) >> 1) for y = height - 1 then, one
 * row past the plane (in the tool that lands in the frame's padding); the same row is written here.
 * Stream-ordered like the calls above.
 */
#define NTSCSIM_OUT422_BOB422        0u
#define NTSCSIM_OUT422_BOB420        1u
#define NTSCSIM_OUT422_INTERLACED420 2u
#define NTSCSIM_OUT422_FRAME         3u   /* 4:2:2 with -interlaced: the tool encodes the processed frame itself (:1158);
                                             a 1:1 copy, for callers that keep several fields in flight (ntscsim_submit422) */

typedef struct ntscsim_out422_desc {
    const void *frame_dev[3];       /* processed YUV422P frame (the dst of ntscsim_fields422_device) */
    void       *bob_dev[3];         /* encoder frame: YUV422P or YUV420P                         */
    int32_t     frame_linesize[3], bob_linesize[3];
    uint32_t    field;              /* output_frame()'s `field` argument (:1793, :1796)          */
    uint32_t    mode;               /* NTSCSIM_OUT422_*                                          */
} ntscsim_out422_desc;

int ntscsim_output422_device(ntscsim_ctx *ctx, const ntscsim_out422_desc *descs, int n,
                             int width, int height, void *hip_stream);

/* ---- encoder-side colour conversion (output side) ------------------------
 * What the tool does with sws_scale(BGRA -> codec pix_fmt) at ffmpeg_ntsc.cpp:2266 (pix_fmt chosen
 * at :1998: YUV420P, or YUV422P with -422).  libswscale is a third-party dependency that is not
 * in the reference tree, so this is NOT a bit-clone of it ("parity unpinned"): BT.601 limited
 * range, 15-bit fixed point, Y = (8414 R + 16519 G + 3208 B + (16<<15) + (1<<14)) >> 15; Cb/Cr from
 * the channel sums of each 2x1 (4:2:2) or 2x2 (4:2:0; an odd last row counts twice) block with
 * coefficients (-4864,-9527,14392) / (14392,-12060,-2331), +128, rounded.  Width must be even.
 * Converting on the GPU shrinks the device-to-host payload from 4 to 1.5 / 2 bytes per pixel. */
#define NTSCSIM_PIX_YUV420P 0
#define NTSCSIM_PIX_YUV422P 1
typedef struct ntscsim_yuv_desc {
    const void *bgra_dev;           /* BGRA frame (e.g. a bob frame written by ntscsim_fields_device) */
    void       *yuv_dev[3];         /* Y, U, V planes; chroma (height+1)/2 rows for 4:2:0          */
    int32_t     bgra_linesize;
    int32_t     yuv_linesize[3];
} ntscsim_yuv_desc;
int ntscsim_bgra_to_yuv_device(ntscsim_ctx *ctx, const ntscsim_yuv_desc *descs, int n,
                               int width, int height, int pix_fmt, void *hip_stream);
/* draws of one composite_video_process() call (chroma noise runs at width/2 samples per row) */
uint64_t ntscsim_rng_calls_per_field_422(const ntscsim_params *p, int width, int height,
                                         unsigned field);

/* Block until everything enqueued by this ctx has finished. */
int ntscsim_sync(ntscsim_ctx *ctx);

/* Which kernels a launch of DEVICE-RESIDENT fields takes (ntscsim_fields_device / ntscsim_fields422_device; the host-frame
 * entry points -- ntscsim_field, ntscsim_submit, ntscsim_field422, ntscsim_submit422 -- decide for themselves):
 *   NTSCSIM_FORM_THROUGHPUT (default)  the one-launch chain: one wavefront per 63 rows walks the whole pipeline -- what long
 *                                      batches want (1.3 us per field at 600 fields, 0.42 ms for a launch of ANY length up to 32);
 *   NTSCSIM_FORM_LATENCY               launches of up to 64 fields run the chain as wavefront ROLES of one workgroup per 63 rows
 *                                      (csrc/ntsc_pipe.hip, k422_pipe): 0.17 ms for a launch of up to 32 fields -- a frame at a
 *                                      time between a decoder and an encoder on the same GPU.  Same bytes either way; switch
 *                                      sets the role kernels do not cover, and longer launches, keep the throughput form.
 * NTSCSIM_OK, NTSCSIM_E_ARG. */
enum { NTSCSIM_FORM_THROUGHPUT = 0, NTSCSIM_FORM_LATENCY = 1 };
int ntscsim_set_launch_form(ntscsim_ctx *ctx, int form);

/* Which kernels the groups of a later ntscsim_mixed_fields_device() call on this ctx run (nothing else is affected: the
 * single-set calls, the YUV422P mixed call and the batches pick their kernels as before):
 *   NTSCSIM_MIXED_GENERIC (default)  every group runs the generic mixed kernel of its decoder class (k_mixed_encode,
 *                                    k_mixed_decode<..>): options read at run time;
 *   NTSCSIM_MIXED_TUNED              a named set of the default or -vhs preset families -- noise levels, tape speed,
 *                                    sharpening, head-switch point, S-Video out, PAL, the -comp-catv* presets -- runs the
 *                                    hand-tuned kernel form ntscsim_fields_device() picks for it on a throughput-form ctx
 *                                    (k_mixed_encode_fast*, k_mixed_decode_fast*: csrc/ntsc_mixed_fast.hip), when that form's
 *                                    preconditions hold for the CALL: 16-byte aligned rows in every descriptor, and a
 *                                    composite plane of the whole call small enough for 32-bit offsets
 *                                    (ntscsim_debug_fast_plane_ok).  Every other set -- odd scanline phases, the full output
 *                                    low-pass, nocolor, a subcarrier amplitude other than 50, no luma noise, no input
 *                                    low-pass ... -- keeps the generic kernel, in the same call.  Still one launch per kernel
 *                                    form present, in a fixed order (csrc/mixed_forms.hpp).  Same bytes, same refusals and
 *                                    same rand() position either way.
 * NTSCSIM_OK, NTSCSIM_E_ARG. */
enum { NTSCSIM_MIXED_GENERIC = 0, NTSCSIM_MIXED_TUNED = 1 };
int ntscsim_set_mixed_forms(ntscsim_ctx *ctx, int forms);

/* Kernel timing from hipEvents recorded on the launch stream around each stage of every
 * ntscsim_fields_device() call made while profiling is on.  ntscsim_get_timings_ms() waits for
 * those calls, returns the SUMS since the previous query (index 0 setup kernels, 1 encode
 * kernel, 2 decode kernel, 3 whole call incl. descriptor upload and bob) and the number of calls. */
void ntscsim_set_profiling(ntscsim_ctx *ctx, int on);
int  ntscsim_get_timings_ms(ntscsim_ctx *ctx, float out_ms[4], int *n_calls);

/* Debug tap used by the stage-level parity tests: copy the composite-signal plane (int32, one
 * value per pixel, row-major [n][L][W]) that the last ntscsim_fields_device() call left in
 * scratch -- the signal after chroma_into_luma + pre-emphasis + luma noise (ffmpeg_ntsc.cpp:1611-1644),
 * before head switching -- into host memory. */
int ntscsim_debug_read_composite(ntscsim_ctx *ctx, int32_t *out, size_t out_elems);

/* Test hook: the number of draws k_row_states looks back at first for the noise accumulators
 * (default 24 / 31, taken from the row's rand() window), e.g. 2 / 2 so that most rows go through
 * the backward extension of that look-back.  Results must not change. */
void ntscsim_debug_set_warmup(ntscsim_ctx *ctx, int luma_draws, int chroma_draws);

/* Test hook: always launch the GENERIC kernels (options read at run time) instead of the PRESET
 * specialisations chosen for the default / -vhs parameter sets.  Results must not change. */
void ntscsim_debug_force_generic(ntscsim_ctx *ctx, int on);

/* Test hook: bit 0 keeps the template-specialised PRESET kernels (k_encode / k_decode) where the
 * hand-tuned ones (csrc/ntsc_encode_fast.hip, csrc/ntsc_decode_fast.hip) would run; bit 1 runs
 * the hand-tuned VHS decoder as two launches (VCR half -> second composite plane -> TV half)
 * instead of one; for the YUV422P tool bit 0 selects the twelve-sweep kernel, bit 1 the run-time-switch
 * form of the four-sweep kernel, bit 2 the four-sweep form of the preset kernel (instead of sweep A + one
 * streamed pass).  Results must not change. */
void ntscsim_debug_no_fast_decode(ntscsim_ctx *ctx, int on);

/* Which kernel forms the last ntscsim_fields_device() / ntscsim_fields422_device() / batch run on this
 * ctx enqueued, in launch order, as a ';'-separated list of names as they appear in a rocprofv3 kernel
 * trace without the argument list (e.g. "k_field_setup;k_row_states;k_encode_fast<double>;
 * k_decode_fast<true,double>").  Returns the length of the full list (it is truncated to cap-1
 * characters), or NTSCSIM_E_ARG.  The parity tests assert on it so that a specialised form cannot
 * silently stop being the one that runs.  Behind a scan call (ntscsim_scan_*) the list names k_scan_splat, and
 * whether it is "k_scan_splat+spill" is read from a device counter: the call then selects the ctx's device and
 * SYNCHRONISES it (hipDeviceSynchronize) before it copies the counter back; otherwise it touches no device. */
int ntscsim_debug_last_kernels(const ntscsim_ctx *ctx, char *out, size_t cap);

/* Test hook: bytes of dynamic LDS the last ntscsim_fields_device() / batch run on this ctx asked for with its decoder
 * launch -- the luma delay ring of the composite -vhs forms at tape speed SP (csrc/ntsc_rowend_plan.hpp: luma_ring),
 * 4096, or 0 where the decoder re-reads its luma samples (LP, EP, rows too narrow for the grouped row ends, every other
 * form).  NTSCSIM_E_ARG without a ctx.  Touches no device. */
int ntscsim_debug_last_decoder_lds(const ntscsim_ctx *ctx);

/* Test hook (pure host arithmetic, no ctx): 1 when a batch of n_fields fields of width x height may take
 * the hand-tuned kernels as far as the size of its composite plane is concerned -- they address the
 * plane with 32-bit buffer offsets, and the displaced index of the head switch must not wrap around
 * 2^32 back into the plane.  head_switching: 0 = off, 1 = displacement of at most width/10 samples,
 * 2 = any displacement (the wrap-around form: a margin of a whole 1.1-width window either way).
 * 0 = the generic kernels run. */
int ntscsim_debug_fast_plane_ok(int n_fields, int width, int height, int head_switching);

/* Test hook (pure host arithmetic, no ctx): the kernel forms a NTSCSIM_MIXED_TUNED call gives the groups of `set` when
 * the call holds n_fields_total fields of width x height in all (its composite plane is sized for all of them), every
 * descriptor has 16-byte aligned rows (aligned != 0) or some have not, and the ctx is in `mode` (NTSCSIM_MODE_*: the forms
 * of the three modes differ in the filter-state type only).  *enc_form: 0 generic, 1 k_mixed_encode_fast, 2 its
 * pre-emphasis form.  *dec_form: 0 | 1 | 2 the generic kernel of the set's decoder class (no VCR | VCR with composite out |
 * VCR with S-Video out), 3 k_mixed_decode_fast<false>, 4 k_mixed_decode_fast<true>, 5 its wrap-around form, 6
 * k_mixed_decode_fast_sv, 7 k_mixed_decode_fast_bk<false>, 8 k_mixed_decode_fast_bk<true> (csrc/mixed_forms.hpp).
 * NTSCSIM_OK, NTSCSIM_E_ARG, or what the mixed call returns for such a set (NTSCSIM_E_PARAM). */
int ntscsim_debug_mixed_form_of(const ntscsim_params *set, int width, int height, int n_fields_total, int aligned, int mode,
                                int *enc_form, int *dec_form);

/* Test hook: what the synchronous call ntscsim_field() did since the ctx was created -- [0] calls, [1] calls whose SOURCE
 * frame was read where it is (pinned memory the GPU can address, 16-byte aligned rows: no upload), [2] calls whose
 * DESTINATION frame was written where it is (no download), [3] calls (of either tool's synchronous entry point) that
 * found their setup kernel already run, launched ahead of time by the call before. */
void ntscsim_debug_field_stats(const ntscsim_ctx *ctx, uint64_t out[4]);

/* Test hook: the table caches of ntscsim_mixed_fields_device() -- [0] jump-table sets cached (one per geometry and draw
 * layout), [1] cos/sin tables cached (one per video_chroma_phase_noise level), [2] times both caches were dropped, which
 * waits for the device: only a call that MISSES more entries than a cache has room for (256 each) does that.  A call whose
 * tables are all cached touches neither.  Touches no device. */
void ntscsim_debug_mixed_tables(const ntscsim_ctx *ctx, uint64_t out[3]);

/* ---- the raw-composite decoder: ffmpeg_raw28ntsc.cpp ---------------
 * The tool reads 8-bit composite video sampled at 8 x fsc (28.636 MHz, e.g. a cxadc capture) and
 * renders one grey-scale BGRA frame of (scanline_samples + 1 & ~1) x 262 per field:
 *   hsync_dc_proc() :556-594 on every sample (sync-tip tracking, low-passed sync detector);
 *   composite_layer() :601-849 per field: vertical-sync search, black / white calibration on the
 *   equalising pulses, then per scanline: level equalisation, delay-4 comb luma / chroma split,
 *   rendering, horizontal re-sync;  field loop main() :1006-1038.
 * A decoder object is not re-entrant (one thread at a time); calls are synchronous.
 * One ntscsim_raw28_decode*() call = one run of the tool on one input file: the decoder state
 * starts from the tool's initial state every call (an empty capture gives 0 fields).  Long captures and
 * pipes: ntscsim_raw28_stream_*() below.  Results are bit-identical to the tool's, including
 * where its calibration sums run past the buffered part of the capture into stale or never-filled
 * records of its sample buffer (:655-676); only reads past the END of that array (undefined in the
 * tool) are defined here, as zero records.
 */
typedef struct ntscsim_raw28_opts {
    uint32_t struct_size;            /* sizeof(ntscsim_raw28_opts)                               */
    uint32_t _pad0;
    double   sample_rate;            /* -s: 0 = "ntsc28" = 315e6*8/88; "40mhz" = 40e6; else Hz   */
    int32_t  mark_sync;              /* -marksig :458                                            */
    int32_t  disable_sync;           /* -nosig   :467                                            */
    int32_t  disable_wp_equ;         /* -nowequ  :464                                            */
    int32_t  show_subcarrier;        /* -showsc  :473                                            */
    int32_t  disable_subcarrier;     /* -nosc    :470                                            */
    int32_t  disable_equalization;   /* -noequ   :461                                            */
} ntscsim_raw28_opts;
typedef struct ntscsim_raw28 ntscsim_raw28;

void ntscsim_raw28_opts_init(ntscsim_raw28_opts *o);
/* mirror of parse_argv() :442-520 (-marksig -noequ -nowequ -nosig -nosc -showsc -s <rate>; -width,
 * -i, -o, -422, -420, -inntsc are accepted and have no effect on the decoder: preset_NTSC() :395
 * overrides the width after parsing).  Returns NTSCSIM_OK, NTSCSIM_E_HELP or NTSCSIM_E_FLAG (the tool's
 * "return 1"). */
int  ntscsim_raw28_parse_argv(ntscsim_raw28_opts *o, int argc, const char *const *argv, int start);
int  ntscsim_raw28_geometry(const ntscsim_raw28_opts *o, int *width, int *height, int *scanline_samples);
int  ntscsim_raw28_create(const ntscsim_raw28_opts *o, int device, ntscsim_raw28 **out);
void ntscsim_raw28_destroy(ntscsim_raw28 *dec);
const char *ntscsim_raw28_last_error(const ntscsim_raw28 *dec);
/* Decode a whole capture.  `capture` is host memory (ntscsim_raw28_decode) or device memory
 * (ntscsim_raw28_decode_device), n_samples < 2^32.  frames_dev: device memory for max_fields BGRA
 * frames, frame k at frames_dev + k * frame_stride, rows of `linesize` bytes (>= 4 * width).  Rows
 * the tool does not render are zero, alpha is 0 (:757-775).  Synchronous.  *n_fields = fields the
 * tool would have produced (its loop stops when fewer than 256 scanlines remain), capped at
 * max_fields. */
int  ntscsim_raw28_decode(ntscsim_raw28 *dec, const uint8_t *capture_host, size_t n_samples,
                          void *frames_dev, size_t frame_stride, int linesize, int max_fields, int *n_fields);
int  ntscsim_raw28_decode_device(ntscsim_raw28 *dec, const void *capture_dev, size_t n_samples,
                                 void *frames_dev, size_t frame_stride, int linesize, int max_fields, int *n_fields);
/* The same decoder on a stream of any length, push by push (a capture file read in pieces, a pipe): the
 * tool itself keeps a window of 2048 scanlines (:353) and never needs the whole capture.
 *   ntscsim_raw28_stream_reset()  start a new stream (the state of a fresh run of the tool);
 *   ntscsim_raw28_stream_push()   `n` more samples (host memory, or device memory with on_device != 0;
 *       n = 0 is allowed), `final` != 0 when the stream ends with them.  Decodes, into frames_dev as in
 *       ntscsim_raw28_decode(), every field whose 2048-scanline window is complete -- the tool blocks in
 *       read() until its buffer is full, so a field is produced exactly when the tool could produce it --
 *       up to max_fields of them; fields held back by max_fields come out of the following pushes.  After
 *       the final push: the fields the tool produces before its "fewer than 256 scanlines left" stop.
 *       *n_fields = fields written by this call.  The sequence of all fields is bit-identical to one
 *       ntscsim_raw28_decode() of the concatenated samples, whatever the push sizes.
 * The decoder keeps only what it can still need (about two windows of samples on the device), so the
 * stream may be far longer than 2^32 samples; one push must be shorter than that.  A push that fails after it has
 * taken its samples (NTSCSIM_E_HIP, NTSCSIM_E_NOMEM, NTSCSIM_E_INTERNAL) leaves the stream half advanced: it is
 * then refused (NTSCSIM_E_ARG) until ntscsim_raw28_stream_reset(); argument errors leave the stream as it was.
 * ntscsim_raw28_decode*() are a reset followed by one final push. */
int  ntscsim_raw28_stream_reset(ntscsim_raw28 *dec);
int  ntscsim_raw28_stream_push(ntscsim_raw28 *dec, const void *samples, size_t n, int on_device, int final,
                               void *frames_dev, size_t frame_stride, int linesize, int max_fields, int *n_fields);
/* blank_level, white_level (:553-554) and the stream position (total_count_src) after the last call */
int  ntscsim_raw28_get_levels(const ntscsim_raw28 *dec, double *blank, double *white, uint64_t *read_pos);
/* Test hooks.  warm-up scanlines of the speculative front end (default 112; 0 forces every chunk
 * through the exact repair rounds) and chunk size in samples (default 4096); results must not
 * change.  stats: [0] front-end repair rounds, [1] chunks repaired, [2] comb-tail rounds (after the serial first guess: 1 when it was the fixed point),
 * [3] sync runs, [4] rendered scanlines, [5] calibration pulses of the last call; [6..11] wall-clock
 * microseconds of its phases: front end, run extraction, sync walk (level calibration, comb tails and rendering of
 * the groups of fields it has finished run on the GPU behind it), queuing the same for the last two groups, waiting
 * for the GPU to finish them, redoing the comb tails by rounds + a second rendering (0 unless a group's first guess
 * of the tails did not settle); [12] calibration pulses whose sums ran past the buffered
 * stream, [13] never-filled records among them; [14] compactions of the device buffer (streams),
 * [15] the most samples the device buffer ever held.  Counters accumulate over the pushes of a stream.
 * (A decoder whose front end leaves more than one chunk link in a hundred open after its speculative pass -- a noisy
 * source -- lengthens the warm-up of its later passes by 16 scanlines, up to 64: speed only.)
 * Environment (read by ntscsim_raw28_create, developer / test switches; results never depend on them):
 * NTSCSIM_RAW28_SEG = samples the front end takes per segment (default 2^29: 8 bytes of scratch per sample),
 * NTSCSIM_RAW28_CHUNKS = chunk count of its second sweep on long streams, NTSCSIM_RAW28_EXACT = scanlines at the end of the second sweep's warm-up that are walked sample
 * by sample (default 30; the ones before are taken in closed form where that is known to be safe; >= 112: all),
 * NTSCSIM_RAW28_LANES = chunks per wavefront of that sweep (default 16), NTSCSIM_RAW28_GROUP = fields per group of the
 * back half's pipeline behind the sync walk (default 160), NTSCSIM_RAW28_TAILROUNDS = 1: test hook, take the path of
 * comb tails whose first guess did not settle. */
void ntscsim_raw28_debug_set_speculation(ntscsim_raw28 *dec, int warm_lines, int chunk_samples);
void ntscsim_raw28_debug_stats(const ntscsim_raw28 *dec, int64_t out[16]);
/* Debug tap (host only, no GPU): the chunk length the front end's second sweep picks for a stream of `target_samples` x
 * 16,384 samples -- `subchunks` pieces of whole 64-sample blocks near a whole number of scanlines */
void ntscsim_raw28_debug_pick_chunk(double scanline_samples, double target_samples, int *chunk, int *subchunks);
/* Debug tap: the front end's hsync_dc_raw of every sample of the last call, to host memory */
int  ntscsim_raw28_debug_read_front(ntscsim_raw28 *dec, uint8_t *hsync_dc_raw, size_t n);

/* ---- frameblend: the frame-rate converter in front of the simulator (frameblend.cpp) ---------------
 * The tool resamples a clip to the output rate: every output period `current` (one tick of
 * output_field_rate) is the blend of the source frames that overlap [current, current + 1), weighted by
 * the overlap, optionally in linear light through a gamma table (main() :929-1081).  Mapping:
 *
 *   globals :44-57 + preset_NTSC() :491-494 + parse_argv() :512-634 | ntscsim_blend_params, _init(), _parse_argv()
 *   InputFile::video_frame_rgb_to_output_f() :100-110               | ntscsim_blend_frame_time()
 *   the weight scan, squelch and weight16 :929-1028, erase :1107-1120 | ntscsim_blend_plan_*()   (host, no GPU)
 *   gamma16_do_init() :724-732                                      | ntscsim_blend_tables()    (host libm)
 *   the pixel loops :1032-1081                                      | ntscsim_blend_frames_device() / _clip_device() / _frames_host()
 *
 * Decoding, scaling (-underscan, sws_scale) and encoding stay with the caller; the
 * switches that steer them are parsed and recorded.  Output frames are BGRA with alpha 0xFF (:1051), stay in
 * device memory and can be handed to ntscsim_fields_device() as sources.
 */
typedef struct ntscsim_blend_params {
    uint32_t struct_size;            /* = sizeof(ntscsim_blend_params)                                   */
    int32_t  rate_num, rate_den;     /* output_field_rate :54 / preset_NTSC() :491-494  60000 / 1001     */
    int32_t  output_width;           /* :55  -1 = size of the input (-width, >= 32)                      */
    int32_t  output_height;          /* :56  -1                                                          */
    int32_t  squelch_near_match;     /* squelch_frameblend_near_match :44  false (-sqnr)                 */
    int32_t  fullframealt;           /* :46  false (-ffa)                                                */
    int32_t  framealt;               /* :47  1 (-fa, clamped 1..8 :548-550)                              */
    double   gamma_correction;       /* :49  -1; the gamma path runs only when > 1 (:1032)               */
    /* recorded for the media I/O layer, not acted on here */
    int32_t  underscan;              /* :51  0 (-underscan, clamped 0..99)                               */
    int32_t  use_422_colorspace;     /* :53  false (-422 / -420)                                         */
    int32_t  n_inputs;               /* number of -i switches seen (:561-565)                            */
    int32_t  _pad;
    const char *input_path;          /* the last -i                                                      */
    const char *output_path;         /* -o :595-599                                                      */
} ntscsim_blend_params;

void ntscsim_blend_params_init(ntscsim_blend_params *p);
/* Mirror of parse_argv() :512-634: same switch names (any number of leading '-'), clamps and the -or forms
 * (:566-594: strtof, optional :d /d \d, "< 5 fps" floor, a bare number is stored x10000 over 10000).
 * argv[0] is the program name.  require_io != 0 applies the "No output file / No input files" checks
 * (:624-631).  Returns NTSCSIM_OK, NTSCSIM_E_HELP (-h / -help) or NTSCSIM_E_FLAG (the tool's "return 1"). */
int  ntscsim_blend_parse_argv(ntscsim_blend_params *p, int argc, const char *const *argv, int require_io);
/* :100-110: pts as a double, times tb_num * rate_num, then divided by tb_den * rate_den (both products in
 * signed 64-bit integers; two roundings, in that order). */
double ntscsim_blend_frame_time(int64_t pts, int32_t tb_num, int32_t tb_den, const ntscsim_blend_params *p);

/* The planner: which source frames make output period `current`, with which 16.16 weights (:929-1028).
 * It is stateful like the tool's two vectors: ntscsim_blend_plan_push() appends a frame (its time from
 * ntscsim_blend_frame_time()) and returns its STABLE id, counted from 0 at the start of the clip;
 * ntscsim_blend_plan_next() must be called once per output period, in order (the tool's `current++`).  It
 * reproduces the erase of the first `cutoff` frames once cutoff reaches 32 (:1107-1120) -- which renumbers
 * the tool's indices and shifts the phase of the -fa scan (:937) -- internally: ids stay stable, and
 * *release_below (may be NULL) is the lowest id a later call can still name, so the caller may free or
 * reuse every source frame below it.  *n receives the tap count (0: the tool writes a black frame); with
 * more than `cap` taps the call returns NTSCSIM_E_SIZE, *n is the count needed and the state is unchanged.
 * Taps whose weight rounded to 0 are listed (they add nothing).  Plain double / integer arithmetic, no GPU. */
typedef struct ntscsim_blend_plan ntscsim_blend_plan;
int     ntscsim_blend_plan_create(const ntscsim_blend_params *p, ntscsim_blend_plan **out);
int64_t ntscsim_blend_plan_push(ntscsim_blend_plan *plan, double frame_t);
int     ntscsim_blend_plan_next(ntscsim_blend_plan *plan, int64_t current, int64_t *ids, uint32_t *weight16,
                                int cap, int *n, int64_t *release_below);
void    ntscsim_blend_plan_reset(ntscsim_blend_plan *plan);
void    ntscsim_blend_plan_destroy(ntscsim_blend_plan *plan);
/* Number of output periods the tool renders for a clip whose LAST frame has time `last_frame_t`: its loop
 * stops at the first current > ceil(last_frame_t) once the input is exhausted (:924-927). */
int64_t ntscsim_blend_clip_periods(double last_frame_t);

/* gamma16_do_init() :724-732 for gamma_correction = gamma: dec[i] = (unsigned long)(pow(i / 255.0, gamma) * 8192),
 * enc[i] = (unsigned long)(pow(i / 8192.0, 1.0 / gamma) * 255), host libm.  NTSCSIM_E_PARAM unless gamma > 0. */
int  ntscsim_blend_tables(double gamma, uint16_t dec[256], uint8_t enc[8193]);

/* Snapshot the blend parameters on a ctx (any ntscsim_params it was created with) and upload the gamma
 * tables when gamma_correction > 1.  Waits for blend work in flight on the ctx. */
int  ntscsim_blend_bind(ntscsim_ctx *ctx, const ntscsim_blend_params *p);

typedef struct ntscsim_blend_tap {
    const void *src_dev;             /* device pointer, BGRA frame of the descriptor's width x height    */
    int32_t     src_linesize;        /* bytes, >= 4*width, multiple of 4                                 */
    uint32_t    weight16;            /* :1027-1028                                                       */
} ntscsim_blend_tap;
typedef struct ntscsim_blend_desc {
    void       *dst_dev;             /* device pointer, BGRA frame; bytes of a row behind 4*width are not touched */
    int32_t     dst_linesize;        /* bytes, >= 4*width, multiple of 4                                 */
    int32_t     width, height;
    int32_t     n_taps;              /* 0: black frame, alpha 0xFF                                        */
    const ntscsim_blend_tap *taps;   /* host memory, n_taps entries                                      */
} ntscsim_blend_desc;
#define NTSCSIM_BLEND_FAST_TAPS 4
/*
 * The pixel loops :1032-1081 for `n` output frames, one launch: per channel
 *   gamma_correction > 1:  out = enc[min(8192, (sum_k dec[src_k] * weight16_k) >> 16)]
 *   otherwise:             out = min(255, (sum_k src_k * weight16_k) >> 16)
 * alpha 0xFF.  All frame pointers are DEVICE pointers; `descs` and the tap lists are host memory and are
 * consumed by the call.  Enqueued on hip_stream (NULL: the ctx's own stream), returns without synchronising.
 * A call whose descriptors all have at most NTSCSIM_BLEND_FAST_TAPS taps runs k_blend_fast (taps in the
 * record), any other k_blend_general (tap lists in device memory); the sums are 32-bit while
 * 8192 * sum(weight16) < 2^32 (255 * sum without gamma) holds for every descriptor and 64-bit otherwise.  Frames whose
 * pointers and linesizes are all multiples of 16 move as 16-byte vectors; any other frame, and the last
 * width % 4 pixels of a row, as dwords.  Same bytes either way.  sum(weight16) >= 2^38 is refused
 * (NTSCSIM_E_ARG; the tool's own clamp255(int) is undefined from 2^39); a destination must not be a source
 * of the same call.  Requires ntscsim_blend_bind().
 */
int  ntscsim_blend_frames_device(ntscsim_ctx *ctx, const ntscsim_blend_desc *descs, int n, void *hip_stream);
/*
 * A clip resident in device memory: n_src BGRA frames (src_dev[j], rows of src_linesize bytes, time
 * frame_t[j]) -> output periods [first, last), period k into dst_dev[k - first].  Runs the planner on the
 * host from period 0 with the tool's read-ahead (:910: frames are appended while the newest is less than 30
 * periods ahead) and enqueues the launches on hip_stream; asynchronous like ntscsim_blend_frames_device().
 */
int  ntscsim_blend_clip_device(ntscsim_ctx *ctx, const void *const *src_dev, int src_linesize,
                               const double *frame_t, int n_src, void *const *dst_dev, int dst_linesize,
                               int width, int height, int64_t first, int64_t last, void *hip_stream);
/* ntscsim_blend_frames_device() on HOST frames: every pointer of descs / taps is host memory.  Each distinct
 * source frame (pointer + linesize) is uploaded once however many outputs it feeds; uploads, the launch and
 * the downloads go through pinned staging of the ctx.  Synchronous.  Same bytes as the device call. */
int  ntscsim_blend_frames_host(ntscsim_ctx *ctx, const ntscsim_blend_desc *descs, int n);

/* ---- colorkey: the retro colour keyer behind the simulator (ffmpeg_colorkey.cpp) --------------------
 * The tool keys its inputs, in order, over a destination frame that is never cleared: a source pixel is
 * copied when its RGB distance to the key colour passes the threshold, the distance is sampled every
 * -xd pixels, -noise lets keyed-out pixels through at random (three rand() per pixel from the unseeded
 * stream) and -f fades what is already there.  The destinations form a ring of -d frames, so output
 * frame t is keyed onto output frame t - d ("hall of mirrors").  Mapping:
 *
 *   InputFile :68, :517-527 + new_input_file() :571-589               | ntscsim_key_layer, ntscsim_key_params_add_layer()
 *   globals :44-63 + preset_NTSC / _PAL :597-613 + parse_argv() :629-739 | ntscsim_key_params, _init(), _parse_argv()
 *   the rand() calls of composite_layer() :837-842, :860-861           | ntscsim_key_rand_advance()  (host, no GPU)
 *   composite_layer() :844-885, all layers of a frame :1119-1146       | ntscsim_key_frames_device() / _frames_host()
 *   the frame loop over the ring :997-1019, :1118-1171                 | ntscsim_key_clip_device()
 *
 * Decoding, scaling (sws_scale), encoding and the audio pass-through stay with the caller.
 * Frames are BGRA in device memory; the simulator's outputs can be handed over as layers without a copy.
 */
typedef struct ntscsim_key_layer {
    uint32_t color;                  /* :517  0 (black)      -color, 0xRRGGBB; the high byte is ignored (:854-856) */
    int32_t  threshhold;             /* :518  0              -threshhold (the tool's spelling), compared signed     */
    uint32_t fade;                   /* :519  0              -f; the factor 256 - fade is unsigned: > 256 wraps     */
    uint32_t xdivr;                  /* :520  1              -xd; 0 behaves as 1 (:883)                              */
    int32_t  invert;                 /* :521  false          -inv                                                    */
    uint32_t noisekey;               /* :527  0              -noise; > 0 draws 3 rand() per pixel                    */
    const char *path;                /* :516  the -i that opened the layer (points into argv), may be NULL            */
} ntscsim_key_layer;

typedef struct ntscsim_key_params {
    uint32_t struct_size;            /* = sizeof(ntscsim_key_params)                                      */
    int32_t  width, height;          /* :46-47  720 x 480 (preset_NTSC), 720 x 576 (-tvstd pal), -width   */
    int32_t  tv_standard;            /* 0 NTSC, 1 PAL (-tvstd)                                             */
    int32_t  delay;                  /* :62  1 (-d, 1..256): frames in the destination ring                */
    int32_t  use_422_colorspace;     /* :44  false (-422 / -420); recorded, not acted on                   */
    int32_t  n_layers;               /* inputs so far, in layering order; no upper limit                   */
    int32_t  layers_cap;             /* allocated entries of `layers`                                      */
    ntscsim_key_layer *layers;       /* heap block owned by the struct: ntscsim_key_params_free()          */
    const char *output_path;         /* -o :693-697                                                        */
} ntscsim_key_params;

void ntscsim_key_params_init(ntscsim_key_params *p);
/* Releases the layer list (the struct itself is the caller's). */
void ntscsim_key_params_free(ntscsim_key_params *p);
/* new_input_file() :571-589: appends a layer that copies the settings of the previous one (defaults :68 for the
 * first).  Returns its index, or NTSCSIM_E_ARG / NTSCSIM_E_NOMEM. */
int  ntscsim_key_params_add_layer(ntscsim_key_params *p, const char *path);
/* Mirror of parse_argv() :629-739: same switch names (any number of leading '-'), every value through strtoul
 * with base 0 and the tool's casts.  argv[0] is the program name.  A per-layer switch (-f -xd -noise -inv
 * -threshhold -color) before the first -i makes the tool throw (current_input_file() :562-569): NTSCSIM_E_ARG.
 * require_io != 0 applies the "No output file / No input files" checks (:729-736).  Otherwise NTSCSIM_OK,
 * NTSCSIM_E_HELP (-h / -help) or NTSCSIM_E_FLAG (the tool's "return 1"; -d outside 1..256, -width < 32). */
int  ntscsim_key_parse_argv(ntscsim_key_params *p, int argc, const char *const *argv, int require_io);
/*
 * The tool's rand() stream is one serial stream; position n is the state after n calls (ntscsim_rng_draw).
 * One output frame visits the layers in list order; a layer that is present and has noisekey > 0 consumes
 * exactly 3 * width * height draws, in raster order, at every pixel whatever its xdivr; an absent layer (no
 * source frame, the early return :837-842) or a layer with noisekey == 0 consumes none.  This advances *pos
 * over one frame: present[l] != 0 marks layer l as present, present == NULL means all of them.  Call it once
 * per frame to chain the positions handed to ntscsim_key_frames_device().
 */
int  ntscsim_key_rand_advance(const ntscsim_key_params *p, const uint8_t *present, uint64_t *pos);

/* Snapshot the key parameters and the layer list on a ctx (any ntscsim_params it was created with).  Waits for
 * key work in flight on the ctx.  NTSCSIM_E_PARAM for delay outside 1..256, NTSCSIM_E_SIZE for a frame size
 * below 1 x 1, above 65536 in either direction or of 2^31 pixels and more. */
int  ntscsim_key_bind(ntscsim_ctx *ctx, const ntscsim_key_params *p);

typedef struct ntscsim_key_src {
    const void *src_dev;             /* device pointer, BGRA frame; NULL: the layer is absent in this frame */
    int32_t     src_linesize;        /* bytes, >= 4*width, multiple of 4                                    */
    int32_t     _pad;
} ntscsim_key_src;
typedef struct ntscsim_key_desc {
    void       *dst_dev;             /* device pointer, BGRA frame, read and written in place; bytes of a row behind 4*width are not touched */
    int32_t     dst_linesize;        /* bytes, >= 4*width, multiple of 4                                    */
    int32_t     width, height;       /* must be the bound params'                                           */
    int32_t     n_layers;            /* must be the bound params'                                           */
    const ntscsim_key_src *layers;   /* host memory, n_layers entries, list order                           */
    uint64_t    rand_pos;            /* position of the frame's first draw                                  */
} ntscsim_key_desc;
#define NTSCSIM_KEY_FAST_LAYERS 4
/*
 * composite_layer() :844-885 for every layer of `n` output frames.  Per pixel and layer, in uint32_t / int
 * arithmetic as the tool has it: the distance d = |dR| + |dG| + |dB| to the key colour is taken from the source
 * pixel where the counter xdivc is 0 (the start of a row and every xdivr pixels) and held between; a noise hit
 * ((r1 * r2 * r3) % 20001 < noisekey on three consecutive draws) sets d = 0xFFFF, which is held likewise; the
 * destination is faded when fade != 0; then all four bytes of the source pixel are copied when d >= threshhold
 * (d < threshhold with invert).  All frame pointers are DEVICE pointers; `descs` and the layer lists are host
 * memory and are consumed by the call.  Enqueued on hip_stream (NULL: the ctx's own stream), returns without
 * synchronising.  Descriptors take effect in order: a later one that names a destination (or reads a frame) an
 * earlier one wrote sees the earlier result.
 * Kernels: k_key_fast<NOISE> (up to NTSCSIM_KEY_FAST_LAYERS layers, in the record) or k_key_general<NOISE> (layer
 * list in device memory); NOISE only when a present layer has noisekey > 0, and then k_key_draw runs in front and
 * leaves one hit bit per pixel.  Frames whose pointers and linesizes are all multiples of 16 move as 16-byte
 * vectors; any other frame, and the last width % 4 pixels of a row, as dwords.  Same bytes either way.
 * NTSCSIM_E_SIZE: a size other than the bound params', a linesize below 4*width or not a multiple of 4.
 * NTSCSIM_E_ARG: a source that overlaps the destination of its descriptor, a NULL destination, no
 * ntscsim_key_bind() before.
 */
int  ntscsim_key_frames_device(ntscsim_ctx *ctx, const ntscsim_key_desc *descs, int n, void *hip_stream);
/*
 * The tool's frame loop :1118-1171 for T output frames of a clip resident in device memory.  ring_dev[0..delay)
 * are the destination frames (the tool zeroes them once, :1013-1016; the caller does that before the first
 * call), *ring_index the slot of the first frame (the tool starts at 0).  Frame t takes layer l from
 * src_dev[l * T + t] (NULL: absent), rows of src_linesize[l] bytes, is keyed onto ring slot
 * (*ring_index + t) % delay and delivered to out_dev[t].  *rand_pos is the position of the first draw.  After
 * the call the ring holds what the tool's ring holds, and *ring_index and *rand_pos are those of frame T: a
 * following call continues the clip.  One launch of k_key_clip_fast<NOISE, layers> (1 to 4 layers) / k_key_clip_general<NOISE> walks the
 * min(delay, T) independent chains through all of their frames with the destination pixel in registers: it is
 * read from the ring once, written to out_dev[t] at every step and to the ring at the end; the fast form keeps the source
 * loads of a chain's next two frames in flight.  Asynchronous like
 * ntscsim_key_frames_device(); ring, sources and outputs must not overlap each other (NTSCSIM_E_ARG).
 */
int  ntscsim_key_clip_device(ntscsim_ctx *ctx, void *const *ring_dev, int ring_linesize, int32_t *ring_index,
                             const void *const *src_dev, const int32_t *src_linesize, void *const *out_dev,
                             int out_linesize, int T, uint64_t *rand_pos, void *hip_stream);
/* ntscsim_key_frames_device() on HOST frames: every pointer of descs / layers is host memory.  Each distinct
 * frame (pointer + linesize) is uploaded once, destinations are downloaded after the last descriptor; all of it
 * goes through pinned staging of the ctx.  Synchronous.  Same bytes as the device call.  A destination must be disjoint
 * from every other frame of the call that is not the very same (pointer, linesize): NTSCSIM_E_ARG otherwise. */
int  ntscsim_key_frames_host(ntscsim_ctx *ctx, const ntscsim_key_desc *descs, int n);
/* Debug tap: the bound on the hit bits of one launch, in bytes (default 128 MiB; 0 restores it).  A clip or frames call
 * whose noisy layers need more is cut into several launches of at least one frame each -- same bytes; the tests set a
 * small bound to reach that path with small frames.  Requires ntscsim_key_bind(); kept across later binds. */
int  ntscsim_key_debug_set_bits_limit(ntscsim_ctx *ctx, size_t bytes);
/* Debug tap (host only, no GPU): the 31-word rand() window from which lane `lane` of k_key_draw starts for a
 * layer whose first draw is at job_pos, computed as the launcher computes it (per-lane polynomial applied to
 * the layer's window).  It must equal the window at job_pos + 768 * lane. */
int  ntscsim_key_debug_lane_state(int width, int height, uint64_t job_pos, uint32_t lane, uint32_t out[31]);

/* ---- average_delay: the frame-averaging delay line behind the simulator (ffmpeg_average_delay.cpp) ----
 * The tool averages its inputs, in order, into a destination frame that is never cleared: every channel of
 * a pixel becomes (source * newlevel + destination * (256 - newlevel) + dither) >> 8, with a 2 x 2 ordered
 * dither that moves with the frame number.  The destinations form a ring of -d frames, so output frame t
 * is an average of the new frame and output frame t - d (camera-tube lag, feedback trails).  Mapping:
 *
 *   InputFile :71-96 + new_input_file() :571-589                       | ntscsim_avg_layer, ntscsim_avg_params_add_layer()
 *   globals :44-68 + preset_NTSC / _PAL :597-613 + parse_argv() :623-708 | ntscsim_avg_params, _init(), _parse_argv()
 *   composite_layer() :801-837, all layers of a frame                   | ntscsim_avg_frames_device() / _frames_host()
 *   the frame loop over the ring :948-970, :1069-1122                   | ntscsim_avg_clip_device()
 *
 * Decoding, scaling (sws_scale), encoding and the audio pass-through stay with the caller.
 * Frames are BGRA in device memory; the simulator's outputs can be handed over as layers without a copy.
 */
typedef struct ntscsim_avg_layer {
    int32_t  newlevel;               /* :73  128             -n ("256=100% 0=0%"); an int, any value: see below   */
    const char *path;                /* the -i that opened the layer (points into argv), may be NULL                */
} ntscsim_avg_layer;

typedef struct ntscsim_avg_params {
    uint32_t struct_size;            /* = sizeof(ntscsim_avg_params)                                      */
    int32_t  width, height;          /* 720 x 480 (preset_NTSC), 720 x 576 (-tvstd pal), -width           */
    int32_t  tv_standard;            /* 0 NTSC, 1 PAL (-tvstd)                                             */
    int32_t  delay;                  /* :67  1 (-d, 1..256): frames in the destination ring                */
    int32_t  use_422_colorspace;     /* false (-422 / -420); recorded, not acted on                        */
    int32_t  n_layers;               /* inputs so far, in layering order; no upper limit                   */
    int32_t  layers_cap;             /* allocated entries of `layers`                                      */
    ntscsim_avg_layer *layers;       /* heap block owned by the struct: ntscsim_avg_params_free()          */
    const char *output_path;         /* -o :662-666                                                        */
} ntscsim_avg_params;

void ntscsim_avg_params_init(ntscsim_avg_params *p);
/* Releases the layer list (the struct itself is the caller's). */
void ntscsim_avg_params_free(ntscsim_avg_params *p);
/* new_input_file() :571-589: appends a layer that copies the newlevel of the previous one (128, :73, for the
 * first).  Returns its index, or NTSCSIM_E_ARG / NTSCSIM_E_NOMEM. */
int  ntscsim_avg_params_add_layer(ntscsim_avg_params *p, const char *path);
/* Mirror of parse_argv() :623-708: -i -o -d -n -width -422 -420 -tvstd pal|ntsc, -h / -help (any number of
 * leading '-'), every value through strtoul with base 0 and the tool's casts: -n becomes an int (so "-1" is -1
 * and "0x100" is 256).  argv[0] is the program name.  -n before the first -i makes the tool throw
 * (current_input_file() :562-569): NTSCSIM_E_ARG.  require_io != 0 applies the "No output file / No input
 * files" checks (:698-705).  Otherwise NTSCSIM_OK, NTSCSIM_E_HELP (-h / -help) or NTSCSIM_E_FLAG (the tool's
 * "return 1"; -d outside 1..256, -width < 32). */
int  ntscsim_avg_parse_argv(ntscsim_avg_params *p, int argc, const char *const *argv, int require_io);

/* Snapshot the parameters and the layer list on a ctx (any ntscsim_params it was created with).  Waits for
 * average work in flight on the ctx.  NTSCSIM_E_PARAM for delay outside 1..256, NTSCSIM_E_SIZE for a frame size
 * below 1 x 1, above 65536 in either direction or of 2^31 pixels and more. */
int  ntscsim_avg_bind(ntscsim_ctx *ctx, const ntscsim_avg_params *p);

typedef struct ntscsim_avg_src {
    const void *src_dev;             /* device pointer, BGRA frame; NULL: the layer is absent in this frame (:808) */
    int32_t     src_linesize;        /* bytes, >= 4*width, multiple of 4                                    */
    int32_t     _pad;
} ntscsim_avg_src;
typedef struct ntscsim_avg_desc {
    void       *dst_dev;             /* device pointer, BGRA frame, read and written in place; bytes of a row behind 4*width are not touched */
    int32_t     dst_linesize;        /* bytes, >= 4*width, multiple of 4                                    */
    int32_t     width, height;       /* must be the bound params' (the tool skips a layer of another size, :812-813) */
    int32_t     n_layers;            /* must be the bound params'                                           */
    const ntscsim_avg_src *layers;   /* host memory, n_layers entries, list order                           */
    uint64_t    field;               /* the `field` argument of composite_layer(): the tool's frame counter `current` */
} ntscsim_avg_desc;
#define NTSCSIM_AVG_FAST_LAYERS 4
/*
 * composite_layer() :801-837 for every layer of `n` output frames.  Per pixel (x, y) and present layer, in
 * unsigned 32-bit arithmetic as the tool has it, with n = (uint32_t)newlevel, s / d the source / destination
 * pixel and dither = ((((x ^ y) + field / delay) & 3) * 255) / 3:
 *     c' = (s_c * n + d_c * (256 - n) + dither) >> 8   for c = R, G, B;     d = (R' << 16) + (G' << 8) + B'
 * For newlevel in 0..256 every channel stays below 256 and the top byte becomes 0; for any other value the
 * factors wrap modulo 2^32, the channels carry into each other and into the top byte, and those are the bytes
 * returned.  An absent layer leaves the destination untouched, top byte included.  All layers of a frame share
 * its dither.  All frame pointers are DEVICE pointers; `descs` and the layer lists are host memory and are
 * consumed by the call.  Enqueued on hip_stream (NULL: the ctx's own stream), returns without synchronising.
 * Descriptors take effect in order: a later one that names a destination (or reads a frame) an earlier one
 * wrote sees the earlier result.  Sources are never written.
 * Kernels: k_avg_fast (up to NTSCSIM_AVG_FAST_LAYERS layers, in the record) or k_avg_general (layer list in
 * device memory).  Frames whose pointers and linesizes are all multiples of 16 move as 16-byte vectors; any
 * other frame, and the last width % 4 pixels of a row, as dwords.  Same bytes either way.
 * NTSCSIM_E_SIZE: a size or layer count other than the bound params', a linesize below 4*width or not a
 * multiple of 4.  NTSCSIM_E_ARG: a source that overlaps the destination of its descriptor, a NULL destination,
 * no ntscsim_avg_bind() before.
 */
int  ntscsim_avg_frames_device(ntscsim_ctx *ctx, const ntscsim_avg_desc *descs, int n, void *hip_stream);
/*
 * The tool's frame loop :1069-1122 for T output frames of a clip resident in device memory.  ring_dev[0..delay)
 * are the destination frames (the tool zeroes them once, :948-970; the caller does that before the first
 * call), *ring_index the slot of the first frame (the tool starts at 0), *field its frame number (the tool
 * starts at 0).  Frame t takes layer l from src_dev[l * T + t] (NULL: absent), rows of src_linesize[l] bytes,
 * is averaged onto ring slot (*ring_index + t) % delay with field *field + t and delivered to out_dev[t].
 * After the call the ring holds what the tool's ring holds, and *ring_index and *field are those of frame T: a
 * following call continues the clip.  One launch of k_avg_clip_fast<layers> (1 to 4 layers) /
 * k_avg_clip_general walks the min(delay, T) independent chains through all of their frames with the
 * destination pixel in registers: it is read from the ring once, written to out_dev[t] at every step and to
 * the ring at the end; the fast form keeps the source loads of a chain's next frames in flight.  Asynchronous
 * like ntscsim_avg_frames_device(); ring, sources and outputs must not overlap each other (NTSCSIM_E_ARG).
 */
int  ntscsim_avg_clip_device(ntscsim_ctx *ctx, void *const *ring_dev, int ring_linesize, int32_t *ring_index,
                             const void *const *src_dev, const int32_t *src_linesize, void *const *out_dev,
                             int out_linesize, int T, uint64_t *field, void *hip_stream);
/* ntscsim_avg_frames_device() on HOST frames: every pointer of descs / layers is host memory.  Each distinct
 * frame (pointer + linesize) is uploaded once, destinations are downloaded after the last descriptor; all of it
 * goes through pinned staging of the ctx.  Synchronous.  Same bytes as the device call.  A destination must be disjoint
 * from every other frame of the call that is not the very same (pointer, linesize): NTSCSIM_E_ARG otherwise. */
int  ntscsim_avg_frames_host(ntscsim_ctx *ctx, const ntscsim_avg_desc *descs, int n);

/* ---- scanimate: the CRT raster re-scan effect (ffmpeg_scanimate.cpp) ----
 * A camera re-scans a picture drawn on a CRT.  Every source sample (two per source pixel) becomes a phosphor
 * dot whose position, size and brightness come from a per-field raster warp -- trapezoid, vertical rotate,
 * vertical stretch, sine "diffuse", 180 fields each -- and the dot is splatted as a cone into a 32-bit
 * accumulator plane, which is then halved, clamped and written out as grey BGRA.  Mapping:
 *
 *   globals + preset_* :601-635 + parse_argv() :643-723, source size :190-197 | ntscsim_scan_params, _init(), _parse_argv()
 *   effect / ef_field :865-867, (current & 1) ^ 1 :1224                       | ntscsim_scan_effect(), ntscsim_scan_field_of()
 *   phosphor_dot() :817-854, scanimate_modify_raster() :859-891,
 *   composite_layer() :894-974                                               | ntscsim_scan_frames_device() / _frames_host()
 *   the field loop :1195-1244, one input                                     | ntscsim_scan_clip_device()
 *
 * With several -i the tool runs composite_layer() once per input onto the same frame, and every call overwrites
 * all of rows field .. height-1: the output is the LAST input's.  The stage therefore takes one source per
 * output, and ntscsim_scan_params keeps the last -i.  Decoding, scaling (sws_scale) to the source size,
 * encoding and the audio pass-through stay with the caller.  Frames are BGRA in device
 * memory; only the green byte of a source pixel is read.
 */
typedef struct ntscsim_scan_params {
    uint32_t struct_size;            /* = sizeof(ntscsim_scan_params)                                      */
    int32_t  output_width, output_height;   /* 720 x 480 (preset_NTSC), the -tvstd presets, -width          */
    int32_t  tv_standard;            /* 0 NTSC, 1 PAL, 2 720p60, 3 1080p60 (-tvstd)                        */
    int32_t  field_rate_num, field_rate_den;    /* 60000 / 1001, PAL 50 / 1                                */
    int32_t  input_ntsc;             /* -inntsc: the source is an interlaced 480-line picture, one field per output */
    int32_t  output_pal;             /* set by preset_PAL only                                             */
    int32_t  use_422_colorspace;     /* false (-422 / -420); recorded, not acted on                        */
    int32_t  n_inputs;               /* number of -i                                                       */
    int32_t  src_width, src_height;  /* derived :190-197 after all of argv: 600 x 800; -inntsc 480 x 480, 480 x 576 when output_pal */
    int32_t  _pad;
    const char *last_input_path;     /* the last -i (points into argv), NULL if none                       */
    const char *output_path;         /* -o                                                                 */
} ntscsim_scan_params;

void ntscsim_scan_params_init(ntscsim_scan_params *p);
/* Mirror of parse_argv() :643-723: -i -o -width -422 -420 -inntsc -tvstd pal|ntsc|720p60|1080p60, -h / -help (any
 * number of leading '-'); -width goes through strtoul with base 0 and the tool's cast to int, and changes the width
 * only.  argv[0] is the program name.  NTSCSIM_E_FLAG (the tool's "return 1") for -width < 32, an unknown standard,
 * an unknown switch, a bare word and a missing value -- the tool hands the NULL behind a trailing -tvstd to
 * strcmp(); here that is the flag error too.  require_io != 0 applies the "No output file / No input files"
 * checks (:713-720).  src_width / src_height are derived when the whole of argv has been read, as the tool derives
 * them when it opens its inputs: the order of -inntsc and -tvstd does not matter.  NTSCSIM_E_HELP for -h / -help. */
int  ntscsim_scan_parse_argv(ntscsim_scan_params *p, int argc, const char *const *argv, int require_io);
/* :865-867: *effect = (fieldno / 180) % 4 (0 trapezoid, 1 rotate, 2 stretch, 3 sine) and *ef_field = fieldno % 180,
 * in the tool's types: the quotient is cut to an unsigned int before it is used, so from fieldno = 180 * 2^32 on both
 * differ from that and ef_field can exceed 179.  Either pointer may be NULL. */
void ntscsim_scan_effect(uint64_t fieldno, uint32_t *effect, uint32_t *ef_field);
/* :1224: the `field` the tool hands to composite_layer() for field number fieldno, (fieldno & 1) ^ 1. */
uint32_t ntscsim_scan_field_of(uint64_t fieldno);

/* Snapshot the parameters on a ctx (any ntscsim_params it was created with).  Waits for scan work in flight on the
 * ctx.  NTSCSIM_E_SIZE for an output or source size below 1 x 1 or above 65536 in either direction, and when
 * 2 * src_width * src_height or output_width * output_height reaches 2^31 (the tool's unsigned int products must
 * not wrap). */
int  ntscsim_scan_bind(ntscsim_ctx *ctx, const ntscsim_scan_params *p);

typedef struct ntscsim_scan_desc {
    void       *dst_dev;             /* device pointer, BGRA frame of the bound output size                 */
    int32_t     dst_linesize;        /* bytes, >= 4*width, multiple of 4                                    */
    int32_t     src_linesize;        /* bytes, >= 4*src_width, multiple of 4                                */
    const void *src_dev;             /* device pointer, BGRA frame; never written                           */
    int32_t     src_width, src_height;   /* any size within the bind limits: the params' are the tool's defaults, not a limit */
    uint64_t    fieldno;             /* the tool's field counter `current`: field = (fieldno & 1) ^ 1       */
} ntscsim_scan_desc;
/*
 * composite_layer() :894-974 for `n` output fields.  Writes bytes 0 .. 4*width of rows field .. height-1 of the
 * destination and nothing else: row 0 when field == 1, the row padding and the bytes around the frame are not
 * touched (the tool's memset :1196 is the caller's).  All frame pointers are DEVICE pointers; `descs` is host
 * memory and is consumed by the call.  Enqueued on hip_stream (NULL: the ctx's own stream), returns without
 * synchronising.  Descriptors take effect in order.  Bit-identical to the tool: the accumulator is an integer sum,
 * every fp64 expression keeps the tool's order (no contraction), and the tool's sin / cos are computed by the
 * host's libm -- per field, and for the sine effect once per source size as two tables over the source samples.
 * Kernels: k_scan_splat (a workgroup sums the dots of a tile of source samples in an on-chip window and flushes
 * the window to the ctx's accumulator plane; a dot whose box leaves the window is added to the plane directly --
 * ntscsim_debug_last_kernels() then says k_scan_splat+spill) and k_scan_resolve.  The ctx owns up to 8 accumulator
 * planes: up to 8 descriptors of a call are in flight together.
 * The descriptor carries no destination size: dst_dev is ASSUMED to hold the bound output_width x output_height
 * with rows of dst_linesize bytes, unchecked -- the call cannot refuse a destination of another size (the Python
 * veneer, which sees the tensor's shape, does, with NTSCSIM_E_SIZE).
 * NTSCSIM_E_ARG: a NULL pointer, a source that overlaps the destination, no ntscsim_scan_bind() before.
 * NTSCSIM_E_SIZE: a linesize below 4*width or not a multiple of 4, a pointer that is not a multiple of 4, a source
 * size outside the bind limits.
 */
int  ntscsim_scan_frames_device(ntscsim_ctx *ctx, const ntscsim_scan_desc *descs, int n, void *hip_stream);
/*
 * The tool's field loop :1195-1244 with one input, for T fields of a clip resident in device memory: output t is
 * the field of *fieldno + t from src_dev[t] (src_w x src_h, rows of src_linesize bytes) in out_dev[t].  Row 0 of a
 * field == 1 output is written as zeros, as the tool's memset leaves it; the row padding is not touched.
 * *fieldno advances by T.  Asynchronous like ntscsim_scan_frames_device(); outputs must not overlap each other
 * or a source (NTSCSIM_E_ARG).
 */
int  ntscsim_scan_clip_device(ntscsim_ctx *ctx, const void *const *src_dev, int src_linesize, int src_w, int src_h,
                              void *const *out_dev, int out_linesize, int T, uint64_t *fieldno, void *hip_stream);
/* ntscsim_scan_frames_device() on HOST frames, through pinned staging of the ctx.  Synchronous.  Same bytes as the
 * device call: the rows and bytes the device call leaves alone keep what the host frame held. */
int  ntscsim_scan_frames_host(ntscsim_ctx *ctx, const ntscsim_scan_desc *descs, int n);
/* Debug taps.  keep_raster(on): k_scan_resolve clears the accumulator as it reads it, so while `on` the plane of the
 * last descriptor of every call is copied aside in front of it.  raster(): that copy -- width * height words, before
 * the >> 1 and the clamp -- to host memory; synchronises; NTSCSIM_E_ARG when nothing was kept.
 * set_window_rows(rows): caps the rows of k_scan_splat's on-chip window (0: every dot takes the spill path; a
 * negative value restores the default).  spill(): workgroups of the last call that drew a dot, and how many of them
 * spilled; synchronises.  All require ntscsim_scan_bind() and are kept across later binds. */
int  ntscsim_scan_debug_keep_raster(ntscsim_ctx *ctx, int on);
int  ntscsim_scan_debug_raster(ntscsim_ctx *ctx, uint32_t *out_host);
int  ntscsim_scan_debug_set_window_rows(ntscsim_ctx *ctx, int rows);
int  ntscsim_scan_debug_spill(ntscsim_ctx *ctx, uint64_t *workgroups, uint64_t *spilled);

/* ---- vhsled: the scanline left-edge aligner (ffmpeg_vhsled.cpp) ----
 * A capture whose scanlines start at wandering horizontal positions is lined up: the tool finds the left edge
 * of the picture in every row (the first run of nine pixels that are not "blackish" against the row's first
 * pixel), takes the mean of that edge over nine rows and moves every row left by the result.  Mapping:
 *
 *   globals :44-52 + preset_NTSC() :457-460 + parse_argv() :476-584     | ntscsim_led_params, _init(), _parse_argv()
 *   blackish() :682-692, the row walk :869-898                          | k_led_frames, the scan of a row
 *   the nine-row mean :900-906, the shifted copy :908-928               | k_led_frames, smoothing and shift
 *   the three together, per frame                                       | ntscsim_led_frames_device() / _frames_host()
 *
 * Decoding, scaling (sws_scale), encoding and the audio pass-through stay with the caller.
 * Frames are BGRA in device memory; a decoder's or the simulator's outputs can be handed over without a copy.
 * A frame carries no state into the next one, so a clip is a list of descriptors and there is no clip call.
 */
typedef struct ntscsim_led_params {
    uint32_t struct_size;            /* = sizeof(ntscsim_led_params)                                       */
    int32_t  width, height;          /* :50-51  -1 x -1: the tool then takes the input's size; -width / -height */
    int32_t  underscan;              /* :46  0 (-underscan, clamped to 0..99); recorded, not acted on       */
    int32_t  use_422_colorspace;     /* :48  false (-422 / -420); recorded, not acted on                    */
    int32_t  field_rate_num, field_rate_den;    /* 60000 / 1001 (preset_NTSC), -or                         */
    int32_t  _pad;
    double   gamma_correction;       /* :44  -1 (-gamma); recorded, not acted on                            */
    const char *input_path;          /* the last -i (points into argv), NULL if none: the tool has one input */
    const char *output_path;         /* -o                                                                  */
} ntscsim_led_params;

void ntscsim_led_params_init(ntscsim_led_params *p);
/* Mirror of parse_argv() :476-584: -i -o -or -width -height -gamma -underscan -422 -420, -h / -help (any number of
 * leading '-').  -width / -height go through strtoul with base 0 and the tool's cast to int, and a result below
 * 32 is refused; -gamma takes a number (isdigit / atof), "vga" or "ntsc" (2.2), and any other word leaves the value
 * alone; -underscan is atoi clamped to 0..99; -or is strtof, an optional : / \ denominator (strtoul base 10, at
 * least 1), a floor of 5 per second, and num / den = round(n) / d for d > 1, round(n * 10000) / 10000 otherwise.
 * The tool's pixel loop :866-931 reads none of gamma, underscan and 422: they are recorded here and change no byte.
 * -fa is in the tool's help text but not in its parser: an unknown switch here too.  argv[0] is the program name.
 * NTSCSIM_E_FLAG (the tool's "return 1") for an unknown switch, a bare word, a missing value and a size below 32;
 * require_io != 0 applies the "No output file / No input files" checks (:574-581).  NTSCSIM_E_HELP for -h / -help. */
int  ntscsim_led_parse_argv(ntscsim_led_params *p, int argc, const char *const *argv, int require_io);

/* Snapshot the parameters on a ctx (any ntscsim_params it was created with).  Waits for vhsled work in flight on
 * the ctx.  NTSCSIM_E_SIZE unless 16 <= width <= 3640 and 16 <= height <= 65536: the tool refuses a frame below
 * 16 x 16 (:717), its loop bound `y < (int)height - 4` is an unsigned comparison that misbehaves for small heights,
 * and its nine-row sum of edges, each up to width << 16, plus 5 must fit an int32 -- 9 * 3640 * 65536 + 5 does,
 * 9 * 3641 * 65536 + 5 does not, and past that the tool's arithmetic is undefined. */
int  ntscsim_led_bind(ntscsim_ctx *ctx, const ntscsim_led_params *p);

typedef struct ntscsim_led_desc {
    const void *src_dev;             /* device pointer, BGRA frame; never written                            */
    int32_t     src_linesize;        /* bytes, >= 4*width, multiple of 4                                     */
    int32_t     dst_linesize;        /* bytes, >= 4*width, multiple of 4                                     */
    void       *dst_dev;             /* device pointer, BGRA frame; bytes of a row behind 4*width are not touched */
    int32_t     width, height;       /* must be the bound params'                                            */
} ntscsim_led_desc;
/*
 * The tool's frame body :866-931 for `n` frames.  With in[y][i] the source pixels as uint32_t:
 *   e[y]    = the first x at which in[y][x .. x+8] are all not blackish, or width if there is none; a pixel is
 *             not blackish when one of its three low bytes exceeds the LOW byte of in[y][0] by 16 or more (the
 *             tool compares all three channels with the first pixel's blue; the top byte plays no part)
 *   adj2[y] = (sum of e[y-4 .. y+4] << 16, plus 5) / 9 for 4 <= y < height - 4, e[y] << 16 for the other rows
 *   x[y]    = (adj2[y] + 0x8000) >> 16
 *   out[y][i] = in[y][i + x[y]] for i < width - x[y] when x[y] < width / 2, in[y][i] for every other pixel
 * Pixels move as whole dwords.  All frame pointers are DEVICE pointers; `descs` is host memory and is consumed by the
 * call.  Enqueued on hip_stream (NULL: the ctx's own stream), returns without synchronising.  Descriptors take
 * effect in order: a later one that reads a frame an earlier one wrote sees the earlier result.
 * Kernel: k_led_frames, one launch for all descriptors that do not depend on each other, grid (bands of 16 rows,
 * frames).  A workgroup scans its rows and four rows above and below (one wavefront per row, the chunk's mask a
 * 64-bit ballot, the first 128 pixels of all of a wave's rows requested before the first wait), keeps the edges
 * on chip, smooths and moves its rows.  Destinations whose pointer and linesize are multiples of 16 are written as
 * 16-byte vectors; any other, and the last width % 4 pixels of a row, as dwords.  Same bytes either way.
 * NTSCSIM_E_SIZE: a size other than the bound params', a linesize below 4*width or not a multiple of 4, a pointer
 * that is not a multiple of 4.  NTSCSIM_E_ARG: a NULL pointer, no ntscsim_led_bind() before, a source that overlaps
 * its destination in any way -- rows are moved in parallel, which cannot be done in place, and the tool never does
 * it either.
 */
int  ntscsim_led_frames_device(ntscsim_ctx *ctx, const ntscsim_led_desc *descs, int n, void *hip_stream);
/* ntscsim_led_frames_device() on HOST frames, through pinned staging of the ctx.  Synchronous.  Same bytes as the
 * device call: the bytes the device call leaves alone keep what the host frame held. */
int  ntscsim_led_frames_host(ntscsim_ctx *ctx, const ntscsim_led_desc *descs, int n);
/* Debug taps.  keep_edges(on): while on, every frames call also writes e[y] and x[y] of each of its frames to a
 * plane of the ctx.  edges(frame, e_host, x_host): those of frame `frame` of the last frames call, `height` int32
 * each (either pointer may be NULL), so that a test can tell a wrong scan from a wrong copy; synchronises;
 * NTSCSIM_E_ARG when nothing was kept or `frame` is outside the last call.  Both require ntscsim_led_bind(). */
int  ntscsim_led_debug_keep_edges(ntscsim_ctx *ctx, int on);
int  ntscsim_led_debug_edges(ntscsim_ctx *ctx, int frame, int32_t *e_host, int32_t *x_host);

/* ---- filmac: the film auto-contrast (filmac.cpp) ----
 * A film transfer whose levels drift is stretched to full range frame by frame: the tool measures the darkest 128 x 128
 * block mean and the brightest pixel of the picture's middle, follows both from frame to frame with a recurrence that
 * opens the range fast and closes it slowly, and maps every B, G, R value linearly so that the followed range fills
 * the output, in linear light with -gamma.  Every decoded frame gives one output frame.  Mapping:
 *
 *   globals :40-56 + preset_NTSC() + parse_argv() :476-584              | ntscsim_filmac_params, _init(), _parse_argv()
 *   gamma16_do_init() :672-680                                          | ntscsim_blend_tables()    (the same text)
 *   the widening :857-884, the block statistics :886-923                | k_filmac_stats
 *   the frame levels of the blocks :887-925                             | k_filmac_frame_levels
 *   the recurrence :927-942                                             | k_filmac_levels (state in device memory)
 *   the stretch :946-954, the packing :979-1006                         | k_filmac_tables (a byte table per frame), k_filmac_apply
 *   all of it, per frame                                                | ntscsim_filmac_frames_device() / _frames_host()
 *
 * Decoding, scaling, encoding and the audio pass-through stay with the caller.  Frames are BGRA
 * in device memory.  The arithmetic is csrc/filmac_levels.hpp, one statement of it for the kernels and the host.
 */
/* The tool's switches are, text for text, ffmpeg_vhsled's (:40-56, :476-584), so the parameters are that struct and
 * the parser is that parser.  The one difference: filmac acts on gamma_correction -- above 1 the levels are measured
 * and stretched in linear light (:859, :886, :979). */
typedef ntscsim_led_params ntscsim_filmac_params;
void ntscsim_filmac_params_init(ntscsim_filmac_params *p);
int  ntscsim_filmac_parse_argv(ntscsim_filmac_params *p, int argc, const char *const *argv, int require_io);

/* Snapshot the parameters on a ctx, build the gamma tables when gamma_correction > 1, and reset the level state (the
 * tool's final_init = false).  Waits for filmac work in flight on the ctx.  NTSCSIM_E_SIZE unless 16 <= width, height
 * <= 16384: the tool refuses a frame below 16 x 16 (:705), and a block's sum stays inside 32 bits. */
int  ntscsim_filmac_bind(ntscsim_ctx *ctx, const ntscsim_filmac_params *p);

typedef struct ntscsim_filmac_desc {
    const void *src;                 /* device pointer, BGRA frame of the bound size                          */
    int32_t     src_linesize;        /* bytes, >= 4*width, multiple of 4                                     */
    int32_t     _pad0;
    void       *dst;                 /* device pointer; bytes of a row behind 4*width are not touched; may be src */
    int32_t     dst_linesize;        /* bytes, >= 4*width, multiple of 4                                     */
    int32_t     _pad1;
} ntscsim_filmac_desc;
/*
 * The tool's frame body :857-1006 for `n` frames, in order.  With S = 0x10000 * 8192 and L(c) = gamma_dec16(c) << 16
 * with gamma, S = 0x10000 * 256 and L(c) = c << 16 without:
 *   blocks    start at x = width*15/100, +128, ... < width*90/100 and y = 0, +128, ... < height (unsigned), are
 *             128 x 128 and clipped by the frame alone: the last block of a row runs past width*90/100
 *   maxv      = max(S*4/10, L of every B, G, R of every pixel of every block)
 *   minv      = min(S*6/10, per block: (sum of min(L_b, L_g, L_r) + count/2) / count);  minv == maxv: maxv++
 *   state     first frame: final_minv = minv, final_maxv = maxv.  Then final_maxv = (final_maxv + maxv) / 2 when it
 *             is below maxv, (4 final_maxv + maxv) / 5 otherwise; final_minv = (final_minv + minv) / 2 when it is
 *             above minv, (4 final_minv + minv) / 5 otherwise
 *   out       v = (L - final_minv) * S / (final_maxv - final_minv) in 64 bits, truncating; clamped to +-0x7FFFFFFF;
 *             t = max(0, v >> 16); the byte is gamma_enc16(min(t, 8192)) with gamma, min(t, 255) without; alpha 0xFF
 * The state lives in device memory and carries from descriptor to descriptor and from call to call without a host
 * round trip; calls on one ctx must be ordered by the caller (one stream, or events between streams).  final_maxv
 * stays above final_minv for every sequence of frames; after ntscsim_filmac_set_state() it may
 * not, and then a denominator of 0 counts as 1 and a negative one divides as the tool's signed division does.
 * All frame pointers are DEVICE pointers; `descs` is host memory and is consumed by the call.  Enqueued on hip_stream
 * (NULL: the ctx's own stream), returns without synchronising.  A later descriptor that reads a frame an earlier one
 * wrote sees the earlier result: it goes into a later launch group.  dst == src with equal linesizes (in place) is
 * allowed: the map reads a pixel before it writes it.
 * Kernels, per launch group: k_filmac_stats, grid (blocks, frames), a workgroup per block; k_filmac_frame_levels,
 * a wavefront per frame; k_filmac_levels, one workgroup, the recurrence by one lane; k_filmac_tables, grid (frames), a
 * 256-entry byte table per frame; k_filmac_apply, grid (bands of 8 rows, frames), the table in LDS.  Destinations whose pointer and linesize are
 * multiples of 16 are written as 16-byte vectors, any other, and the last width % 4 pixels of a row, as dwords; whole
 * quads of a source are read with one 16-byte load from their dword-aligned address.  Same bytes either way.
 * NTSCSIM_E_SIZE: a linesize below 4*width or not a multiple of 4, a pointer that is not a multiple of 4.
 * NTSCSIM_E_ARG: a NULL pointer, no ntscsim_filmac_bind() before, a source that overlaps its destination in any way
 * but in place.
 */
int  ntscsim_filmac_frames_device(ntscsim_ctx *ctx, const ntscsim_filmac_desc *descs, int n, void *hip_stream);
/* ntscsim_filmac_frames_device() on HOST frames, through pinned staging of the ctx.  Synchronous.  Same bytes as the
 * device call: the bytes the device call leaves alone keep what the host frame held. */
int  ntscsim_filmac_frames_host(ntscsim_ctx *ctx, const ntscsim_filmac_desc *descs, int n);

typedef struct ntscsim_filmac_state {
    int32_t init;                    /* final_init :829: 0 before the first frame                            */
    int32_t _pad;
    int64_t final_minv, final_maxv;  /* :828; meaningless while init is 0                                     */
} ntscsim_filmac_state;
/* The level state: reset() is the tool's start (bind does it too); get / set for a clip that is processed in pieces
 * or resumed.  All three wait for the device.  set: NTSCSIM_E_PARAM for a value outside +-2^32, which the stretch's
 * 64-bit product would not hold.  All require ntscsim_filmac_bind(). */
int  ntscsim_filmac_reset(ntscsim_ctx *ctx);
int  ntscsim_filmac_get_state(ntscsim_ctx *ctx, ntscsim_filmac_state *out);
int  ntscsim_filmac_set_state(ntscsim_ctx *ctx, const ntscsim_filmac_state *in);
/* Debug tap: minv, maxv, final_minv, final_maxv (in this order) of frame `frame` of the last frames call, so that a
 * test can tell wrong statistics from a wrong recurrence from a wrong map; the kernels pass these values through device
 * memory anyway, so nothing has to be switched on.  Synchronises.  NTSCSIM_E_ARG when `frame` is outside the last call. */
int  ntscsim_filmac_debug_levels(ntscsim_ctx *ctx, int frame, int64_t out[4]);
/* Developer timing (tools/bench_filmac.py).  time_kernels(on): while on, every frames call records events between its
 * kernels.  kernel_ms(): the time of k_filmac_stats, k_filmac_frame_levels, k_filmac_levels, k_filmac_tables and
 * k_filmac_apply of the last frames_device call, summed over its launch groups; synchronises; NTSCSIM_E_ARG when nothing was timed. */
int  ntscsim_filmac_debug_time_kernels(ntscsim_ctx *ctx, int on);
int  ntscsim_filmac_debug_kernel_ms(ntscsim_ctx *ctx, float out_ms[5]);

/* ---- the switches of the two pixel-map tools (ffmpeg_posterize.cpp, ffmpeg_colormap.cpp) ----
 * The two tools have the same globals, the same InputFile list and the same parse_argv() (posterize :620-696,
 * colormap :622-693) but for one switch: posterize has -threshhold, a number that belongs to the current input.  One
 * struct and one parser serve both; the stages' own names below are typedefs and thin wrappers, as filmac's are on
 * vhsled's.
 */
typedef struct ntscsim_pixmap_layer {
    const char *path;                /* the -i that opened the input (points into argv), may be NULL          */
    int32_t  threshhold;             /* posterize :71  3 (-threshhold): bits kept of every byte; an int, any value */
    int32_t  _pad;
} ntscsim_pixmap_layer;

typedef struct ntscsim_pixmap_params {
    uint32_t struct_size;            /* = sizeof(ntscsim_pixmap_params)                                     */
    int32_t  width, height;          /* 720 x 480 (preset_NTSC), 720 x 576 (-tvstd pal), -width             */
    int32_t  use_422_colorspace;     /* false (-422 / -420); recorded, not acted on                         */
    int32_t  field_rate_num, field_rate_den;    /* 60000 / 1001 (preset_NTSC), 50 / 1 (-tvstd pal)          */
    int32_t  output_pal;             /* 0 NTSC, 1 PAL (-tvstd)                                              */
    int32_t  n_layers;               /* inputs so far, in order; no upper limit                             */
    int32_t  layers_cap;             /* allocated entries of `layers`                                       */
    int32_t  _pad;
    ntscsim_pixmap_layer *layers;    /* heap block owned by the struct: ntscsim_pixmap_params_free()        */
    const char *output_path;         /* -o                                                                  */
} ntscsim_pixmap_params;

void ntscsim_pixmap_params_init(ntscsim_pixmap_params *p);
/* Releases the input list (the struct itself is the caller's). */
void ntscsim_pixmap_params_free(ntscsim_pixmap_params *p);
/* Mirror of both parse_argv(): -i -o -width -422 -420 -tvstd pal|ntsc, -h / -help (any number of leading '-'), and
 * -threshhold when with_threshhold != 0 (otherwise it is an unknown switch, as in ffmpeg_colormap).  -width and
 * -threshhold go through strtoul with base 0 and the tool's cast to int; a width below 32 is refused.  Every -i
 * appends an input that copies the threshhold of the one before (new_input_file(); 3 for the first), and -threshhold
 * sets that of the last input so far; before any -i the tool throws (current_input_file()): NTSCSIM_E_FLAG.  A value
 * outside 0..8 is recorded as the tool records it and refused by ntscsim_post_bind().  argv[0] is the program name.
 * NTSCSIM_E_FLAG (the tool's "return 1") for an unknown switch, a bare word, a missing value (-tvstd's too, which the
 * tool hands to strcmp as NULL), an unknown tv standard; require_io != 0 applies the "No output file / No input files"
 * checks.  NTSCSIM_E_HELP for -h / -help. */
int  ntscsim_pixmap_parse_argv(ntscsim_pixmap_params *p, int argc, const char *const *argv, int require_io, int with_threshhold);

/* ---- posterize: the bit-mask posteriser (ffmpeg_posterize.cpp) ----
 * Every byte of every pixel, alpha included, keeps its `threshhold` high bits.  Mapping:
 *
 *   globals + InputFile :71 + preset_NTSC() :604-611 + parse_argv() :620-696 | ntscsim_post_params, _init(), _free(), _parse_argv()
 *   composite_layer() :789-813                                          | k_post_frames
 *   the call site :1061, one layer of one frame                         | a descriptor of ntscsim_post_frames_device() / _frames_host()
 *
 * Decoding, scaling, encoding and the audio pass-through stay with the caller.  Frames are BGRA
 * in device memory.  A frame carries no state into the next one.
 */
typedef ntscsim_pixmap_params ntscsim_post_params;
void ntscsim_post_params_init(ntscsim_post_params *p);
void ntscsim_post_params_free(ntscsim_post_params *p);
int  ntscsim_post_parse_argv(ntscsim_post_params *p, int argc, const char *const *argv, int require_io);

/* Snapshot the parameters and the input list on a ctx.  Waits for posterize work in flight on the ctx.
 * NTSCSIM_E_SIZE unless 1 <= width, height <= 16384.  NTSCSIM_E_PARAM for an input whose threshhold is outside 0..8:
 * the tool's `0xFF << (8 - threshhold)` then shifts by a count that C leaves undefined.  The parameters are checked
 * before the ctx is looked at (a NULL ctx: NTSCSIM_E_ARG), so a host without a device can validate a command line. */
int  ntscsim_post_bind(ntscsim_ctx *ctx, const ntscsim_post_params *p);

typedef struct ntscsim_post_desc {
    const void *src;                 /* device pointer, BGRA frame of the bound size                          */
    int32_t     src_linesize;        /* bytes, >= 4*width, multiple of 4                                     */
    int32_t     _pad0;
    void       *dst;                 /* device pointer; bytes of a row behind 4*width are not touched; may be src */
    int32_t     dst_linesize;        /* bytes, >= 4*width, multiple of 4                                     */
    int32_t     layer;               /* index into the bound input list: whose threshhold masks the frame     */
} ntscsim_post_desc;
/*
 * composite_layer() :789-813 for `n` (frame, input) pairs, in order:
 *   mask = ((0xFF << (8 - threshhold)) & 0xFF) * 0x01010101;  out = in & mask
 * so threshhold 8 copies and threshhold 0 clears.  The tool's loop :1035-1062 calls this for every input in turn on
 * one output frame, each call overwriting all of it: a caller that wants the tool's frame passes the last input that
 * has a frame (or all of them, in order, with one dst: each goes into a launch group of its own).
 * All frame pointers are DEVICE pointers; `descs` is host memory and is consumed by the call.  Enqueued on hip_stream
 * (NULL: the ctx's own stream), returns without synchronising.  Descriptors take effect in order.  dst == src with
 * equal linesizes (in place) is allowed: a lane reads a pixel before it writes it.
 * Kernel: k_post_frames, one launch for all descriptors that do not depend on each other, grid (bands of 8 rows,
 * frames).  Destinations whose pointer and linesize are multiples of 16 are written as 16-byte vectors, any other, and
 * the last width % 4 pixels of a row, as dwords; whole quads of a source are read with one 16-byte load from their
 * dword-aligned address.  Same bytes either way.
 * NTSCSIM_E_SIZE: a linesize below 4*width or not a multiple of 4, a pointer that is not a multiple of 4.
 * NTSCSIM_E_ARG: a NULL pointer, no ntscsim_post_bind() before, a layer outside the bound list, a source that overlaps
 * its destination in any way but in place.
 */
int  ntscsim_post_frames_device(ntscsim_ctx *ctx, const ntscsim_post_desc *descs, int n, void *hip_stream);
/* ntscsim_post_frames_device() on HOST frames, through pinned staging of the ctx.  Synchronous.  Same bytes as the
 * device call: the bytes the device call leaves alone keep what the host frame held. */
int  ntscsim_post_frames_host(ntscsim_ctx *ctx, const ntscsim_post_desc *descs, int n);

/* ---- colormap: false colour through a table taken from a second picture (ffmpeg_colormap.cpp) ----
 * A 256-entry table of pixels is taken, before every output frame, from the middle scanline of the second input; the
 * first input's green byte then selects the output pixel from it.  Mapping:
 *
 *   globals + preset_NTSC() + parse_argv() :622-693                     | ntscsim_cmap_params, _init(), _free(), _parse_argv()
 *   colormap[256] :58, its start value :833                             | device memory of the ctx; ntscsim_cmap_reset(), _get_table(), _set_table()
 *   take_colormap() :785-799                                            | the table fill of k_cmap_frames; k_cmap_take
 *   composite_layer() :802-822                                          | k_cmap_frames
 *   the call site :1072-1075, one output frame                          | a descriptor of ntscsim_cmap_frames_device() / _frames_host()
 *
 * Decoding, scaling, encoding and the audio pass-through stay with the caller.
 */
typedef ntscsim_pixmap_params ntscsim_cmap_params;
void ntscsim_cmap_params_init(ntscsim_cmap_params *p);
void ntscsim_cmap_params_free(ntscsim_cmap_params *p);
int  ntscsim_cmap_parse_argv(ntscsim_cmap_params *p, int argc, const char *const *argv, int require_io);

/* Snapshot the parameters on a ctx and reset the table to the tool's start, colormap[i] = i * 0x01010101 (:833).
 * Waits for colormap work in flight on the ctx.  NTSCSIM_E_SIZE unless 1 <= width, height <= 16384. */
int  ntscsim_cmap_bind(ntscsim_ctx *ctx, const ntscsim_cmap_params *p);

typedef struct ntscsim_cmap_desc {
    const void *src;                 /* device pointer, BGRA frame of the bound size: the first input         */
    int32_t     src_linesize;        /* bytes, >= 4*width, multiple of 4                                     */
    int32_t     _pad0;
    void       *dst;                 /* device pointer; bytes of a row behind 4*width are not touched; may be src */
    int32_t     dst_linesize;        /* bytes, >= 4*width, multiple of 4                                     */
    int32_t     _pad1;
    const void *map;                 /* device pointer, BGRA frame of the bound size: the second input; NULL when
                                      * there is none (no second -i, or a file without video): the table stays    */
    int32_t     map_linesize;        /* bytes, >= 4*width, multiple of 4; ignored when map is NULL             */
    int32_t     _pad2;
} ntscsim_cmap_desc;
/*
 * The tool's :1072-1075 for `n` output frames, in order.  With the pixels as uint32_t (B | G<<8 | R<<16 | A<<24):
 *   map != NULL:  table[i] = map[height / 2][(i * width) / 256] for i < 256, whole dwords, unsigned and truncating
 *   out[y][x]   = table[(src[y][x] >> 8) & 0xFF]
 * A second input that has not decoded a frame yet is an all-zero frame in the tool (:198), not an absent one: pass
 * zeros.  The table lives in device memory and carries from descriptor to descriptor and from call to call without a
 * host round trip; calls on one ctx must be ordered by the caller (one stream, or events between streams).
 * All frame pointers are DEVICE pointers; `descs` is host memory and is consumed by the call.  Enqueued on hip_stream
 * (NULL: the ctx's own stream), returns without synchronising.  Descriptors take effect in order: a later one that
 * reads a frame (a map's middle row too) an earlier one wrote goes into a later launch group.  dst == src with equal
 * linesizes (in place) is allowed.
 * Kernels, per launch group: k_cmap_frames, grid (bands of 8 rows, frames): every workgroup fills a 256-dword table in
 * LDS from the middle row of the nearest map at or before its descriptor in the group, or from the ctx's table when
 * there is none, and gathers from it; then k_cmap_take, 256 lanes, which writes the ctx's table from the group's last
 * map (not launched when the group has none).  Vector and dword forms as for posterize.
 * NTSCSIM_E_SIZE: a linesize below 4*width or not a multiple of 4, a pointer that is not a multiple of 4.
 * NTSCSIM_E_ARG: a NULL src or dst, no ntscsim_cmap_bind() before, a source that overlaps its destination in any way
 * but in place, a destination that overlaps the middle row of its own map.
 */
int  ntscsim_cmap_frames_device(ntscsim_ctx *ctx, const ntscsim_cmap_desc *descs, int n, void *hip_stream);
/* ntscsim_cmap_frames_device() on HOST frames, through pinned staging of the ctx.  Synchronous.  Same bytes as the
 * device call; of a map only the middle row travels. */
int  ntscsim_cmap_frames_host(ntscsim_ctx *ctx, const ntscsim_cmap_desc *descs, int n);
/* The table: reset() is the tool's start (bind does it too); get / set for a clip that is processed in pieces, and
 * for a test to tell a wrong table from a wrong gather.  All three wait for the device and require ntscsim_cmap_bind(). */
int  ntscsim_cmap_reset(ntscsim_ctx *ctx);
int  ntscsim_cmap_get_table(ntscsim_ctx *ctx, uint32_t out[256]);
int  ntscsim_cmap_set_table(ntscsim_ctx *ctx, const uint32_t in[256]);

/* ------------------------------------------------------------------------------------------
 * The VHS audio chain of ffmpeg_ntsc and ffmpeg_to_composite as a device stage: composite_audio_process()
 * (ffmpeg_ntsc.cpp:889-970, filters :74-203, set-up :2031-2067; the sibling's :558-627 and :2126-2162 are the same
 * text).  Interleaved int16 in and out, bit-identical to the tool, the rand() draws of the hiss included: they come
 * from the ctx's stream position, which the call advances as the field calls do, so that fields and audio blocks
 * called in the tool's order reproduce the tool's stream.  DESIGN.md 7l.
 */
typedef struct ntscsim_audio_params {
    uint32_t struct_size;          /* sizeof(ntscsim_audio_params)                                              */
    int32_t  enabled;              /* enable_audio_emulation :799; 0 (-nocomp): a copy that draws nothing        */
    int32_t  channels;             /* output_audio_channels :1229-1262                                          */
    int32_t  rate;                 /* output_audio_rate :212  44100                                             */
    int32_t  passes;               /* :2035  6 (the only value the stage runs)                                   */
    int32_t  hifi;                 /* output_vhs_hifi                                                           */
    int32_t  preemphasis;          /* emulating_preemphasis                                                     */
    int32_t  deemphasis;           /* emulating_deemphasis                                                      */
    int32_t  hiss_level;           /* (int)(dBFS(output_audio_hiss_db) * 5000) :1267                            */
    int32_t  tv_standard;          /* NTSCSIM_TV_NTSC / NTSCSIM_TV_PAL                                          */
    int32_t  vsync_lines;          /* :905  525 / 625                                                           */
    int32_t  vpulse_end;           /* :906  10 / 12                                                             */
    double   lowpass_hz;           /* output_audio_lowpass                                                      */
    double   highpass_hz;          /* output_audio_highpass                                                     */
    double   emphasis_hz;          /* :2047 / :2052  16000 (Hi-Fi) or 8000 (linear)                             */
    double   boost_hz;             /* :2040  10000                                                              */
    double   hsync_hz;             /* :904  15734 / 15625                                                       */
    double   hpulse_end;           /* :907  hsync_hz * (4.7 or 4.0 us)                                          */
    double   buzz;                 /* dBFS(output_audio_linear_buzz) :903, libm pow on the host                  */
    double   boost_gain;           /* vhs_linear_high_boost                                                     */
    double   alpha_lowpass, alpha_highpass, alpha_pre, alpha_post, alpha_boost; /* LowpassFilter::setFilter :78  */
} ntscsim_audio_params;
/* From what the two parsers record: the post-parse derivation :1229-1267 and the set-up :2031-2067.  `cli` is the one
 * the parser filled next to `p` (either tool's).  NTSCSIM_E_ARG for a NULL pointer or a wrong struct_size of p. */
int  ntscsim_audio_params_from_cli(ntscsim_audio_params *ap, const ntscsim_params *p, const ntscsim_cli *cli);

typedef struct ntscsim_audio_state {
    double   bandpass[2][12];      /* per channel: the six low-pass states, then the six high-pass states        */
    double   pre[2], post[2];      /* audio_linear_preemphasis_pre / _post: SHARED by the channels (:920, :960)  */
    double   boost[2];             /* audio_post_vhs_boost, per channel                                         */
    uint64_t count;                /* audio_proc_count :889                                                     */
} ntscsim_audio_state;

typedef struct ntscsim_audio_desc {
    const int16_t *src;            /* device pointer, `samples` frames of `channels` interleaved int16           */
    int16_t       *dst;
    uint32_t       samples;        /* sample frames, as composite_audio_process()'s second argument; 0 allowed   */
    uint32_t       _pad;
    uint64_t       rng_pos;        /* rand() position of the block's first draw, or NTSCSIM_RNG_AUTO             */
} ntscsim_audio_desc;

typedef struct ntscsim_audio_stats {
    uint64_t segments;             /* of the last call                                                          */
    uint64_t repaired;             /* segments of it that k_audio_verify_repair ran again                        */
} ntscsim_audio_stats;

/* Snapshot the parameters and reset the state (zeros, count 0).  Waits for audio work in flight.
 * NTSCSIM_E_PARAM: channels outside 1..2, passes != 6, a rate or cut-off <= 0. */
int  ntscsim_audio_bind(ntscsim_ctx *ctx, const ntscsim_audio_params *ap);
/*
 * The n blocks are ONE continuous stream, in order: filter states and the sample count run through them (and on into
 * the next call).  Each block has its own rand() position, because the tool's audio packets interleave with its
 * fields; NTSCSIM_RNG_AUTO continues from the ctx's position.  The ctx's position moves at call time, by
 * samples * channels per block when hiss_level != 0.  Pointers are DEVICE pointers; `descs` is host memory and is
 * consumed by the call.  Enqueued on hip_stream (NULL: the ctx's own stream), returns without synchronising.
 * Kernels: k_audio_hiss (the draws, by jump-ahead, when hiss_level != 0), k_audio_pulses (sync pulse counts, when the
 * buzz is on), k_audio_segments (segments of the stream run speculatively from a zero state one warm-up early, each by
 * a group of 21 adjacent lanes, one lane per stage of the chain), k_audio_verify_repair (one workgroup: compares each
 * segment's recorded start state bitwise with its predecessor's true end state, runs it again where they differ,
 * writes the ctx's state).  The result never depends on the plan.  Calls on one ctx must be ordered by the caller (one
 * stream, or events between streams): they share the ctx's state and scratch.
 * NTSCSIM_E_ARG: no ntscsim_audio_bind() before, a NULL or odd pointer in a block with samples, a dst that overlaps
 * any src of the call (a warm-up reads input again).
 */
int  ntscsim_audio_device(ntscsim_ctx *ctx, const ntscsim_audio_desc *descs, int n, void *hip_stream);
/*
 * Many independent streams in one call.  A track is what one ntscsim_audio_device() call takes: blocks that form ONE
 * continuous stream.  The call equals, in bytes, end states and the ctx's rand() position, this sequence for
 * t = 0 .. n_tracks-1 in order: ntscsim_audio_set_state(*tracks[t].state), ntscsim_audio_device(blocks of t),
 * ntscsim_audio_get_state(tracks[t].state) -- but the tracks run side by side in one launch of each kernel, nothing
 * waits for the device, and the ctx's own carried state is neither read nor written.  All tracks use the parameters of
 * the last ntscsim_audio_bind().  rand() positions: as above, each block carries its own; NTSCSIM_RNG_AUTO continues
 * from the ctx's position, tracks in order and blocks in order within a track; the ctx's position moves at call time.
 * A track's sample count (the sync buzz) runs from its state's count.  Tracks without frames and blocks without
 * samples may stand anywhere; a track without frames leaves its state as it is.  With enabled == 0 the call copies,
 * draws nothing and leaves the states alone.  `tracks` and the block arrays are host memory, consumed by the call.
 * Enqueued on hip_stream (NULL: the ctx's own stream), returns without synchronising.
 * Kernels: k_audio_hiss, k_audio_track_pulses (when the buzz is on), k_audio_track_segments (group g of workgroup b
 * takes segment 3 b + g of the call and finds its track in the track table), k_audio_track_verify (one workgroup per
 * track: the verify / repair walk over that track's records, then its state).  The result never depends on the plan.
 * NTSCSIM_E_ARG, before anything is enqueued or the rand() position moves: no ntscsim_audio_bind() before, n_tracks
 * < 0, a NULL `tracks` or `blocks` that should hold something, a NULL or odd pointer in a block with samples, a state
 * that is not 8-byte aligned, two tracks whose states overlap, a dst of any track that overlaps a src of any track.
 */
typedef struct ntscsim_audio_track {
    const ntscsim_audio_desc *blocks;   /* host memory: this track's blocks, ONE continuous stream                    */
    int32_t                   n_blocks;
    int32_t                   _pad;
    ntscsim_audio_state      *state;    /* DEVICE pointer, 8-byte aligned, read at the start and written at the end;
                                           NULL: start from zeros / count 0, end state discarded                     */
} ntscsim_audio_track;
int  ntscsim_audio_tracks_device(ntscsim_ctx *ctx, const ntscsim_audio_track *tracks, int n_tracks, void *hip_stream);
/*
 * Many independent streams in one call, EACH WITH ITS OWN PARAMETERS: a tracks call whose tracks name a set of `sets`
 * (Hi-Fi stereo next to linear mono, SP next to LP and EP, NTSC buzz next to PAL buzz, different hiss levels).  The
 * call equals, in output bytes, every track's end state and count and the ctx's rand() position, this sequence for
 * t = 0 .. n_tracks-1 in order: ntscsim_audio_bind(set of track t), ntscsim_audio_set_state(*tracks[t].state),
 * ntscsim_audio_device(blocks of t), ntscsim_audio_get_state(tracks[t].state) -- but the tracks run side by side in one
 * launch of each kernel however many sets there are, nothing waits for the device, and the ctx's own carried state and
 * bound parameters are neither read (except through set == -1) nor written.
 * Frame size: a block of track t holds samples * channels(set of t) int16; the frame size is the track's, so mono and
 * stereo tracks stand in one call.
 * rand() positions: tracks go in order, and blocks in order within a track; NTSCSIM_RNG_AUTO continues from the ctx's
 * position; a block advances the position by samples * channels only when ITS track's hiss_level != 0; the position
 * moves at call time.
 * Buzz: each track's sync buzz runs from its own state's count with its own hsync_hz, vsync_lines and pulse ends; a PAL
 * track and an NTSC track can share a wavefront.
 * Disabled tracks: a track whose set has enabled == 0 is copied; it draws nothing (its blocks' rng_pos are not looked
 * at, as ntscsim_audio_device() does not look at them), keeps its state and reports zero segments.  Its neighbours run
 * the chain.
 * Warm-up: with the default plan each track's warm-up is its own set's (72 time constants of ITS high-pass: 25,280
 * frames at 20 Hz, 5,056 at 100 Hz), so each track is planned exactly as a lone call of its frames would be.
 * ntscsim_audio_debug_set_plan overrides it for all tracks as it does for the other calls; the segment length is
 * call-wide.
 * ntscsim_audio_debug_track_stats and ntscsim_audio_debug_kernel_ms work after a mixed call as they do after a tracks
 * call; ntscsim_debug_last_kernels names the kernels that ran: k_audio_hiss (when a track draws; the level is per
 * block), k_audio_mixed_pulses (when a track's buzz is on; tracks without buzz are skipped), k_audio_mixed_segments (a
 * group of 21 lanes takes the cfg of its segment's track from the call's set table), k_audio_mixed_verify.
 * A previous ntscsim_audio_bind() is required: it owns the stage's scratch and polynomials.  n_sets == 0 with every
 * set == -1 is allowed.  `sets`, `tracks` and the block arrays are host memory, consumed by the call.
 * Refused before anything is enqueued or the rand() position moves -- NTSCSIM_E_ARG: everything
 * ntscsim_audio_tracks_device refuses, the overlap checks in each track's own frame size; a `set` outside
 * -1 .. n_sets-1; n_sets < 0; a NULL `sets` that should hold something; a set some track names with a wrong
 * struct_size.  NTSCSIM_E_PARAM: a set some track names that ntscsim_audio_bind() would refuse.  Sets that no track
 * names are not looked at.
 */
typedef struct ntscsim_audio_mixed_track {
    const ntscsim_audio_desc *blocks;   /* host memory: ONE continuous stream, as in ntscsim_audio_track               */
    int32_t                   n_blocks;
    int32_t                   set;      /* index into `sets`; -1: the parameters of the last ntscsim_audio_bind()      */
    ntscsim_audio_state      *state;    /* DEVICE pointer, 8-byte aligned; NULL: zeros / count 0, end discarded        */
} ntscsim_audio_mixed_track;
int  ntscsim_audio_mixed_tracks_device(ntscsim_ctx *ctx, const ntscsim_audio_params *sets, int n_sets,
                                       const ntscsim_audio_mixed_track *tracks, int n_tracks, void *hip_stream);
/* The same call on HOST memory: the block pointers (any alignment) and the states are host memory, dst may equal src
 * (results are written after every source has been read; other overlaps are the caller's business).  Synchronous.  It
 * goes through pinned staging of the ctx in ONE device call, not one per track, and returns the same bytes, states and
 * position as the device call.  Two tracks on one state: NTSCSIM_E_ARG. */
int  ntscsim_audio_mixed_tracks_host(ntscsim_ctx *ctx, const ntscsim_audio_params *sets, int n_sets,
                                     const ntscsim_audio_mixed_track *tracks, int n_tracks);
/* Drop-in for composite_audio_process(audio, samples): HOST memory, in place, through pinned staging of the ctx.
 * Synchronous.  The rand() position is the ctx's. */
int  ntscsim_audio_host(ntscsim_ctx *ctx, int16_t *audio, uint32_t samples);
/* reset: the tool's start.  get / set: a track processed in pieces, or started at any sample count.  All wait for
 * the device and require ntscsim_audio_bind(). */
int  ntscsim_audio_reset(ntscsim_ctx *ctx);
int  ntscsim_audio_get_state(ntscsim_ctx *ctx, ntscsim_audio_state *out);
int  ntscsim_audio_set_state(ntscsim_ctx *ctx, const ntscsim_audio_state *in);
/* Debug taps.  set_plan: segment length and warm-up in frames.  (0, 0) restores both defaults (4096 frames; 72 time
 * constants of the high-pass, up to a multiple of 64); with any other pair the warm-up is taken as given (0: none) and a
 * seg_len of 0 is the default length.  seg_len >= the call's frames is the serial form.  pulses: the device's pulse counts of frames count0 .. count0+n-1 (host `out`). */
int  ntscsim_audio_debug_set_plan(ntscsim_ctx *ctx, uint32_t seg_len, uint32_t warmup);
int  ntscsim_audio_debug_stats(ntscsim_ctx *ctx, ntscsim_audio_stats *out);
/* stats of tracks 0 .. n_tracks-1 of the last ntscsim_audio_tracks_device() or mixed tracks call (n_tracks beyond that call's:
 * NTSCSIM_E_ARG).  Waits for the device. */
int  ntscsim_audio_debug_track_stats(ntscsim_ctx *ctx, ntscsim_audio_stats *out, int n_tracks);
int  ntscsim_audio_debug_pulses(ntscsim_ctx *ctx, uint64_t count0, uint32_t n, uint8_t *out);
int  ntscsim_audio_debug_time_kernels(ntscsim_ctx *ctx, int on);
/* (k_audio_hiss + k_audio_pulses, k_audio_segments, k_audio_verify_repair) milliseconds of the last call; after a
 * tracks call (k_audio_hiss + k_audio_track_pulses, k_audio_track_segments, k_audio_track_verify), after a mixed
 * tracks call their k_audio_mixed_* counterparts */
int  ntscsim_audio_debug_kernel_ms(ntscsim_ctx *ctx, float out_ms[3]);

/* ------------------------------------------------------------------------------------------
 * ffmpeg_cassette's tape chain as a device stage: composite_audio_process() of ffmpeg_cassette.cpp:334-416 (filters
 * :80-209, ConvolutionMap :278-324, set-up :864-880).  It is the VHS chain without buzz and boost, plus a per-sample
 * FIR between hiss and de-emphasis whose taps follow a head tilt that wavers with sin(), mirrored between left and
 * right, and an integer mono downmix behind the pack.  Interleaved int16 stereo in and out, bit-identical to the tool
 * on the host that makes the call: the per-frame sin() is libm's, evaluated by the host and uploaded, never by the
 * device.  The hiss draws come from the ctx's rand() position, as the audio stage's do.  DESIGN.md 7m.
 */
#define NTSCSIM_CASS_MAX_TAPS 512  /* enough for |headalign| <= 100 */
typedef struct ntscsim_cass_params {
    uint32_t struct_size;          /* sizeof(ntscsim_cass_params)                                               */
    int32_t  channels;             /* output_audio_channels :448  2, the tool never changes it                   */
    int32_t  rate;                 /* output_audio_rate :236  44100                                             */
    int32_t  passes;               /* :868  6                                                                   */
    int32_t  preemphasis;          /* -preemphasis <n>: n > 0                                                    */
    int32_t  deemphasis;           /* -deemphasis <n>: n > 0                                                     */
    int32_t  mono;                 /* -mono                                                                     */
    int32_t  hiss_level;           /* derived: (int)(dBFS(hiss_db) * 5000) :582, libm pow on the host            */
    int32_t  taps;                 /* derived: (int)floor(fabs(tilt*2) + fabs(tilt*3) + 7.5) :338                */
    int32_t  audio_stream_index;   /* -a <n> / -an (-1): recorded, never used                                    */
    double   hiss_db;              /* -audio-hiss, -45                                                          */
    double   lowpass_hz;           /* -low (int)strtoul, presets; 20000                                         */
    double   highpass_hz;          /* -high (int)strtoul, presets; 20                                           */
    double   emphasis_hz;          /* :873 / :878  4000 for both filters                                        */
    double   head_tilt;            /* -headalign atoi, presets; 0.2                                             */
    double   head_tilt_waver;      /* -headalignwaver atoi, presets; 0.5                                        */
    double   transcode_start, transcode_end, transcode_dur; /* -ss -se -t: recorded, never used                   */
    double   alpha_lowpass, alpha_highpass, alpha_pre, alpha_post; /* derived: LowpassFilter::setFilter :84      */
    const char *input_path, *output_path; /* -i / -o: point into argv; recorded, never used by the stage         */
} ntscsim_cass_params;
/* the tool's initial values (:235-248, :327-332, :446-448), derived fields included */
void ntscsim_cass_params_init(ntscsim_cass_params *p);
/* Mirror of parse_argv() :441-590; later switches override earlier ones.  argv[0] is the program name.  require_io != 0
 * applies the tool's "You must specify an input and output file".  Ends with ntscsim_cass_params_derive().
 * NTSCSIM_OK, NTSCSIM_E_HELP (-h / -help), NTSCSIM_E_FLAG (the tool's "return 1", or a switch without its value), or
 * what the derivation answers. */
int  ntscsim_cass_parse_argv(ntscsim_cass_params *p, int argc, const char *const *argv, int require_io);
/* hiss_level, taps and the four alphas from the fields above them.  NTSCSIM_E_ARG: a cut-off of 0 (the tool's
 * HiLoComboPass::init() returns without filters and its assert :335 ends it).  NTSCSIM_E_PARAM: a cut-off below 0, more
 * than NTSCSIM_CASS_MAX_TAPS taps, a hiss level outside int. */
int  ntscsim_cass_params_derive(ntscsim_cass_params *p);

typedef struct ntscsim_cass_state {
    double   bandpass[2][12];      /* per channel: the six low-pass states, then the six high-pass states        */
    double   pre[2];               /* audio_linear_preemphasis_pre: SHARED by the channels (:383)                */
    uint64_t count;                /* audio_proc_count :276                                                     */
    double   post[2];              /* audio_linear_preemphasis_post: shared as well (:403)                       */
    uint32_t taps;                 /* of the params the state belongs to                                        */
    uint32_t _pad;
    double   history[NTSCSIM_CASS_MAX_TAPS - 1][2]; /* the FIR's delay line: [k][c] is the value in front of the
                                    * FIR of channel c, taps-1-k frames before the next frame; k < taps-1 are used */
} ntscsim_cass_state;

typedef struct ntscsim_cass_desc {
    const int16_t *src;            /* device pointer, `samples` frames of 2 interleaved int16                     */
    int16_t       *dst;
    uint32_t       samples;        /* sample frames, as composite_audio_process()'s second argument; 0 allowed   */
    uint32_t       _pad;
    uint64_t       rng_pos;        /* rand() position of the block's first draw, or NTSCSIM_RNG_AUTO             */
} ntscsim_cass_desc;

typedef struct ntscsim_cass_stats {
    uint64_t segments;             /* of the last call                                                          */
    uint64_t repaired_front;       /* segments of it that k_cass_front_verify ran again                          */
    uint64_t repaired_back;        /* segments of it that k_cass_back_verify ran again (0 without de-emphasis)    */
} ntscsim_cass_stats;

/* Snapshot the parameters and reset the state (zeros, count 0).  Waits for cassette work in flight.  Does not touch a
 * bound audio stage.  NTSCSIM_E_PARAM: channels != 2, passes != 6, rate <= 0, a cut-off <= 0, taps that are not
 * cass_taps(head_tilt) or outside 1..NTSCSIM_CASS_MAX_TAPS, a hiss level below 0. */
int  ntscsim_cass_bind(ntscsim_ctx *ctx, const ntscsim_cass_params *cp);
/*
 * The n blocks are ONE continuous stream, as ntscsim_audio_device()'s are; the same rules for rand() positions, device
 * pointers, stream order and overlap hold.  The host evaluates head_tilt_final of every frame (libm sin) into pinned
 * staging of the ctx -- after it has enqueued the front's kernels, so the two overlap; a call of 2^18 frames or more
 * splits the fill over four threads, a fixed number -- and uploads it on the call's stream.  Kernels: k_audio_hiss (the draws), k_cass_front (band-pass,
 * pre-emphasis, clip, hiss: the speculative lane pipeline, doubles into a scratch plane), k_cass_front_verify (ordered
 * walk, repairs), k_cass_conv (the FIR, parallel over frames from an LDS tile; packs and stores without de-emphasis),
 * and with de-emphasis k_cass_back + k_cass_back_verify (the two shared poles, pack, downmix; speculative again).
 * NTSCSIM_E_ARG: no ntscsim_cass_bind() before, a NULL or odd pointer in a block with samples, a dst that overlaps any
 * src of the call.
 */
int  ntscsim_cass_device(ntscsim_ctx *ctx, const ntscsim_cass_desc *descs, int n, void *hip_stream);
/*
 * Many independent tapes in one call.  A track is what one ntscsim_cass_device() call takes: blocks that form ONE
 * continuous stream.  The call equals, in output bytes, end states (the FIR's history included) and the ctx's rand()
 * position, this sequence for t = 0 .. n_tracks-1 in order: ntscsim_cass_set_state(*tracks[t].state with its count set
 * to tracks[t].count and its taps to the bound ones), ntscsim_cass_device(blocks of t),
 * ntscsim_cass_get_state(tracks[t].state) -- but the tracks run side by side in one launch of each kernel, nothing
 * waits for the device, and the ctx's own carried state and its host-side count are neither read nor written.  All
 * tracks use the parameters of the last ntscsim_cass_bind().
 * State on entry and exit: the `count` and `taps` fields of a state are IGNORED on entry -- the sines of a track are
 * the host's, made from tracks[t].count, which the host knows without asking the device; that is also what makes a
 * zero-filled device buffer a fresh track -- and written on exit as count + frames and the bound taps.  A track shorter
 * than taps - 1 frames keeps the rest of its old history, as a short call does.  Tracks without frames and blocks
 * without samples may stand anywhere; a track without frames leaves its state as it is, count and taps included.
 * rand() positions: as above, each block carries its own; NTSCSIM_RNG_AUTO continues from the ctx's position, tracks in
 * order and blocks in order within a track; the ctx's position moves at call time, by 2 * samples per block when
 * hiss_level != 0.  The tilt table is made once over the UNION of the tracks' ranges [count, count + frames): tracks
 * that cover the same counts share their sines (ntscsim_cass_debug_tilt_frames).  The cassette parameters have no
 * `enabled`: there is no copying mode.  `tracks` and the block arrays are host memory, consumed by the call.
 * Enqueued on hip_stream (NULL: the ctx's own stream), returns without synchronising.
 * Kernels: k_audio_hiss, k_cass_track_front (group g of workgroup b takes segment 3 b + g of the call and finds its
 * track in the track table), k_cass_track_front_verify (one workgroup per track: its history laid in front of its
 * section of x, the verify / repair walk over its records), k_cass_track_conv (one workgroup per tile of the call; a
 * tile never crosses a track; the first tile of a track writes its new history), and with de-emphasis
 * k_cass_track_back (one lane per segment of the call) + k_cass_track_back_verify (one lane per track).  The result
 * never depends on the plan.
 * NTSCSIM_E_ARG, before anything is enqueued or the rand() position moves: no ntscsim_cass_bind() before, n_tracks
 * < 0, a NULL `tracks` or `blocks` that should hold something, a NULL or odd pointer in a block with samples, a state
 * that is not 8-byte aligned, two tracks whose states overlap, a dst of any track that overlaps a src of any track,
 * count + frames of a track overflowing 64 bits.
 */
typedef struct ntscsim_cass_track {
    const ntscsim_cass_desc *blocks;   /* host memory: this track's blocks, ONE continuous stream                     */
    int32_t                  n_blocks;
    int32_t                  _pad;
    uint64_t                 count;    /* audio_proc_count of the track's first frame: the HOST's knowledge, used for
                                          the sines and for the state's count                                         */
    ntscsim_cass_state      *state;    /* DEVICE pointer, 8-byte aligned, read at the start and written at the end;
                                          NULL: start from zeros, end state discarded                                 */
} ntscsim_cass_track;
int  ntscsim_cass_tracks_device(ntscsim_ctx *ctx, const ntscsim_cass_track *tracks, int n_tracks, void *hip_stream);
/*
 * The tracks call with parameters PER TRACK: a library of tapes, a worn deck (-preset 3, 57 taps) next to a good one (8
 * taps), mono next to stereo, de-emphasis on some, a hiss level and a band limit each.  Track t names one of `sets`
 * (set == -1: the parameters of the last ntscsim_cass_bind()).  The call equals, in output bytes, in every end state
 * (the 28 filter values, the FIR history of THAT track's taps - 1 frames, count, taps) and in the ctx's rand() position,
 * this sequence for t = 0 .. n_tracks-1 in order: ntscsim_cass_bind(set of t), ntscsim_cass_set_state(*state_t with
 * count = tracks[t].count and taps = that set's), ntscsim_cass_device(blocks of t), ntscsim_cass_get_state(state_t) --
 * but each kernel is launched once however many sets there are, nothing waits for the device, and the ctx's bound
 * parameters, carried state and host-side count are neither read (except through set == -1) nor written.
 * State on entry and exit: as ntscsim_cass_tracks_device(), with "the bound taps" read as "the taps of the track's
 * set": count and taps are ignored on entry and written on exit; a track shorter than its own taps - 1 keeps the rest
 * of its history; tracks without frames are left alone.
 * rand() positions: tracks in order, blocks in order within a track; a block advances the position by 2 * samples only
 * when ITS track's hiss_level != 0; the position moves at call time.
 * Warm-up: with the default plan the front's warm-up of a track is its own set's (72 time constants of ITS high-pass:
 * 25,280 frames at 20 Hz, 5,056 at 100 Hz), so each track is planned exactly as a lone call of its frames would be;
 * ntscsim_cass_debug_set_plan overrides it for all tracks.  Segment length and the back's warm-up are call-wide.
 * Sines: the table the FIR reads holds sin() of each sample count -- it depends on the count and the rate alone -- over
 * the union of [count, count + frames) of the tracks whose sets share a rate, one union per distinct rate; the device
 * makes head_tilt_final = (waver * s) + tilt from it per frame with the track's tilt and waver, the same two rounded
 * operations the tool performs.  Tracks on different decks that cover the same counts share their sines
 * (ntscsim_cass_debug_tilt_frames).  The host calls sin(); the device never does.
 * Kernels (ntscsim_debug_last_kernels): k_audio_hiss (when some track draws; blocks of tracks that draw nothing are not
 * in its launch), k_cass_mixed_front (a lane takes what its stage reads of its track's cfg from the call's set table
 * in front of the run), k_cass_mixed_front_verify, k_cass_mixed_conv (the halo of a tile is its track's taps - 1; a
 * track without de-emphasis is packed, stored and closed here), and -- only if some track that has frames has
 * de-emphasis -- k_cass_mixed_back and k_cass_mixed_back_verify, which skip the tracks that have none.
 * ntscsim_cass_debug_track_stats, _tilt_frames, _kernel_ms (the same eight slots) and _set_plan work as after a tracks
 * call; repaired_back of a track without de-emphasis is 0.
 * A previous ntscsim_cass_bind() is required: it owns the stage's scratch and polynomials.  n_sets == 0 with every
 * set == -1 is allowed.  `sets`, `tracks` and the block arrays are host memory, consumed by the call.
 * Refused before anything is enqueued or the rand() position moves -- NTSCSIM_E_ARG: everything
 * ntscsim_cass_tracks_device refuses; a `set` outside -1 .. n_sets-1; n_sets < 0; a NULL `sets` that should hold
 * something; a set some track names with a wrong struct_size.  NTSCSIM_E_PARAM: a set some track names that
 * ntscsim_cass_bind() would refuse.  Sets that no track names are not looked at.
 */
typedef struct ntscsim_cass_mixed_track {
    const ntscsim_cass_desc *blocks;   /* host memory: ONE continuous stream, as in ntscsim_cass_track                */
    int32_t                  n_blocks;
    int32_t                  set;      /* index into `sets`; -1: the parameters of the last ntscsim_cass_bind()       */
    uint64_t                 count;    /* the HOST's audio_proc_count of the first frame, as in ntscsim_cass_track    */
    ntscsim_cass_state      *state;    /* DEVICE pointer, 8-byte aligned; NULL: zeros, end discarded                  */
} ntscsim_cass_mixed_track;
int  ntscsim_cass_mixed_tracks_device(ntscsim_ctx *ctx, const ntscsim_cass_params *sets, int n_sets,
                                      const ntscsim_cass_mixed_track *tracks, int n_tracks, void *hip_stream);
/* The same call on HOST memory: the block pointers (any alignment) and the states are host memory, dst may equal src
 * (results are written after every source has been read; other overlaps are the caller's business).  Synchronous.  It
 * goes through pinned staging of the ctx [sources | states | results]: one copy up, ONE device call, one copy down,
 * and returns the same bytes, states and position as the device call.  Two tracks on one state: NTSCSIM_E_ARG. */
int  ntscsim_cass_mixed_tracks_host(ntscsim_ctx *ctx, const ntscsim_cass_params *sets, int n_sets,
                                    const ntscsim_cass_mixed_track *tracks, int n_tracks);
/* Drop-in for composite_audio_process(audio, samples): HOST memory, in place, any alignment.  Synchronous. */
int  ntscsim_cass_host(ntscsim_ctx *ctx, int16_t *audio, uint32_t samples);
/* reset: the tool's start.  get / set: a track processed in pieces, or started at any sample count.  set refuses a
 * state whose taps are not the bound params' (NTSCSIM_E_ARG).  All wait for the device. */
int  ntscsim_cass_reset(ntscsim_ctx *ctx);
int  ntscsim_cass_get_state(ntscsim_ctx *ctx, ntscsim_cass_state *out);
int  ntscsim_cass_set_state(ntscsim_ctx *ctx, const ntscsim_cass_state *in);
/* Debug taps.  set_plan: segment length and the two warm-ups in frames.  (0, 0, 0) restores the defaults (4096 frames;
 * 72 time constants of the high-pass for the front, 64 frames for the back); any other triple is taken as given. */
int  ntscsim_cass_debug_set_plan(ntscsim_ctx *ctx, uint32_t seg_len, uint32_t warmup_front, uint32_t warmup_back);
int  ntscsim_cass_debug_stats(ntscsim_ctx *ctx, ntscsim_cass_stats *out);
/* stats of tracks 0 .. n_tracks-1 of the last ntscsim_cass_tracks_device() or mixed tracks call (n_tracks beyond that call's:
 * NTSCSIM_E_ARG).  Waits for the device.  set_plan applies to a tracks call as it does to the single call. */
int  ntscsim_cass_debug_track_stats(ntscsim_ctx *ctx, ntscsim_cass_stats *out, int n_tracks);
/* sines the last call's host fill evaluated: a single call's frames; a tracks call's union of [count, count + frames);
 * a mixed tracks call's unions, one per distinct rate */
int  ntscsim_cass_debug_tilt_frames(ntscsim_ctx *ctx, uint64_t *evaluated);
int  ntscsim_cass_debug_time_kernels(ntscsim_ctx *ctx, int on);
/* milliseconds of the last call: [0] the host's sin fill (CPU clock), [1] its upload, [2] k_audio_hiss, [3] k_cass_front,
 * [4] k_cass_front_verify, [5] k_cass_conv, [6] k_cass_back, [7] k_cass_back_verify; after a tracks call the same
 * eight slots hold the k_cass_track_* kernel of the same name, after a mixed tracks call the k_cass_mixed_* one */
int  ntscsim_cass_debug_kernel_ms(ntscsim_ctx *ctx, float out_ms[8]);

#ifdef __cplusplus
}
#endif
#endif /* NTSCSIM_H */
