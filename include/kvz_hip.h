/*
 * kvz_hip.h -- C ABI of libkvzhip.so: Kvazaar's per-CTU block kernels as
 * hand-written HIP kernels for MI355X (gfx950), exposed
 *
 *   (1) as a "hip" strategy for Kvazaar's strategyselector plugin API
 *       (reference: src/strategyselector.h:86-87 and the per-group
 *       registration hooks kvz_strategy_register_<group>_<isa>, e.g.
 *       src/strategies/avx2/picture-avx2.c:1224-1258), and
 *   (2) as batched entry points on device-resident buffers -- the form the
 *       kernels really implement and the one that is measured.
 *
 * All paths cited below are relative to the reference's src/ directory.
 * Plain C: pointers and sizes only.  Every extern symbol is kvz_-prefixed
 * (reference rule: tests/test_external_symbols.sh:7).
 *
 * Conventions
 *   kvz_pixel = uint8_t (KVZ_BIT_DEPTH 8, kvazaar.h:72-77), coeff_t = int16_t
 *   (global.h:99).  Batched entries take DEVICE pointers and a stream; they are
 *   asynchronous (enqueue only) and return KVZ_HIP_OK or a negative error code.
 *   Strategy (per-call) entries take HOST pointers exactly like the reference's
 *   typedefs and are complete (results visible to the host) on return.
 *   There is no CPU fallback anywhere: without a usable GPU kvz_hip_init fails,
 *   the registration hooks return 0 (=> kvz_strategyselector_init fails, as for
 *   any strategy that cannot register: strategyselector.c:54-95) and the batched
 *   entries return KVZ_HIP_ERR_NO_DEVICE.
 */
#ifndef KVZ_HIP_H_
#define KVZ_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define KVZ_HIP_API __attribute__((visibility("default")))
#else
#define KVZ_HIP_API
#endif

typedef uint8_t kvz_hip_pixel;
typedef int16_t kvz_hip_coeff;
typedef void *kvz_hip_stream;        /* hipStream_t; any HIP stream of the current device is accepted.  NULL = the library's
                                      * default stream of the calling thread's current device: a BLOCKING stream, i.e. ordered
                                      * like the legacy default stream -- work enqueued with NULL starts after everything the host
                                      * queued on the legacy default stream before the call (hipMemcpy, a framework's default
                                      * stream) and is waited for by what the host queues there afterwards.  Streams made by
                                      * kvz_hip_stream_create() are non-blocking: inputs produced on another stream must be
                                      * complete (or ordered by an event, kvz_hip_stream_wait_event) before the entry is called. */

enum {
  KVZ_HIP_OK = 0,
  KVZ_HIP_ERR_NO_DEVICE = -1,       /* no gfx950 device / runtime failed to initialise */
  KVZ_HIP_ERR_INVALID = -2,         /* bad argument (size not supported, NULL pointer ...) */
  KVZ_HIP_ERR_RUNTIME = -3          /* a HIP call failed; see kvz_hip_last_error() */
};

/* ------------------------------------------------------------------ */
/* context                                                            */
/* ------------------------------------------------------------------ */
/* One context per device, all reachable from ONE process (the reference is a single process whose strategy
 * pointers are process-global, strategies/strategies-picture.c:33-64, and whose workers are pthreads,
 * threadqueue.c:263).  Every host thread has a current device, as with hipSetDevice: kvz_hip_init(device) creates
 * that device's context if needed (idempotent) and makes it the calling thread's current device; kvz_hip_set_device
 * switches the calling thread; a thread that never chose uses the process default = the first device initialised.
 * Every entry below runs on the calling thread's current device, so its pointer arguments and its stream must
 * belong to that device.  kvz_hip_init(-1): keep the thread's current device / the process default if there is one,
 * else $KVZ_HIP_DEVICE, else device 0 -- what the registration hooks call, the analogue of set_hardware_flags(),
 * strategyselector.c:452.  An index >= kvz_hip_device_count() fails with KVZ_HIP_ERR_INVALID. */
KVZ_HIP_API int kvz_hip_init(int device);
KVZ_HIP_API int kvz_hip_set_device(int device);      /* binds the calling thread; initialises the device on first use */
KVZ_HIP_API int kvz_hip_get_device(void);            /* the calling thread's current device, -1 before any kvz_hip_init */
KVZ_HIP_API void kvz_hip_shutdown(void);             /* destroys every context */
KVZ_HIP_API int kvz_hip_device_count(void);
KVZ_HIP_API const char *kvz_hip_last_error(void);    /* text of the calling thread's last failure */
KVZ_HIP_API const char *kvz_hip_device_name(void);   /* of the calling thread's current device */
/* Version of this header's ABI as the library was built (layouts of the kvz_hip_* structs, entry signatures); a host
 * compares it with the KVZ_HIP_ABI_VERSION it was compiled against before it registers the strategies. */
#define KVZ_HIP_ABI_VERSION 4   /* 2: per-device contexts, kvz_hip_me_params with tile / mv-constraint / mv-rdo fields;
                                   3: kvz_hip_me_params.cost_to_beat (96 bytes), candidate derivation and intra reference entries;
                                   4: kvz_hip_me_params.n_cabac (was reserved), the search service, kvz_hip_halo_exchange */
KVZ_HIP_API int kvz_hip_abi_version(void);

/* Launch-geometry / kernel-selection knobs for A/B runs (tools/bench_all.py --tune key=v1,v2); value < 0 restores the built-in
 * default.  Returns KVZ_HIP_OK or KVZ_HIP_ERR_INVALID (unknown key).  The environment variable KVZ_HIP_TUNE="key=value,..." presets
 * knobs at kvz_hip_init() for A/B runs of an unmodified host.  The keys, each with its default and meaning ("*_wgs_per_cu":
 * workgroups per CU of a streaming grid, 0 counts as 1; "per site": the kernels behind the key each have their own default):
 *   "sad_wgs_per_cu"           256       the SAD batch kernels
 *   "satd8_wgs_per_cu"         256       the 8x8 SATD batch kernel
 *   "dct32_wgs_per_cu"         4096      the 32x32 forward transform
 *   "idct32_wgs_per_cu"        96        the 32x32 inverse transform
 *   "dct_wgs_per_cu"           per site  the LDS butterfly transforms: 8x8 160, 16x16 48, other sizes 16
 *   "qr32_wgs_per_cu"          8         the 32x32 matrix-core tile kernel of the fused quantize_residual
 *   "qr_wgs_per_cu"            per site  the LDS butterfly kernel of quantize_residual: 8x8 64, other sizes 16
 *   "dct16_wgs_per_cu"         128       the 16x16 forward transform
 *   "idct16_wgs_per_cu"        64        the 16x16 inverse transform
 *   "qr16_wgs_per_cu"          8         the 16x16 matrix-core tile kernel of quantize_residual
 *   "qr4_lane_kernel"          1         0: the LDS butterfly kernel instead of the 4x4 lane kernel of quantize_residual
 *   "sao_edge_fast"            1         0/1: the packed-accumulator kernel of the SAO edge statistics
 *   "intra_rough_waves"        per site  4/8 waves per workgroup of the rough search: 4x4 8, other sizes 4
 *   "pair_wave_kernel"         1         0/1: one wave per descriptor for frame-level pair batches of up to 4096 descriptors
 *   "qr4_wgs_per_cu"           96        the 4x4 lane kernel of quantize_residual
 *   "quant_wgs_per_cu"         256       quant and dequant
 *   "qr8_reg_kernel"           1         0: the LDS butterfly kernel instead of the 8x8 register kernel of quantize_residual
 *   "qr8_wgs_per_cu"           per site  8x8 quantize_residual: the matrix-core tile kernel 8, the register kernel 32
 *   "qr_tile_kernel"           1         0: the LDS butterfly (8x8: the register) kernel instead of the matrix-core tile kernels
 *   "dct4_tile"                1         0: the LDS butterfly kernel for 4x4 transforms
 *   "dct4_wgs_per_cu"          192       the 4x4 forward transform
 *   "idct4_wgs_per_cu"         64        the 4x4 inverse transform
 *   "wg_chunk_min_wgs"         4096      the workgroup-per-descriptor kernels of the sampling / fractional search entries take up to 64
 *                                        descriptors per workgroup once the list would give more workgroups than this; 0: always one
 *   "pair_satd_threads"        256       128 / 256 / 512 threads per workgroup of the descriptor SATD kernel
 *   "qr8_tile_kernel"          1         0: 8x8 TUs of the fused quantize_residual on the register kernel instead of sixteen to a
 *                                        matrix-core tile
 *   "qr_tile_pipe"             1         0: the tile kernels' wait on vector memory left to the compiler instead of placed before the
 *                                        iteration's first store
 *   "pipe"                     0         1: the same hand placement in the 4x4 / 8x8 register kernels, where it measured slower
 *   "dct_pipe"                 0         1: the same hand placement in the 32x32 transform, where it measured slower
 *   "sample8_wave"             1         0: 8x8 luma blocks of the sampling entry on the general path
 *   "full_qsad"                1         0: the search service's exhaustive search prices positions with v_sad_u8 on byte-aligned
 *                                        operands instead of four alignments per v_qsad_pk_u16_u8
 *   "service_streams"          8         launch streams of the launch-per-batch way
 *   "service_inflight"         4         batches in the air of the launch-per-batch way
 *   "service_workers"          64        resident workgroups of the search service, 0: a launch per batch
 *   "service_linger_us"        2000      how long the workers stay without work
 *   "service_life_ms"          20        how long the workers stay at most
 *   "service_spin_us"          per site  how long a caller polls for its answer before it naps: 100; once set, it holds with more
 *                                        callers than cores too
 *   "service_ticket_base_k"    0         tests: first ticket of the ring x 1024
 *   "service_push"             1         0: the workers read the units from host memory even where the host could write them into
 *                                        device memory through a large BAR
 *   "service_nap_us"           10        a caller's nap with more callers than cores
 *   "service_spin_crowded_us"  5         how long a caller polls before it naps with more callers than cores
 *   "event_fence"              0         what a record of this ABI's events releases: 0 nothing, 1 to the device, 2 HIP's default (below)
 *   "event_alias"              1         0: every event record is a packet of its own (below)
 *   "cost_store_nt"            1         0: the 8x8 SAD and SATD batch kernels store their costs with the default cache policy
 *                                        instead of the nontemporal one
 * The search service reads its knobs when it is created.  How long a caller polls for its answer before it naps (the keys
 * "service_spin_us" / "service_spin_crowded_us" / "service_nap_us"): 100 us with a core per caller, 5 us and naps of 10 us with more
 * callers than cores.
 * KVZ_HIP_SERVICE_DEBUG in the environment: a few lines of the workers' own timing on stderr when a service is destroyed. */
KVZ_HIP_API int kvz_hip_set_tuning(const char *key, int value);

/* Thin device-memory helpers so a C host needs no HIP headers. */
KVZ_HIP_API void *kvz_hip_malloc(size_t bytes);
KVZ_HIP_API void kvz_hip_free(void *dptr);
/* page-locked host memory: what kvz_hip_memcpy_h2d / _d2h move without an intermediate copy (a host that feeds the
 * batched entries front by front -- descriptors up, results down -- stages them here) */
KVZ_HIP_API void *kvz_hip_malloc_host(size_t bytes);
KVZ_HIP_API void kvz_hip_free_host(void *hptr);
KVZ_HIP_API int kvz_hip_memcpy_h2d(void *dst, const void *src, size_t bytes, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_memcpy_d2h(void *dst, const void *src, size_t bytes, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_memset(void *dst, int value, size_t bytes, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_memcpy_d2d(void *dst, const void *src, size_t bytes, kvz_hip_stream s);
/* The reconstructed-pixel exchange at a shard boundary (the reference's analogue is the bounded
 * cross-row read of WPP / tiles, encoderstate.c:777-828, encoder.c:240-241) for a host that drives several devices
 * from one process: an asynchronous peer copy (xGMI) of `bytes` from src on src_device to dst on dst_device, on a
 * stream of the calling thread's current device.  Both devices must have been initialised.  A CTU-row shard sends
 * the `margin` rows at its top / bottom edge into the halo rows of the shard above / below: with stride == width
 * those rows are one contiguous range, i.e. one call per direction per plane. */
KVZ_HIP_API int kvz_hip_memcpy_peer(void *dst, int dst_device, const void *src, int src_device, size_t bytes, kvz_hip_stream s);
/* The calling thread's current device must be src_device or dst_device; peer access towards the other one is enabled on first
 * use (an error if the devices cannot reach each other); a stream that belongs to another device is refused.
 *
 * One shard's whole exchange step in one call: the C form of kvazaar_amd/shard.py exchange_halo_into for a host whose shards
 * live on several devices of ONE process.  A shard's plane is an EXTENDED buffer: `rows` own rows starting at row `top`, the
 * neighbour's rows (the halo, `margin` of them) above and below.  The calling thread's shard PUSHES the first `margin` of its own
 * rows into the halo below the own rows of `up`, and its last `margin` own rows into the halo above the own rows of `down`
 * (either may be NULL: the frame's edge).  Asynchronous on stream s of self->device; the receiving shard orders its search
 * behind it with kvz_hip_event_record on that stream + kvz_hip_stream_wait_event on its own. */
typedef struct {
  void *ext;                    /* the shard's extended plane on `device`: (top + rows + halo below) rows of `stride` bytes */
  int32_t device;
  int32_t top, rows;            /* where the own rows start, and how many there are */
} kvz_hip_shard_plane;
KVZ_HIP_API int kvz_hip_halo_exchange(const kvz_hip_shard_plane *self, const kvz_hip_shard_plane *up, const kvz_hip_shard_plane *down,
                                      uint32_t stride, int margin, kvz_hip_stream s);
/* A batch of 2-D byte rectangles copied by ONE kernel launch on stream s of the calling thread's current device: rect i copies h rows
 * of w bytes from src (rows src_stride bytes apart) to dst (rows dst_stride bytes apart).  The rects travel as a kernel argument (no
 * upload), so n is at most KVZ_HIP_MAX_RECTS.  The pointers may be device memory of the current device or of a peer device whose
 * access is enabled (kvz_hip_tile_halo_exchange / kvz_hip_memcpy_peer enable it); any alignment and width is accepted, 16-byte
 * accesses are used where both pointers and both strides are multiples of 16.  A rect with w == 0 or h == 0 is skipped.  Sources and
 * destinations must not overlap.  KVZ_HIP_ERR_INVALID: n outside 0..KVZ_HIP_MAX_RECTS, rects NULL with n > 0, a negative w / h, a
 * NULL pointer or a stride < w in a non-empty rect (with h > 1), a batch of 2^31 or more 16-byte chunks, a stream of another device.
 * Uses: packing halo strips into contiguous staging, unpacking them into an extended buffer, copying a tile's own rectangle into
 * its extended buffer (a strided copy kvz_hip_memcpy_d2d cannot do). */
#define KVZ_HIP_MAX_RECTS 16
typedef struct {
  const void *src;
  void *dst;
  uint32_t src_stride, dst_stride;    /* bytes */
  int32_t w, h;                       /* bytes per row, rows */
} kvz_hip_rect_copy;                  /* 32 bytes */
KVZ_HIP_API int kvz_hip_copy_rects_batch(const kvz_hip_rect_copy *rects, int n, kvz_hip_stream s);
/* The exchange step of a frame cut into TILES in both directions (kvazaar_amd/shard.py TileShard / exchange_tile_halo_into) for a host
 * that drives its tiles from one process.  A tile's plane is an EXTENDED buffer on `device`: the rectangle (ext_x, ext_y, ext_w, ext_h)
 * of the frame, rows `stride` bytes apart; the tile's own rectangle (own_x, own_y, own_w, own_h), also in frame coordinates, lies
 * inside it.  The calling thread's tile PUSHES, for every neighbour, the pixels of the intersection of self.own and neighbour.ext to the same frame position
 * in the neighbour's buffer: up to 8 neighbours (left, right, above, below and the four corners), all regions in ONE launch of the
 * kvz_hip_copy_rects_batch kernel on stream s of self->device; a neighbour on another device is written through peer access (enabled
 * on first use).  A full-width row shard is the special case ext_x = own_x = 0, ext_w = own_w = width: the same bytes as
 * kvz_hip_halo_exchange.  KVZ_HIP_ERR_INVALID: the calling thread does not work on self->device, n outside 0..8, neighbours NULL with
 * n > 0, a NULL buffer, a stride < ext_w, an own rectangle outside its extended rectangle, own rectangles (self's and the neighbours')
 * that overlap, a device that was not initialised, a stream of another device. */
typedef struct {
  void *ext;                          /* the tile's extended plane on `device` */
  int32_t device;
  uint32_t stride;                    /* bytes between rows of ext (>= ext_w) */
  int32_t ext_x, ext_y, ext_w, ext_h; /* the extended rectangle, frame coordinates */
  int32_t own_x, own_y, own_w, own_h; /* the own rectangle, frame coordinates, inside the extended one */
} kvz_hip_tile_plane;                 /* 48 bytes */
KVZ_HIP_API int kvz_hip_tile_halo_exchange(const kvz_hip_tile_plane *self, const kvz_hip_tile_plane *neighbours, int n, kvz_hip_stream s);
KVZ_HIP_API kvz_hip_stream kvz_hip_stream_create(void);
KVZ_HIP_API void kvz_hip_stream_destroy(kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_stream_sync(kvz_hip_stream s);
/* HIP-event timing of the enqueued work on stream s (used by bench.py for the
 * roofline: the event pair brackets exactly the launches issued in between).
 * What an event is for: it ORDERS and TIMES device work on ONE device.  Work enqueued behind kvz_hip_stream_wait_event on
 * any stream of the same device sees everything the recording stream wrote before the record; kvz_hip_event_elapsed_ms
 * returns the device time between two records.  An event does NOT publish memory: results reach the host through
 * kvz_hip_stream_sync (and kvz_hip_memcpy_d2h, which synchronises), and a peer device through the exchange entries
 * (kvz_hip_memcpy_peer, kvz_hip_halo_exchange, kvz_hip_tile_halo_exchange), which end with a fenced record of their own
 * on their stream: an event recorded behind one of them orders a receiving device's work behind pixels it can see.  Any
 * other write to a peer's memory (kvz_hip_copy_rects_batch with peer pointers) is published by kvz_hip_stream_sync.
 * Nothing else does.  The events are therefore created without HIP's system-scope fence, which would write back
 * and invalidate the device's caches at every record (tuning key "event_fence", read by kvz_hip_event_create: 0 = no
 * system fence, the default; 1 = release to the device; 2 = HIP's default event).
 * The handle is opaque (it is not a hipEvent_t).
 * A RECORD THAT DIRECTLY FOLLOWS A BATCH LAUNCH MARKS THAT LAUNCH'S COMPLETION.  When kvz_hip_event_record is the next operation
 * of this ABI on the stream after kvz_hip_sad_nxn_batch, kvz_hip_satd_nxn_batch, their _dual_ forms or kvz_hip_transform_batch
 * (DCT / IDCT / DST / IDST), and the caller had recorded an event just before that entry as well, the record enqueues nothing:
 * the event stands for the end of that kernel, which the kernel's own dispatch reports.  It orders (kvz_hip_stream_wait_event)
 * and times (kvz_hip_event_elapsed_ms) exactly as a record behind the kernel does, and like every event of this ABI it has
 * never published memory.  Records with nothing in between share that instant: the time between them is 0.  Every other
 * record -- behind any other entry, behind a copy, a memset, a wait, a graph launch, inside a capture, or with no record in
 * front of the launch -- is a record of its own, as before.
 * ONE CAVEAT: the library sees only what goes through this ABI.  A stream from kvz_hip_stream_create, or a hipStream_t of the
 * caller's, can also take work by other means -- a framework that was handed the stream, plain HIP calls.  (NULL is the
 * library's own stream of the device, which nobody else holds; work on HIP's legacy default stream is ordered against it by
 * HIP but never enqueued on it.)  Work placed that way BETWEEN one of the launches above and the record behind it is not
 * covered by the event.  Such a caller puts any operation of this ABI in between or switches the behaviour off: tuning key
 * "event_alias", 1 = on (the default), 0 = every record is a packet of its own.
 * THREADS: a record rides only on a launch of the calling thread.  Threads that share a stream (NULL is one per device) get
 * records of their own for each other's launches, so each thread's record still covers the work it enqueued before it. */
KVZ_HIP_API void *kvz_hip_event_create(void);
KVZ_HIP_API void kvz_hip_event_destroy(void *ev);
KVZ_HIP_API int kvz_hip_event_record(void *ev, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_event_elapsed_ms(void *start, void *stop, float *ms);  /* syncs on stop */

/* A frame's launch sequence as one hipGraph (the encoder issues the same batched entries, on
 * the same buffers, for every frame: encoderstate.c:1330-1400 walks the same LCU grid per frame).
 * Every batched entry above and below is capture-safe: it only enqueues kernels on `s`.
 *   kvz_hip_graph_begin(s);  ...batched entries on s (and on streams forked from it with
 *   kvz_hip_event_record + kvz_hip_stream_wait_event, joined back the same way)...
 *   kvz_hip_graph_end(s, &g);  then per frame: kvz_hip_graph_launch(g, s).
 * Independent stages (motion search, intra search, SAO statistics) put on forked streams become
 * parallel branches of the graph and share the 256 CUs when one stage alone cannot fill them. */
typedef void *kvz_hip_graph;         /* an instantiated graph (hipGraphExec_t) */
KVZ_HIP_API int kvz_hip_stream_wait_event(kvz_hip_stream s, void *ev);
KVZ_HIP_API int kvz_hip_graph_begin(kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_graph_end(kvz_hip_stream s, kvz_hip_graph *graph_out);
KVZ_HIP_API int kvz_hip_graph_launch(kvz_hip_graph graph, kvz_hip_stream s);
KVZ_HIP_API void kvz_hip_graph_destroy(kvz_hip_graph graph);

/* ------------------------------------------------------------------ */
/* (2) batched entries -- picture group                               */
/*     reference typedefs: strategies/strategies-picture.h:102-130    */
/* ------------------------------------------------------------------ */

/* cost_pixel_nxn_func over `count` contiguous N*N block pairs:
 * costs[i] = sad_NxN(blk1 + i*N*N, blk2 + i*N*N); N in {4,8,16,32,64}.
 * Replaces sad_4x4..sad_64x64 (generic/picture-generic.c:460-486). */
KVZ_HIP_API int kvz_hip_sad_nxn_batch(int n, const kvz_hip_pixel *blk1, const kvz_hip_pixel *blk2,
                                      size_t count, uint32_t *costs, kvz_hip_stream s);
/* satd_4x4..satd_64x64 (picture-generic.c:189-196, strategies-picture.h:40-56) */
KVZ_HIP_API int kvz_hip_satd_nxn_batch(int n, const kvz_hip_pixel *blk1, const kvz_hip_pixel *blk2,
                                       size_t count, uint32_t *costs, kvz_hip_stream s);

/* cost_pixel_nxn_multi_func (sad_NxN_dual / satd_NxN_dual, picture-generic.c:357-390,
 * :497-519): item i has two predictions at preds + i*item_stride + {0, pred_stride}
 * (pred_stride = 1024 for the reference's pred_buffer, strategies-picture.h:34) and
 * one original block at orig + i*N*N; costs[2*i + k]. */
KVZ_HIP_API int kvz_hip_sad_nxn_dual_batch(int n, const kvz_hip_pixel *preds, size_t pred_stride, size_t item_stride,
                                           const kvz_hip_pixel *orig, size_t count, uint32_t *costs, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_satd_nxn_dual_batch(int n, const kvz_hip_pixel *preds, size_t pred_stride, size_t item_stride,
                                            const kvz_hip_pixel *orig, size_t count, uint32_t *costs, kvz_hip_stream s);

/* PLANES.  Every entry that takes a picture plane takes it as a pointer, a row stride in bytes and (where it clamps) a
 * width and a height: a rectangle inside any larger device buffer, e.g. the extended buffer of a shard.  Unless an entry
 * says otherwise below
 *   - the pointer may have ANY alignment (an odd address included) and the stride may be ANY value >= the width, odd
 *     ones included: pixels are fetched with byte-addressed vector loads, never with loads that need an aligned address;
 *   - every plane of a call has its own stride (pic / ref, ref0 / ref1, rec / new_rec, luma / chroma are independent);
 *   - nothing left of the pointer, right of the width (the bytes between width and stride), above the first or below
 *     the last row is read or written.
 * The exceptions document their rule at the entry and refuse what breaks it with KVZ_HIP_ERR_INVALID:
 * kvz_hip_deblock_frame, the CU-map entries built like it and the whole-picture SAO entries kvz_hip_sao_stats_frame /
 * kvz_hip_sao_frame (4-byte aligned planes and strides).  kvz_hip_inter_residual_frame and kvz_hip_intra_recon_frame take
 * the general rule.  The search service
 * owns its planes (width a multiple of 4, PU x a multiple of 4) and is not concerned.
 * tests/test_gpu_plane_layout.py holds each of these entries to this on padded, offset and odd layouts. */

/* One block pair inside two planes; the unit of the frame-level entries below. */
typedef struct {
  int32_t x1, y1;          /* top-left of the block in plane 1 (the picture being coded) */
  int32_t x2, y2;          /* top-left of the block in plane 2 (the reference picture)   */
  int32_t width, height;
} kvz_hip_block_pair;

/* reg_sad_func (picture-generic.c:86-99) over a list of block pairs that lie
 * INSIDE their planes: costs[i] = reg_sad(p1 + y1*stride1 + x1, p2 + y2*stride2 + x2, w, h, ..).
 * Any width/height >= 1 (tests/sad_tests.c:369-376 shapes, 64x63, 1x1).
 * Planes: any base alignment, any strides >= the widths in use, stride1 and stride2 independent (PLANES above); the
 * same holds for the three entries that follow. */
KVZ_HIP_API int kvz_hip_reg_sad_batch(const kvz_hip_pixel *plane1, uint32_t stride1,
                                      const kvz_hip_pixel *plane2, uint32_t stride2,
                                      const kvz_hip_block_pair *pairs, size_t count,
                                      uint32_t *costs, kvz_hip_stream s);
/* kvz_image_calc_sad (image.c:455-486): plane 2 coordinates may be outside the
 * w2 x h2 reference frame; outside pixels are edge replicated, which is what
 * image_interpolated_sad (image.c:320-444) computes. */
KVZ_HIP_API int kvz_hip_image_calc_sad_batch(const kvz_hip_pixel *pic, uint32_t pic_stride,
                                             const kvz_hip_pixel *ref, uint32_t ref_stride, int ref_w, int ref_h,
                                             const kvz_hip_block_pair *pairs, size_t count,
                                             uint32_t *costs, kvz_hip_stream s);
/* cost_pixel_any_size_func (strategies-picture.h:62-100) / kvz_image_calc_satd
 * (image.c:488-545): width and height multiples of 4; edge replication as above. */
KVZ_HIP_API int kvz_hip_image_calc_satd_batch(const kvz_hip_pixel *pic, uint32_t pic_stride,
                                              const kvz_hip_pixel *ref, uint32_t ref_stride, int ref_w, int ref_h,
                                              const kvz_hip_block_pair *pairs, size_t count,
                                              uint32_t *costs, kvz_hip_stream s);
/* pixels_calc_ssd_func (picture-generic.c:521-536): square blocks, width = pairs[i].width */
KVZ_HIP_API int kvz_hip_pixels_calc_ssd_batch(const kvz_hip_pixel *plane1, uint32_t stride1,
                                              const kvz_hip_pixel *plane2, uint32_t stride2,
                                              const kvz_hip_block_pair *pairs, size_t count,
                                              uint32_t *ssd, kvz_hip_stream s);
/* cost_pixel_any_size_multi_func (satd_any_size_quad, picture-generic.c:392-456),
 * including its behaviour for widths/heights that are not multiples of 8:
 * item i compares 4 candidate blocks preds + (4*i + k)*pred_item_stride
 * (row stride pred_stride, 64 in search_inter.c:1076) with the block at
 * (x1,y1) of `orig`; costs[4*i + k].  orig: any base alignment and stride; preds: any pred_stride >= the width and
 * any pred_item_stride >= height * pred_stride, the bytes in the gaps are not read. */
KVZ_HIP_API int kvz_hip_satd_any_size_quad_batch(const kvz_hip_pixel *preds, uint32_t pred_stride, size_t pred_item_stride,
                                                 const kvz_hip_pixel *orig, uint32_t orig_stride,
                                                 const kvz_hip_block_pair *pairs, size_t count,
                                                 uint32_t *costs, kvz_hip_stream s);
/* Batched integer motion-estimation costs, one CTU per workgroup: what check_mv_cost
 * (search_inter.c:195-232) computes one candidate at a time through
 * kvz_image_calc_sad (image.c:455-486), for every candidate of a pattern and every
 * square PU size of the CTU in one launch.  For CTU i (64x64 at (x, y) in `pic`),
 * search centre (mvx, mvy) in full pels, and candidate m = centre + mv_offsets[m]:
 *   costs[(i*n_mv + m)*85 + k] = kvz_image_calc_sad(pic, ref, bx, by, bx + mv, by + mv, bw, bw)
 * with k = 0: the 64x64 PU; 1..4: the 32x32 PUs, 5..20: 16x16, 21..84: 8x8, each
 * group in raster order inside the CTU.  The reference block may leave the frame
 * (edge replicated).  PUs not entirely inside `pic` (ragged last CTU row/column)
 * get 0xFFFFFFFF.  The CTU's source block and its search window are fetched from
 * HBM once and stay in LDS; larger PUs are sums of the 8x8 SADs.
 * |mv_offsets| <= 64 in each component.
 * pic and ref: any base alignment, any stride >= the width, independent of each other; the window is clamped against
 * ref_w / ref_h, never against the stride. */
typedef struct {
  int32_t x, y;            /* CTU top-left in the picture (multiples of 8) */
  int32_t mvx, mvy;        /* search centre, full-pel */
} kvz_hip_ctu_search;
#define KVZ_HIP_CTU_PUS 85
KVZ_HIP_API int kvz_hip_ctu_sad_grid_batch(const kvz_hip_pixel *pic, uint32_t pic_stride, int pic_w, int pic_h,
                                           const kvz_hip_pixel *ref, uint32_t ref_stride, int ref_w, int ref_h,
                                           const kvz_hip_ctu_search *ctus, size_t count,
                                           const int16_t *mv_offsets /* device, [n_mv][2] = (dx, dy) */, int n_mv,
                                           uint32_t *costs /* [count][n_mv][85] */, kvz_hip_stream s);

/* inter_recon_bipred_func's blend (picture-generic.c:538-588) for `count` planes
 * of w x h samples laid out contiguously (stride w): each source is either 14-bit
 * int16 samples (hi_prec != 0) or pixels. */
KVZ_HIP_API int kvz_hip_bipred_blend_batch(int w, int h, int hi_prec0, const void *src0, int hi_prec1, const void *src1,
                                           kvz_hip_pixel *dst, size_t count, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* (2) batched entries -- dct group (strategies/strategies-dct.h:31)   */
/* ------------------------------------------------------------------ */
enum { KVZ_HIP_DCT = 0, KVZ_HIP_IDCT = 1, KVZ_HIP_DST = 2, KVZ_HIP_IDST = 3, KVZ_HIP_TRSKIP = 4, KVZ_HIP_ITRSKIP = 5 };
/* dct_func over `count` contiguous N*N int16 blocks (generic/dct-generic.c:567-617).
 * kind DCT/IDCT: n in {4,8,16,32}; DST/IDST: n == 4 (fast_forward_dst_4x4 / inverse);
 * TRSKIP/ITRSKIP: kvz_transformskip / kvz_itransformskip (transform.c:150-180), n in {4,8,16,32}. */
KVZ_HIP_API int kvz_hip_transform_batch(int kind, int n, const int16_t *in, int16_t *out,
                                        size_t count, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* (2) batched entries -- quant group (strategies/strategies-quant.h)  */
/* ------------------------------------------------------------------ */
/* The encoder state the reference's quant functions read, flattened
 * (generic/quant-generic.c:40-50, :283-289). */
typedef struct {
  int32_t qp;               /* state->qp */
  int32_t slice_is_intra;   /* state->frame->slicetype == KVZ_SLICE_I */
  int32_t signhide;         /* encoder->cfg.signhide_enable */
  int32_t scaling_list;     /* encoder->scaling_list.enable; 0 = flat list */
  const int32_t *quant_coeff;    /* DEVICE (batched) / HOST (per-call) [w*h] factors when scaling_list */
  const int32_t *dequant_coeff;  /* likewise */
} kvz_hip_quant_params;

/* quant_func (quant-generic.c:37-163) over `count` w*w blocks.
 * type: 0 luma, 2/3 chroma; scan_idx 0 diag / 1 hor / 2 ver. */
KVZ_HIP_API int kvz_hip_quant_batch(const kvz_hip_quant_params *p, const kvz_hip_coeff *coef, kvz_hip_coeff *q_coef,
                                    int width, int type, int scan_idx, size_t count, kvz_hip_stream s);
/* dequant_func (quant-generic.c:279-321) */
KVZ_HIP_API int kvz_hip_dequant_batch(const kvz_hip_quant_params *p, const kvz_hip_coeff *q_coef, kvz_hip_coeff *coef,
                                      int width, int type, size_t count, kvz_hip_stream s);
/* coeff_abs_sum_func (quant-generic.c:323-330) per block of `length` coeffs */
KVZ_HIP_API int kvz_hip_coeff_abs_sum_batch(const kvz_hip_coeff *coeffs, size_t length, size_t count,
                                            uint32_t *sums, kvz_hip_stream s);
/* quant_residual_func, the rdoq-off path of kvz_quantize_residual_generic
 * (quant-generic.c:180-273): residual -> transform -> quant -> dequant ->
 * inverse -> reconstruction, one fused kernel per TU.  Blocks are contiguous
 * (stride = width).  rec_out may alias pred_in.  has_coeffs[i] receives the
 * function's return value.  color 0 Y / 1 U / 2 V. */
KVZ_HIP_API int kvz_hip_quantize_residual_batch(const kvz_hip_quant_params *p, int cu_is_intra, int width, int color,
                                                int scan_order, int use_trskip,
                                                const kvz_hip_pixel *ref_in, const kvz_hip_pixel *pred_in,
                                                kvz_hip_pixel *rec_out, kvz_hip_coeff *coeff_out, int32_t *has_coeffs,
                                                size_t count, kvz_hip_stream s);
/* The two elementwise ends of kvz_quantize_residual as separate entries (quant-generic.c:196-204 and :253-259), for
 * callers that run something of their own between transform and dequantisation (the drop-in does, when RDOQ is on):
 * residual[i] = ref[i] - pred[i];  rec[i] = clip((int16)(residual[i] + pred[i])).  n = number of pixels. */
KVZ_HIP_API int kvz_hip_residual_batch(const kvz_hip_pixel *ref_in, const kvz_hip_pixel *pred_in, kvz_hip_coeff *residual,
                                       size_t n, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_reconstruct_batch(const kvz_hip_coeff *residual, const kvz_hip_pixel *pred_in, kvz_hip_pixel *rec_out,
                                          size_t n, kvz_hip_stream s);
/* The same fused kernel with the two numbers the rd=0 TU cost is made of
 * (kvz_cu_rd_cost_luma / _chroma, search.c:236-306, :309-383): ssd_out[i] =
 * kvz_pixels_calc_ssd(ref_i, rec_i, width) (picture-generic.c:521-536) and
 * coeff_abs_sum_out[i] = kvz_coeff_abs_sum(coeff_i, width*width) (rdo.c:219,
 * quant-generic.c:323-330), taken from the registers / LDS the reconstruction
 * and coefficients are in -- neither array is read back from HBM.
 * SURVEY.md section 8(f) row 3. */
KVZ_HIP_API int kvz_hip_quantize_residual_cost_batch(const kvz_hip_quant_params *p, int cu_is_intra, int width, int color,
                                                     int scan_order, int use_trskip,
                                                     const kvz_hip_pixel *ref_in, const kvz_hip_pixel *pred_in,
                                                     kvz_hip_pixel *rec_out, kvz_hip_coeff *coeff_out, int32_t *has_coeffs,
                                                     uint32_t *ssd_out, uint32_t *coeff_abs_sum_out,
                                                     size_t count, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* (2) batched entries -- ipol group (strategies/strategies-ipol.h)    */
/* ------------------------------------------------------------------ */
typedef struct {
  int32_t x, y;            /* integer-pel top-left of the block in the reference plane (may be outside) */
  int32_t mv_frac_x, mv_frac_y;   /* mv & 3 (luma) / mv & 7 (chroma) */
  int32_t width, height;
} kvz_hip_ipol_block;

/* kvz_sample_quarterpel_luma / kvz_sample_octpel_chroma and their 14-bit
 * variants (generic/ipol-generic.c:122-190, :660-728), with the source window
 * fetched like kvz_get_extended_block (ipol-generic.c:731-784: coordinates
 * clamped to the plane; ref_stride may exceed ref_w, and nothing right of
 * ref_w or below ref_h is read).  Output block i is written contiguously
 * (stride = width) at dst + out_offsets[i] (elements); the offsets may come in
 * any order and at any alignment, and nothing outside the w*h elements of each
 * block is written.  Supported shapes: 1..64 (luma) / 1..32 (chroma) on each
 * side.  A descriptor of any other shape (a side of 0 or less, or too large)
 * is skipped: nothing is written for it. */
KVZ_HIP_API int kvz_hip_sample_luma_batch(const kvz_hip_pixel *ref, uint32_t ref_stride, int ref_w, int ref_h,
                                          const kvz_hip_ipol_block *blocks, const uint64_t *out_offsets, size_t count,
                                          int out_14bit, void *dst, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_sample_chroma_batch(const kvz_hip_pixel *ref, uint32_t ref_stride, int ref_w, int ref_h,
                                            const kvz_hip_ipol_block *blocks, const uint64_t *out_offsets, size_t count,
                                            int out_14bit, void *dst, kvz_hip_stream s);

/* Fractional motion search of search_frac (search_inter.c:965-1128): for block
 * pair i (x1,y1 in pic; x2,y2 = integer-pel position in ref; w,h multiples of
 * 4 up to 64, not both 4 mod 8 -- for the SMP / AMP shapes the integer position
 * is scored by satd_any_size and the candidates by satd_any_size_quad, whose
 * 4x4 stages add nothing, exactly as the reference does) the four filter steps (filter_hpel/qpel_blocks_*_luma,
 * ipol-generic.c:192-658) fused with satd_any_size(_quad); filtered candidates
 * stay in LDS, only costs leave the CU.  costs[17*i + 0] integer position,
 * [1..8] half-pel neighbours, [9..16] quarter-pel neighbours of the best
 * half-pel position; best[2*i + {0,1}] = chosen hpel / qpel index (0 = centre),
 * ties and order as in the reference, MV bit costs taken as zero.  A
 * descriptor of any other shape (4x4, 12x12, a side that is not a multiple of
 * 4, 0 or less, or larger than 64) is flagged: its 17 costs are 0xFFFFFFFF and
 * best[2*i + {0,1}] = -1; its neighbours are computed as usual. */
KVZ_HIP_API int kvz_hip_search_frac_batch(const kvz_hip_pixel *pic, uint32_t pic_stride,
                                          const kvz_hip_pixel *ref, uint32_t ref_stride, int ref_w, int ref_h,
                                          const kvz_hip_block_pair *pairs, size_t count,
                                          uint32_t *costs, int32_t *best, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* (2) batched entries -- motion search of whole PUs                   */
/*     SURVEY.md section 8(f) row 1                                    */
/* ------------------------------------------------------------------ */
/* One merge candidate as calc_mvd_cost / select_starting_point see it
 * (inter_merge_cand_t, inter.h): */
typedef struct {
  int16_t mv[2];       /* merge_cand[i].mv[dir - 1], quarter-pel */
  uint8_t usable;      /* merge_cand[i].dir != 3 */
  uint8_t same_ref;    /* state->frame->ref_LX[dir - 1][merge_cand[i].ref[dir - 1]] == ref_idx */
} kvz_hip_me_merge;
/* inter_search_info_t (search_inter.c:40-76) of one PU for one reference picture */
typedef struct {
  int32_t x, y, width, height;   /* PU inside the picture; width, height multiples of 4 in 4..64, not both 4 mod 8:
                                  * every shape of the inter search incl. the SMP / AMP ones (8x4, 4x8, 16x4, 4x16, 16x12, 12x16) */
  int16_t mv_cand[2][2];         /* AMVP candidates (kvz_inter_get_mv_cand), quarter-pel */
  int16_t extra_mv[2];           /* start vector from the co-located CU (search_inter.c:1190-1206), quarter-pel */
  int16_t num_merge_cand;        /* 0..5 */
  int16_t reserved;              /* mv_rdo: index of this PU's snapshot in kvz_hip_me_params.cabac */
  kvz_hip_me_merge merge[5];
  int16_t pad;                   /* bits 0-1: merge neighbours barred (kvz_hip_inter_candidates_batch); bits 2..: plane pair
                                    (kvz_hip_search_pu_multi_batch); ignored by kvz_hip_search_pu_batch */
} kvz_hip_me_pu;                 /* 64 bytes */
/* The CABAC state kvz_calc_mvd_cost_cabac (rdo.c:908-1060, --mv-rdo) starts from: what it reads of state->cabac
 * (cabac_data_t, cabac.h:41-88).  The encoder's contexts change from LCU to LCU; a batch carries one snapshot per
 * distinct state and every PU names its own (kvz_hip_me_pu.reserved). */
typedef struct {
  uint16_t range;                /* cabac.range */
  uint8_t ctx[8];                /* uc_state of ctx.cu_merge_flag_ext_model, cu_merge_idx_ext_model, cu_ref_pic_model[0], [1],
                                    cu_mvd_model[0], [1], mvp_idx_model[0]; [7] unused */
  uint8_t pad[6];
} kvz_hip_me_cabac;              /* 16 bytes */
/* the encoder settings the search reads */
typedef struct {
  int32_t lambda_cost;           /* (int32_t)(state->lambda_sqrt + 0.5), search_inter.c:411 */
  int32_t early_termination;     /* cfg.me_early_termination: 0 off, 1 on, 2 sensitive */
  uint32_t max_steps;            /* cfg.me_max_steps */
  int32_t fme_level;             /* cfg.fme_level, 0..4 */
  int32_t wpp_owf;               /* cfg.owf && cfg.wpp: enforce the reference-availability rule of fracmv_within_tile */
  int32_t ref_delay_px;          /* SAO_DELAY_PX (sao on), DEBLOCK_DELAY_PX (deblock only) or 0 (global.h:163,175) */
  int32_t max_ref_lcu_down, max_ref_lcu_right;   /* ctrl->max_inter_ref_lcu (encoder.c:240-241) */
  int32_t algorithm;             /* cfg.ime_algorithm: 0 hexbs (hexagon_search), 1 dia (diamond_search, :796-883), 2 tz (tz_search, :595-672),
                                    3 full (search_mv_full, :886-962; no early termination) */
  int32_t search_range;          /* algorithm 3 only: 8, 16, 32 or 64 (search_inter.c:1208-1215), any value 1..64 accepted */
  int32_t size_classes;          /* optional hint, 0 = unknown: OR of 1 (PUs up to 16x16), 2 (up to 32x32), 4 (larger) present in the
                                    batch; the entry runs one kernel per size class and skips the launches for absent ones */
  int32_t mv_constraint;         /* cfg.mv_constraint (enum kvz_mv_constraint, kvazaar.h:113-119): 0 none, 1 frame, 2 tile, 3 frame and tile,
                                    4 frame and tile with the interpolation margin -- the five branches of fracmv_within_tile
                                    (search_inter.c:142-171; the reference treats 1..3 alike) */
  int32_t tile_x, tile_y;        /* state->tile->offset_x / offset_y: top-left of the tile in the picture (multiples of 64 in the reference;
                                    required here only with wpp_owf, whose rule counts LCUs from the tile origin) */
  int32_t tile_w, tile_h;        /* state->tile->frame->width / height; 0 x 0 = the whole picture is one tile.  PU coordinates stay
                                    picture coordinates; the entry derives the tile-relative info->origin the reference tests.
                                    A CTU-row shard of a frame is a tile of full width: with mv_constraint 3 or 4 its
                                    search reads nothing outside its own rows (+ nothing at all beyond them), with wpp_owf and
                                    max_ref_lcu_down = 1 nothing beyond one CTU row + ref_delay_px + 4 rows below them. */
  int32_t mv_rdo;                /* cfg.mv_rdo: MV bit costs from the CABAC model (kvz_calc_mvd_cost_cabac, rdo.c:908-1060, and
                                    kvz_get_mvd_coding_cost_cabac in select_mv_cand) instead of the exp-Golomb estimate */
  int32_t ref_idx;               /* mv_rdo: info->ref_idx of the reference picture searched */
  int32_t refs_before;           /* mv_rdo: pictures of state->frame->ref with poc < current poc (rdo.c:990-998); ref_idx is coded when > 1 */
  int32_t n_cabac;               /* mv_rdo: number of snapshots in cabac (>= 1); a PU whose kvz_hip_me_pu.reserved is not an index into it is
                                    flagged (cost 0xFFFFFFFF, reserved -1) instead of searched.  Else unused (0) */
  const kvz_hip_me_cabac *cabac; /* mv_rdo: DEVICE array of n_cabac snapshots, indexed by kvz_hip_me_pu.reserved; else unused (NULL) */
  const uint32_t *cost_to_beat;  /* NULL, or a DEVICE array with one entry per PU: *inter_cost as search_pu_inter_ref finds it
                                    (search_inter.c:1239), i.e. the best cost of the reference pictures searched before this one
                                    (MAX_INT for the first).  A PU whose integer search does not get below it skips the fractional
                                    search and is scored like fme_level 0 (:1242-1252), exactly as the reference's loop over
                                    the pictures of a multi-reference frame does */
} kvz_hip_me_params;             /* 96 bytes */
typedef struct {
  int32_t mv[2];                 /* info->best_mv, quarter-pel */
  uint32_t cost, bitcost;        /* info->best_cost, info->best_bitcost; cost 0xFFFFFFFF: nothing allowed / bad descriptor */
  int32_t merged, merge_idx;     /* the match loop of search_inter.c:1253-1266 */
  int32_t mv_cand;               /* select_mv_cand (search_inter.c:1268-1273) */
  int32_t reserved;              /* -1 flags a malformed descriptor */
} kvz_hip_me_result;

/* The --me hexbs / dia / tz / full paths of search_pu_inter_ref (search_inter.c:1134-1300) for
 * `count` PUs against one reference plane in one launch: hexagon_search
 * diamond_search or tz_search (:463-883, with select_starting_point and early_terminate) over
 * kvz_image_calc_sad + calc_mvd_cost, then search_frac (:965-1128) -- or, for
 * fme_level 0, the SATD re-cost of :1236-1248.  Same visiting order and
 * tie-breaks as the reference, so results[i] equals what the reference leaves
 * in inter_search_info_t.  pus / results are device arrays.
 * pic and ref: any base alignment, any stride >= the width (odd ones included), independent of each other, for every
 * algorithm, with mv_rdo and with a tile -- the exhaustive search (algorithm 3) included: its kernels here stage the
 * current block in LDS with byte-addressed loads.  (Only the search service prices the block from scalar dword loads;
 * it owns its planes and keeps them 4-byte aligned itself.) */
KVZ_HIP_API int kvz_hip_search_pu_batch(const kvz_hip_pixel *pic, uint32_t pic_stride, int pic_w, int pic_h,
                                        const kvz_hip_pixel *ref, uint32_t ref_stride, int ref_w, int ref_h,
                                        const kvz_hip_me_pu *pus, size_t count, const kvz_hip_me_params *params,
                                        kvz_hip_me_result *results, kvz_hip_stream s);
/* The same search over SEVERAL pictures of one size in one launch: pics / refs are DEVICE arrays of n_planes plane pointers
 * (all planes share the strides and sizes given), and a PU names its pair in kvz_hip_me_pu.pad >> 2 (bits 0 and 1 keep
 * their meaning for kvz_hip_inter_candidates_batch).  This is how work that is independent by construction -- the same
 * dependency front of several frames in flight (--owf), of several tiles, of several encoder instances -- shares a launch:
 * a front of a dozen PUs leaves the chip idle, and host threads stop scaling at the runtime's launch rate, but fronts of
 * many pictures merged into one launch cost what one does.  A plane index outside 0 .. n_planes - 1 flags the PU
 * (reserved -1).  mv_rdo is not available here.  The planes of one table share a stride and a size but each may start
 * at any address of its own buffer: any base alignment, any stride >= the width, pic_stride and ref_stride independent. */
KVZ_HIP_API int kvz_hip_search_pu_multi_batch(const kvz_hip_pixel *const *pics, uint32_t pic_stride, int pic_w, int pic_h,
                                              const kvz_hip_pixel *const *refs, uint32_t ref_stride, int ref_w, int ref_h, int n_planes,
                                              const kvz_hip_me_pu *pus, size_t count, const kvz_hip_me_params *params,
                                              kvz_hip_me_result *results, kvz_hip_stream s);

/* ---- search service: the searches of MANY host threads, without a launch per search ---- */
/* The reference runs one CTU job per threadqueue worker (encoderstate.c:777-828: WPP rows, frames in flight under
 * --owf, tiles), and every worker reaches search_pu_inter (search_inter.c:1451-1520) with ONE PU at a time.  A launch per
 * PU and per reference picture leaves the chip idle and pays the launch price every time; the service is the piece
 * between those workers and the kernels of kvz_hip_search_pu_batch:
 *   - the luma planes the searches read (source pictures, reconstructed pictures) stay resident on the device in
 *     numbered slots, written rectangle by rectangle as the host produces them;
 *   - kvz_hip_me_service_search() is called concurrently by the workers, each with one PU and ALL the reference pictures
 *     of search_pu_inter's loop (:1502-1507).  By default the (PU, picture) units go into a ring in page-locked memory and are
 *     taken by workgroups that stay on the device ("resident workers": started when a request finds none, gone when the
 *     service has been idle for a couple of milliseconds; tuning "service_workers" = their number, default 64, 0 = off).
 *     Without them -- and always with more than 128 calling threads -- requests that are pending at the same time leave in
 *     one launch: whichever caller finds the launch path free takes everything that is queued, so batches grow with the load;
 *     at most "service_inflight" (4) such batches are in the air;
 *   - the reference pictures of a PU are searched IN PARALLEL.  The loop of :1502-1507 is sequential only through
 *     *inter_cost: a picture whose integer search does not get below it skips search_frac and is re-scored with SATD
 *     (:1239-1252).  Every (PU, picture) unit therefore computes both outcomes -- the search with its fractional stage,
 *     and the integer vector with the SATD cost, which is search_frac's own first candidate (:1019-1029) -- and the call
 *     replays the sequential rule over the units before it returns.  results[i] is what search_pu_inter_ref leaves in
 *     info for picture i when the pictures are visited in order, starting from cost_to_beat;
 *   - descriptors are read, and results written, by the kernels in page-locked host memory: no copy commands, a caller
 *     waits on its own results only.
 * One service per device and picture size.  Thread-safe.  mv_rdo is not available here. */
typedef struct kvz_hip_me_service kvz_hip_me_service;
#define KVZ_HIP_SERVICE_MAX_REFS 16
typedef struct {
  int32_t width, height;        /* luma size of every picture of the service */
  int32_t max_pictures;         /* slots, 1..256 */
  int32_t max_threads;          /* host threads that will ever call kvz_hip_me_service_search (each gets its own result area), 1..1024 */
  int32_t reserved[4];          /* 0 */
} kvz_hip_me_service_config;
typedef struct {
  int32_t pic_slot;             /* the picture being coded */
  int32_t n_refs;               /* 1..KVZ_HIP_SERVICE_MAX_REFS */
  int32_t ref_slot[KVZ_HIP_SERVICE_MAX_REFS];
  uint32_t cost_to_beat;        /* *inter_cost as search_pu_inter hands it to the first picture (MAX_INT, :1492) */
  int32_t reserved;
  kvz_hip_me_params params;     /* as for kvz_hip_search_pu_batch; cost_to_beat / cabac / mv_rdo / size_classes unused (NULL, 0) */
  kvz_hip_me_pu pu[KVZ_HIP_SERVICE_MAX_REFS];   /* the PU as picture i sees it: mv_cand, extra_mv and merge[].same_ref differ per picture */
} kvz_hip_me_request;
typedef struct {
  uint64_t requests, units;     /* searches asked for; (PU, picture) units searched */
  uint64_t batches, launches;   /* a launch per batch: times the queue was drained = kernel launches; resident workers: requests posted to the ring, times workers were started */
  uint64_t max_batch_units;     /* (0 with resident workers) */
  uint64_t rects, rect_bytes;   /* kvz_hip_me_service_put_rect calls and the bytes they moved */
  uint64_t wait_ns;             /* summed over callers: time between posting a request and seeing its results */
  uint64_t tables, table_bytes; /* kvz_hip_me_service_sad_tables: (CTU, picture) tables filled and the bytes the kernels wrote to host memory */
  uint64_t table_ns;            /* summed over callers: time spent in kvz_hip_me_service_sad_tables */
} kvz_hip_me_service_stats;
KVZ_HIP_API kvz_hip_me_service *kvz_hip_me_service_create(const kvz_hip_me_service_config *cfg);
KVZ_HIP_API void kvz_hip_me_service_destroy(kvz_hip_me_service *svc);
/* Copies a w x h rectangle of a host plane (host points at its top-left pixel) to (x, y) of slot's plane; complete on
 * return, so a request posted afterwards by any thread reads it. */
KVZ_HIP_API int kvz_hip_me_service_put_rect(kvz_hip_me_service *svc, int slot, const kvz_hip_pixel *host, uint32_t host_stride,
                                            int x, int y, int w, int h);
/* Blocks until the request's results[0 .. n_refs - 1] are there.  KVZ_HIP_ERR_INVALID for a malformed request (slots, n_refs, parameters,
 * mv_rdo; with the exhaustive search a pu.x that is not a multiple of 4) or PU (outside the picture, impossible shape). */
KVZ_HIP_API int kvz_hip_me_service_search(kvz_hip_me_service *svc, const kvz_hip_me_request *req, kvz_hip_me_result *results);
KVZ_HIP_API int kvz_hip_me_service_get_stats(kvz_hip_me_service *svc, kvz_hip_me_service_stats *out);
/* The device plane of a slot, for a host that wants to run another batched entry on the resident pictures. */
KVZ_HIP_API const kvz_hip_pixel *kvz_hip_me_service_plane(kvz_hip_me_service *svc, int slot);
/* The candidate-INDEPENDENT half of the integer search, for hosts that keep the search itself: every value check_mv_cost
 * (search_inter.c:195-232) can ask kvz_image_calc_sad (image.c:455-486) for while it searches the square PUs of one CTU
 * within +-range full pixels of their own position -- no neighbour decision enters, so the host can ask for it when it
 * starts the CTU.  One kvz_hip_ctu_sad_grid_batch launch per picture (a workgroup per window row: the CTU's source block and
 * that row's reference pixels staged in LDS once, larger PUs as sums of the 8x8 SADs), written by the kernels straight into
 * page-locked host memory owned by the service.  Returns the calling thread's table, valid until its next call:
 *   table[((i * side + (dy + range)) * side + (dx + range)) * KVZ_HIP_CTU_PUS + k],  side = 2 * range + 1,
 * i = index in ref_slots, k = the PU as in kvz_hip_ctu_sad_grid_batch (0: 64x64; 1..4: 32x32; 5..20: 16x16; 21..84: 8x8, raster
 * order inside the CTU); 0xFFFFFFFF = the PU is not inside the picture.  Reference blocks that leave the picture are edge
 * replicated like image_interpolated_sad (image.c:320-444).  range 1..32; ctu_x, ctu_y multiples of 64.  NULL on failure.
 * Bytes per call: n_refs * side^2 * 340 (range 16: 370 KB per picture). */
KVZ_HIP_API const uint32_t *kvz_hip_me_service_sad_tables(kvz_hip_me_service *svc, int pic_slot, int n_refs, const int32_t *ref_slots,
                                                          int ctu_x, int ctu_y, int range);

/* ---- candidate derivation next to the search: what a host derives between two dependency fronts ---- */
/* One record per 4x4 SCU, row-major: the fields of cu_info_t (cu.h:117-153) the candidate derivation and the
 * deblocking filter (below) read.  Inter CUs carry mv_dir 1..3. */
typedef struct {
  uint8_t type;                 /* cu_type_t: CU_INTRA 1, CU_INTER 2 (cu.h:38-43) */
  uint8_t depth, part_size, tr_depth;
  uint8_t cbf_y;                /* cbf_is_set(cu->cbf, cu->tr_depth, COLOR_Y) (cu.h:504-507) */
  uint8_t mv_dir;               /* inter.mv_dir */
  uint8_t qp;                   /* cu->qp */
  uint8_t reserved;
  int16_t mv[2][2];             /* inter.mv */
  uint8_t mv_ref[2];            /* inter.mv_ref */
  uint8_t pad[2];
} kvz_hip_cu_info;              /* 20 bytes */
/* What kvz_inter_get_mv_cand / kvz_inter_get_merge_cand (inter.c:1209-1446) read of the encoder state. */
typedef struct {
  int32_t poc;                   /* state->frame->poc */
  int32_t slice_is_b;            /* state->frame->slicetype == KVZ_SLICE_B */
  int32_t tmvp_enable;           /* cfg.tmvp_enable */
  int32_t num_refs;              /* state->frame->ref->used_size, 0..16 */
  int32_t ref_pocs[16];          /* state->frame->ref->pocs */
  uint8_t ref_LX[2][16];         /* state->frame->ref_LX (encoderstate.h:100) */
  uint8_t ref_LX_size[2];        /* state->frame->ref_LX_size */
  uint8_t pad[2];
  int32_t col_ref_pocs[16];      /* state->frame->ref->images[c]->ref_pocs, c = ref_LX[0][0]: the collocated picture (inter.c:1020-1055) */
  uint8_t col_ref_LX[2][16];     /* state->frame->ref->ref_LXs[c] */
  int32_t pic_width, pic_height; /* state->tile->frame->width / height: the (tile) picture the reference's functions see */
  int32_t in_width, in_height;   /* encoder_control->in.width / height: the bounds of the temporal neighbours (inter.c:747,763) */
  int32_t tile_x, tile_y;        /* state->tile->offset_x / _y.  Descriptors carry PICTURE coordinates (the search entry's
                                    convention); the derivation subtracts the offset, cus is indexed tile-relative, col_cus /
                                    ref_cus picture-wide (the start vector's lookup, search_inter.c:1193-1194, adds it back) */
  int32_t ref_idx;               /* info->ref_idx: the picture of state->frame->ref about to be searched */
  int32_t cus_stride;            /* records per row of cus */
  int32_t col_stride;            /* records per row of col_cus / ref_cus (cu_array_t: the picture width rounded up to whole LCUs, / 4) */
  int32_t reserved;
} kvz_hip_inter_params;          /* 252 bytes */
/* inter_merge_cand_t (inter.h:36-41) */
typedef struct {
  uint8_t dir;                   /* 1 L0, 2 L1, 3 both */
  uint8_t ref[2];                /* index in L0 / L1 */
  uint8_t pad;
  int16_t mv[2][2];
} kvz_hip_merge_cand;            /* 12 bytes */
/* Completes the search descriptors of `count` PUs on the device -- everything search_pu_inter and
 * search_pu_inter_ref derive before the search of picture params->ref_idx (search_inter.c:1470-1500, :1143-1206):
 *   in : pus[i].x, y (picture coordinates), width, height (any PU shape of the inter search) and pus[i].pad: bit 0 = merge candidate A1
 *        barred, bit 1 = B1 barred (the second PU of a two-PU CU, search_inter.c:1470-1475);
 *   out: pus[i].num_merge_cand and merge[] (kvz_inter_get_merge_cand, inter.c:1314-1446, seen as calc_mvd_cost sees
 *        it), mv_cand (kvz_inter_get_mv_cand, inter.c:1209-1240, for the list and index that hold ref_idx),
 *        extra_mv (the vector of the CU of picture ref_idx under the PU's centre, search_inter.c:1190-1206);
 *        merge_out (DEVICE, 5 per PU, may be NULL): the full inter_merge_cand_t list for the merge / skip evaluation.
 * cus = the current (tile) picture's CUs, one kvz_hip_cu_info per 4x4 SCU, holding what lcu->cu holds while its LCU
 * is searched: the decided neighbours (type 0 = not coded yet; of a record only type, mv_dir, mv, mv_ref are read);
 * col_cus = the CUs of the collocated picture ref_LX[0][0] (needed when tmvp_enable and num_refs > 0), ref_cus = those
 * of picture ref_idx (may be NULL: extra_mv 0), both whole-picture arrays.  params is a HOST struct.  A descriptor
 * outside the picture or off the 4-pixel grid gets num_merge_cand -1.  The results feed kvz_hip_search_pu_batch on
 * the same stream: with the CU arrays resident, a dependency front costs no host round trip for its candidates. */
KVZ_HIP_API int kvz_hip_inter_candidates_batch(const kvz_hip_cu_info *cus, const kvz_hip_cu_info *col_cus, const kvz_hip_cu_info *ref_cus,
                                               const kvz_hip_inter_params *params, kvz_hip_me_pu *pus, size_t count,
                                               kvz_hip_merge_cand *merge_out, kvz_hip_stream s);

/* The same derivation for PUs of SEVERAL pictures in one launch (cf. kvz_hip_search_pu_multi_batch): one record per picture
 * in DEVICE memory, a PU names its picture in kvz_hip_me_pu.pad >> 2.  What the one-picture entry refuses as a bad
 * argument (table sizes, strides, a missing collocated array) makes the PUs of that picture read num_merge_cand -1 here,
 * as does a picture index outside 0 .. n_pictures - 1. */
typedef struct {
  const kvz_hip_cu_info *cus, *col_cus, *ref_cus;   /* as the arguments of kvz_hip_inter_candidates_batch */
  kvz_hip_inter_params params;
  int32_t reserved;
} kvz_hip_inter_picture;         /* 280 bytes */
KVZ_HIP_API int kvz_hip_inter_candidates_multi_batch(const kvz_hip_inter_picture *pictures, int n_pictures, kvz_hip_me_pu *pus, size_t count,
                                                     kvz_hip_merge_cand *merge_out, kvz_hip_stream s);


/* Bi-prediction candidate cost of search_pu_inter_bipred (search_inter.c:1304-1440): for candidate i the luma of
 * kvz_inter_recon_bipred (inter.c:430-477; a 14-bit quarter-pel sample per reference when its vector is fractional,
 * else the edge-clamped pixels << 6, blended and clipped) scored with kvz_satd_any_size against the source block
 * (:1359-1362).  The caller adds the MV bit costs (:1366-1389).  Quarter-pel vectors; both reference planes have
 * ref_w x ref_h pixels; width, height multiples of 4 in 4..64 and not both 4 mod 8 (every PU shape), block inside the
 * picture (else cost 0xFFFFFFFF).  pic, ref0 and ref1: any base alignment, three independent strides >= the widths. */
typedef struct {
  int32_t x, y, width, height;
  int16_t mv0[2], mv1[2];
} kvz_hip_bipred_cand;
KVZ_HIP_API int kvz_hip_bipred_cost_batch(const kvz_hip_pixel *pic, uint32_t pic_stride, int pic_w, int pic_h,
                                          const kvz_hip_pixel *ref0, uint32_t ref0_stride,
                                          const kvz_hip_pixel *ref1, uint32_t ref1_stride, int ref_w, int ref_h,
                                          const kvz_hip_bipred_cand *cands, size_t count, uint32_t *costs, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* (2) batched entries -- intra group (strategies/strategies-intra.h)  */
/*     SURVEY.md section 8(f) row 2                                    */
/* ------------------------------------------------------------------ */
/* kvz_intra_ref (intra.h:35-38): reference pixels of one PU, entry 0 of both
 * arrays = the top-left corner, entries 1..2N the left / top neighbours. */
typedef struct {
  kvz_hip_pixel left[2 * 32 + 1];
  kvz_hip_pixel top[2 * 32 + 1];
} kvz_hip_intra_ref;

#define KVZ_HIP_INTRA_LUMA 1             /* color == COLOR_Y */
#define KVZ_HIP_INTRA_FILTER_BOUNDARY 2  /* kvz_intra_predict's filter_boundary */
#define KVZ_HIP_INTRA_RAW 4              /* the bare strategies kvz_angular_pred / kvz_intra_pred_planar
                                            (intra-generic.c:37-189) on the given references: no smoothing
                                            decision, no DC / boundary filters */

/* Luma position of an intra PU in its (tile's) picture: the luma_px argument of
 * kvz_intra_build_reference (intra.h:94-100). */
typedef struct { int32_t x, y; } kvz_hip_intra_pos;

/* kvz_intra_build_reference (intra.c:334-588) for every listed PU, gathered on
 * the device from `rec`, the plane of `color` (0 Y, 1 U, 2 V; stride in pixels
 * of that plane) of the reconstruction BEFORE deblocking -- what lcu->rec,
 * lcu->top_ref and lcu->left_ref are views of (init_lcu_t,
 * search.c:761-835).  pic_width / pic_height are pic_px, the luma size of
 * the (tile) picture (multiples of 8, as the encoder pads them).  Which neighbours count as coded follows from the PU's
 * place in the coding order of its LCU exactly as num_ref_pixels_top / _left
 * (intra.c:35-70) say, so pixels of CUs that come later are never read and may
 * hold anything.  Entries 0..2N of both arrays are the reference's, the rest
 * is zero.  A position outside the picture or off the 4-pixel grid yields an
 * all-zero record.  refs feeds kvz_hip_intra_predict_batch / _rough_batch on
 * the same stream without a host round trip.  rec: any base alignment, any stride >= the width of the plane (pixels
 * are read one byte at a time); nothing right of the plane's width is read. */
KVZ_HIP_API int kvz_hip_intra_build_reference_batch(int log2_width, int color, const kvz_hip_pixel *rec, int stride,
                                                    int pic_width, int pic_height, const kvz_hip_intra_pos *pus, size_t count,
                                                    kvz_hip_intra_ref *refs, kvz_hip_stream s);

/* kvz_intra_predict (intra.c:281-331) for every PU x every listed mode:
 * reference smoothing (intra.c:164-192) chosen per mode and size, planar,
 * DC with its edge filter (intra.c:217-278), angular modes 2..34 with the
 * boundary post-process of modes 10 / 26 (intra.c:195-208).  modes is a HOST
 * array of num_modes (1..35) mode numbers; prediction (i, k) is written as
 * N*N contiguous pixels at dst + (i * num_modes + k) * N * N. */
KVZ_HIP_API int kvz_hip_intra_predict_batch(int log2_width, int flags, const kvz_hip_intra_ref *refs, size_t count,
                                            const int8_t *modes, int num_modes, kvz_hip_pixel *dst, kvz_hip_stream s);

/* The cost loop of search_intra_rough (search_intra.c:404-520) for all 35
 * modes at once: satd_costs[35*i + m] = satd_NxN(kvz_intra_predict(mode m), orig_i)
 * (luma), orig = count contiguous N x N blocks.  sad_costs (NULL, or same shape)
 * receives sad_NxN for the 4x4 transform-skip test of get_cost
 * (search_intra.c:99-126).  The host walks the table in the reference's order
 * and adds the mode-bit cost, so decisions are identical; predictions never
 * leave the CU. */
KVZ_HIP_API int kvz_hip_intra_rough_batch(int log2_width, int flags, const kvz_hip_intra_ref *refs,
                                          const kvz_hip_pixel *orig, size_t count,
                                          uint32_t *satd_costs, uint32_t *sad_costs, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* (2) batched entries -- SAO group (strategies/strategies-sao.h)      */
/*     SURVEY.md section 8(f) row 4                                    */
/* ------------------------------------------------------------------ */
/* Statistics / distortion entries: `count` contiguous block_width x
 * block_height blocks (stride = block_width, at most 64 x 64), the way
 * sao.c blits an LCU plane before calling the strategies. */

/* calc_sao_edge_dir (sao-generic.c:80-109) for the four edge classes at once:
 * cat_sum_cnt[((i * 4 + eo_class) * 2 + {0 sum, 1 count}) * 5 + category]. */
KVZ_HIP_API int kvz_hip_sao_edge_stats_batch(const kvz_hip_pixel *orig, const kvz_hip_pixel *rec, int block_width, int block_height,
                                             size_t count, int32_t *cat_sum_cnt, kvz_hip_stream s);
/* sao_edge_ddistortion (sao-generic.c:46-77) for the four classes:
 * ddistortion[i * 4 + eo_class] with offsets[(i * 4 + eo_class) * 5 + category]. */
KVZ_HIP_API int kvz_hip_sao_edge_ddistortion_batch(const kvz_hip_pixel *orig, const kvz_hip_pixel *rec, int block_width, int block_height,
                                                   size_t count, const int32_t *offsets, int32_t *ddistortion, kvz_hip_stream s);
/* calc_sao_bands (sao.c:247-261): sao_bands[(i * 2 + {0 sum, 1 count}) * 32 + band] */
KVZ_HIP_API int kvz_hip_sao_band_stats_batch(const kvz_hip_pixel *orig, const kvz_hip_pixel *rec, int block_width, int block_height,
                                             size_t count, int32_t *sao_bands, kvz_hip_stream s);
/* sao_band_ddistortion (sao-generic.c:157-183): ddistortion[i] for band_pos[i], sao_bands[i * 4 + k] */
KVZ_HIP_API int kvz_hip_sao_band_ddistortion_batch(const kvz_hip_pixel *orig, const kvz_hip_pixel *rec, int block_width, int block_height,
                                                   size_t count, const int32_t *band_pos, const int32_t *sao_bands,
                                                   int32_t *ddistortion, kvz_hip_stream s);

/* the fields of sao_info_t (sao.h:42-50) the reconstruction reads */
typedef struct {
  int32_t type;                 /* SAO_TYPE_NONE 0 (copy), SAO_TYPE_BAND 1, SAO_TYPE_EDGE 2 */
  int32_t eo_class;
  int32_t band_position[2];     /* [0] Y / U, [1] V */
  int32_t offsets[10];          /* [0..4] Y / U, [5..9] V */
} kvz_hip_sao_info;
typedef struct { int32_t x, y, width, height, sao_index; } kvz_hip_sao_block;
/* sao_reconstruct_color (sao-generic.c:112-154, with kvz_calc_sao_offset_array,
 * sao.c:164-180) for `count` blocks of one plane: new_rec <- filter(rec) inside
 * each block.  Edge blocks read one pixel beyond the block in the directions of
 * their class, so the caller trims them at the picture border like
 * kvz_sao_reconstruct (sao.c:296-318); a descriptor whose reads would leave the
 * plane is skipped -- "the plane" is plane_w x plane_h, not the stride: a read of the bytes between plane_w and the
 * stride counts as outside.  color 0 Y, 1 U, 2 V.  rec and new_rec: any base alignment, independent strides >=
 * plane_w; new_rec is written inside the executed blocks only (its other pixels and its padding keep their bytes). */
KVZ_HIP_API int kvz_hip_sao_reconstruct_color_batch(const kvz_hip_pixel *rec, uint32_t stride, int plane_w, int plane_h,
                                                    kvz_hip_pixel *new_rec, uint32_t new_stride,
                                                    const kvz_hip_sao_block *blocks, size_t count,
                                                    const kvz_hip_sao_info *infos, int n_infos, int color, kvz_hip_stream s);

/* The whole-picture SAO entries, kvz_hip_sao_stats_frame and kvz_hip_sao_frame, take a kvz_hip_ref_picture and are declared
 * with the picture chain below, after kvz_hip_inter_residual_frame. */

/* ------------------------------------------------------------------ */
/* deblocking of a reconstructed frame                                 */
/*   reference: kvz_filter_deblock_lcu (filter.c:770-779) called for   */
/*   every LCU (encoderstate.c:579-616), with filter.c:83-768 below it */
/*   SURVEY.md section 8(f) row 4                                      */
/* ------------------------------------------------------------------ */
/* cus: kvz_hip_cu_info records (defined with the candidate derivation above), one per 4x4 SCU, row-major,
 * ceil(width / 4) records per row. */
typedef struct {
  int32_t beta_offset_div2;     /* cfg.deblock_beta */
  int32_t tc_offset_div2;       /* cfg.deblock_tc */
  int32_t qp;                   /* state->qp, used when per_cu_qp == 0 (get_qp_y_pred, filter.c:263-282) */
  int32_t frame_qp;             /* state->frame->QP */
  int32_t per_cu_qp;            /* encoder_control->max_qp_delta_depth >= 0 */
  int32_t slice_is_b;           /* state->frame->slicetype == KVZ_SLICE_B */
  int32_t chroma;               /* 0: 4:0:0 (rec_u / rec_v unused), 1: 4:2:0 */
  int32_t reserved;
  uint8_t ref_LX[2][16];        /* state->frame->ref_LX (encoderstate.h:100) */
} kvz_hip_deblock_params;       /* 64 bytes */
/* Filters the planes in place: every vertical edge of the frame, then every
 * horizontal edge (two launches) -- the order the reference's LCU walk with its
 * deferred rightmost 4 pixels (filter.c:711-779) implements.  width / height
 * multiples of 8, planes / strides / cus 4-byte aligned (anything else returns KVZ_HIP_ERR_INVALID and writes
 * nothing); stride_y and stride_c are independent (stride_c need not be stride_y / 2), rec_u and rec_v share
 * stride_c; the bytes between width and stride are neither read nor written.  Bitdepth 8, lossless
 * and PCM blocks are not handled (kvz_filter_deblock_lcu asserts !lossless). */
KVZ_HIP_API int kvz_hip_deblock_frame(kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v,
                                      uint32_t stride_c, int width, int height, const kvz_hip_cu_info *cus,
                                      const kvz_hip_deblock_params *params, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* motion compensation (inter recon) of PUs and of a whole picture     */
/*   reference: kvz_inter_recon_cu (inter.c:492-540) through           */
/*   inter_recon_unipred / kvz_inter_recon_bipred (inter.c:314-477),   */
/*   the sample filters of ipol-generic.c:122-190, :660-728 and the    */
/*   blend of inter_recon_bipred_generic (picture-generic.c:538-588)   */
/* ------------------------------------------------------------------ */
#define KVZ_HIP_MAX_REF_PICTURES 16
/* One reference picture (kvz_picture, image.h:53-74): DEVICE planes.  width / height are the luma size, multiples of 8;
 * the chroma planes are width/2 x height/2 (4:2:0; u, v unused and may be NULL for 4:0:0).  Strides may exceed the
 * widths; nothing right of the width or below the height of a plane is ever read. */
typedef struct {
  const kvz_hip_pixel *y, *u, *v;
  uint32_t stride_y, stride_c;
  int32_t width, height;
} kvz_hip_ref_picture;          /* 40 bytes */
/* One PU as kvz_inter_recon_cu hands it to inter_recon_unipred / kvz_inter_recon_bipred (inter.c:501-538). */
typedef struct {
  int32_t x, y, width, height;  /* luma rectangle in PICTURE coordinates; x, y multiples of 4 */
  int16_t mv[2][2];             /* inter.mv: [list][x, y], quarter-pel */
  uint8_t mv_dir;               /* inter.mv_dir: 1 L0, 2 L1, 3 both */
  uint8_t ref[2];               /* per list: index into the table of reference pictures, i.e. ref_LX[list][mv_ref[list]] */
  uint8_t pad;
} kvz_hip_inter_pu;             /* 28 bytes */
/* Writes the Y, U and V prediction of `count` PUs into the destination planes, at the PUs' own positions, bit-exact
 * with the reference's generic strategy at bit depth 8:
 *   uni-prediction (inter_recon_unipred with hi_prec_out == NULL, inter.c:314-421): luma kvz_sample_quarterpel_luma on
 *     the window of kvz_get_extended_block when mv & 3 is non-zero in either component, else the pixels with each
 *     coordinate clamped to the picture (inter_cp_with_ext_border, inter.c:277-298; inside the picture the plain blit);
 *     chroma kvz_sample_octpel_chroma at (x >> 1, y >> 1) + ((mv >> 2) >> 1) with fraction mv & 7 when mv & 7 is
 *     non-zero in either component, else the clamped copy;
 *   bi-prediction (kvz_inter_recon_bipred, inter.c:435-477): per reference and per plane the 14-bit sample
 *     (kvz_sample_14bit_quarterpel_luma / _octpel_chroma) when that plane's fraction is non-zero, else the clamped pixel
 *     << 6; result clip((s0 + s1 + 64) >> 7) (picture-generic.c:538-588).  A luma-integer, chroma-fractional vector
 *     (mv & 7 == 4) mixes the two kinds in one PU, as the reference does.  The 14-bit samples never leave the chip.
 * refs is a HOST table of n_refs (1..16) pictures of one size, which is the size of the picture being predicted; it
 * is copied at the call.  pus is a DEVICE array.  PU shapes: every shape of the inter search -- sides multiples of 4 in
 * 4..64, never both 4 mod 8 -- inside the picture; vectors may point anywhere.  A descriptor of another shape, off
 * the 4-pixel grid, outside the picture, with mv_dir outside 1..3 or with a used ref index >= n_refs is skipped:
 * nothing is written for it.  Only the pixels of valid PUs are written; the destination planes must not alias a
 * reference plane.  chroma: 1 = 4:2:0, 0 = 4:0:0 (pred_u / pred_v unused, may be NULL).  count == 0 is a no-op; a
 * missing pointer or a malformed table returns KVZ_HIP_ERR_INVALID.  Asynchronous on s, no host synchronisation,
 * usable between kvz_hip_graph_begin / _end.
 * Coordinates are picture-wide: the reference adds state->tile->offset_x / _y before it clamps against the whole
 * picture (inter.c:328-331), so a tile-relative caller gets the same pixels by passing picture coordinates. */
KVZ_HIP_API int kvz_hip_inter_recon_batch(const kvz_hip_ref_picture *refs, int n_refs, const kvz_hip_inter_pu *pus, size_t count,
                                          kvz_hip_pixel *pred_y, uint32_t stride_y, kvz_hip_pixel *pred_u, kvz_hip_pixel *pred_v,
                                          uint32_t stride_c, int chroma, kvz_hip_stream s);
typedef struct {
  int32_t chroma;               /* 0: 4:0:0 (pred_u / pred_v unused), 1: 4:2:0 */
  int32_t n_refs;               /* pictures in the table, 1..16 */
  uint8_t ref_LX[2][16];        /* state->frame->ref_LX (encoderstate.h:100) */
} kvz_hip_inter_recon_params;   /* 40 bytes */
/* kvz_inter_recon_cu (inter.c:492-540) for every inter CU of a picture, in one asynchronous call: the prediction of
 * the picture from its CU array.  cus: DEVICE, one kvz_hip_cu_info per 4x4 SCU, row-major, ceil(width / 4) records
 * per row, 4-byte aligned (as kvz_hip_deblock_frame takes it).  A CU is 64 >> depth wide at the SCU position rounded
 * down to that size; part_size is read from the CU's first record, the PUs are those of PU_GET_X / _Y / _W / _H
 * (cu.h:69-104) for all eight part modes, and each PU's mv_dir, mv and mv_ref are read from the record at the PU's own
 * top-left SCU (inter.c:507); its pictures are refs[params->ref_LX[list][mv_ref[list]]].  Records whose type is not
 * CU_INTER (intra, or 0 = not coded yet) contribute nothing and their destination pixels are left untouched.  A CU
 * that would leave the picture is skipped, and so is a PU whose shape kvz_hip_inter_recon_batch would skip (an 8x8 CU
 * in NxN or an AMP mode) or whose reference resolves outside the table.  The PUs are enumerated on the device: no
 * host round trip, and a captured call (kvz_hip_graph_begin / _end) may be replayed after the CONTENTS of cus changed.
 * The records of all SCUs of one PU must agree about the CU's depth and type (cu_array_t holds copies of one
 * cu_info_t, cu.c:167-190); a map that disagrees inside a PU is a caller error: the output inside that CU is
 * unspecified, but no access leaves the planes.  refs, params: HOST, copied at the call.  width, height: multiples of 8
 * and the size of every reference picture.  Coordinates are picture-wide, as for kvz_hip_inter_recon_batch.
 * Several independent pictures in one call: kvz_hip_inter_recon_frames, near the end of this header, whose records index one shared
 * pool of reference pictures. */
KVZ_HIP_API int kvz_hip_inter_recon_frame(kvz_hip_pixel *pred_y, uint32_t stride_y, kvz_hip_pixel *pred_u, kvz_hip_pixel *pred_v,
                                          uint32_t stride_c, int width, int height, const kvz_hip_cu_info *cus,
                                          const kvz_hip_ref_picture *refs, const kvz_hip_inter_recon_params *params,
                                          kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* residual coding and reconstruction of a picture's inter CUs         */
/*   reference: kvz_quantize_lcu_residual (transform.c:424-482, called */
/*   at search.c:587) over quantize_tr_residual (transform.c:281-406)  */
/*   and the rdoq-off path of kvz_quantize_residual                    */
/*   (quant-generic.c:180-273); flags as lcu_set_coeff leaves them     */
/*   (search.c:173-190); cost inputs of search.c:580-642               */
/* ------------------------------------------------------------------ */
typedef struct {
  int32_t qp;               /* state->qp: one QP per call */
  int32_t slice_is_intra;   /* state->frame->slicetype == KVZ_SLICE_I */
  int32_t signhide;         /* encoder->cfg.signhide_enable */
  int32_t scaling_list;     /* 0: flat lists; non-zero with the _sl entries only, which take the tables (below) */
  int32_t chroma;           /* 0: 4:0:0 (U / V pointers unused), 1: 4:2:0 */
  int32_t reserved;
} kvz_hip_inter_residual_params;   /* 24 bytes; the first four fields are those of kvz_hip_quant_params */
/* What the rd=0 cost of a CU and its zero-coefficient alternative are made of (search.c:580-642), as raw integers: the caller
 * applies the chroma weight and lambda.  c = U + V. */
typedef struct {
  uint32_t ssd_y, ssd_c;             /* sum of kvz_pixels_calc_ssd(source, reconstruction) over the CU's TUs */
  uint32_t zero_ssd_y, zero_ssd_c;   /* the same against the PREDICTION: the input of cu_zero_coeff_cost */
  uint32_t coeff_abs_y, coeff_abs_c; /* sum of kvz_coeff_abs_sum over the CU's TUs */
} kvz_hip_inter_residual_cost;     /* 24 bytes */
/* kvz_quantize_lcu_residual for every inter CU of a picture, in one asynchronous call, between kvz_hip_inter_recon_frame and
 * kvz_hip_deblock_frame: prediction -> residual coding -> deblocking of a picture are three calls on one stream, driven by
 * one CU array, with no host involvement.
 * src: HOST, copied at the call; the source picture (DEVICE planes, const); its width / height (multiples of 8) are the
 *   picture's.  rec_y / rec_u / rec_v: DEVICE planes that hold the PREDICTION on entry (what kvz_hip_inter_recon_frame wrote)
 *   and the reconstruction on return -- in place, as lcu->rec in the reference.  cus: DEVICE, one kvz_hip_cu_info per 4x4 SCU,
 *   row-major, ceil(width / 4) per row, 4-byte aligned; READ AND WRITTEN.  params: HOST, copied at the call.
 * Which CUs: records of type CU_INTER; a CU is 64 >> depth wide at the SCU position rounded down to that size, and a CU that
 *   would leave the picture is skipped (the rules of kvz_hip_inter_recon_frame).  Everything that belongs to other records
 *   is left untouched: rec, coefficients, flags, costs.
 * Transform tree (transform.c:448-481): the luma leaf depth is max(depth, tr_depth, 1), at most 4 -- luma TUs 32 / 16 / 8 / 4
 *   wide -- with tr_depth READ FROM THE MAP (from the record at the TU's own top-left SCU), not derived from part_size.  Chroma
 *   TUs are half as wide; with 4x4 luma TUs the chroma of the 8x8 area is one 4x4 TU per plane (transform.c:293-313).
 * Per TU: kvz_quantize_residual, rdoq off (quant-generic.c:180-273), cu_is_intra = 0, diagonal scan (kvz_get_scan_order of
 *   an inter CU), no transform skip; bit-exact with the generic strategy at bit depth 8.  A picture coded with --lossless goes
 *   through kvz_hip_inter_residual_frame_lossless (below) instead.  OUT OF SCOPE:
 *   transform skip, RDOQ, scaling lists (params->scaling_list != 0 returns KVZ_HIP_ERR_INVALID; kvz_hip_inter_residual_frame_sl
 *   below takes them) and per-CU QP (the qp field of the records is not read; a QP per LCU: kvz_hip_inter_residual_frame_qp below).  Intra CUs need their neighbours' reconstruction and are not handled, as in
 *   kvz_hip_inter_recon_frame: kvz_hip_intra_recon_frame (below) does them next.  RDOQ is built since as a batch entry of its own,
 *   kvz_hip_rdoq_batch (further below); this stage does not call it.  Since then kvz_hip_inter_residual_frame_rdoq
 *   (further below) is this stage with kvz_rdoq as its quantiser.
 * Outputs:
 *   rec planes: the reconstruction inside the inter CUs (a TU without coefficients keeps its prediction).
 *   coeff_y / coeff_u / coeff_v: DEVICE, 16-byte aligned, the layout of lcu->coeff: per LCU, in raster order of the
 *     ceil(width / 64) x ceil(height / 64) LCUs, 4096 luma and 1024 + 1024 chroma values; the w * w values of a TU at (lx, ly)
 *     inside its LCU are contiguous and row-major at xy_to_zorder(64, lx, ly) (chroma: xy_to_zorder(32, lx / 2, ly / 2)),
 *     cu.h:373-410.  A TU without coefficients gets zeros.
 *   cus[i].cbf_y of every SCU of an inter CU = has_coeffs of the luma leaf TU that covers it: what lcu_set_coeff
 *     (search.c:173-190) leaves for the deblocking filter, so kvz_hip_deblock_frame can run next on the same array.
 *   cbf_out (optional, may be NULL): DEVICE, one byte per SCU: bit 0 Y, bit 1 U, bit 2 V of the covering leaf TUs.
 *   costs (optional, may be NULL): DEVICE, shaped like cus; the record at the index of each inter CU's top-left SCU
 *     receives the CU's sums.  Integer sums: the result does not depend on scheduling.
 * Asynchronous on s; no host synchronisation, no allocation and no scratch memory.  Usable between kvz_hip_graph_begin / _end,
 * and a captured call may be replayed after the CONTENTS of cus, of the source and of the prediction changed: the TUs are
 * found on the device by launches of a fixed shape.  The records of all SCUs of one CU must agree; a map that disagrees
 * inside a CU is a caller error with unspecified output inside that CU, but no access leaves the planes or arrays.
 * A missing required pointer, a size that is not a multiple of 8, a stride below the width or scaling_list != 0 returns
 * KVZ_HIP_ERR_INVALID and nothing is written. */
KVZ_HIP_API int kvz_hip_inter_residual_frame(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                             kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                             kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v,
                                             uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                             const kvz_hip_inter_residual_params *params, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* prediction, residual coding and reconstruction of a picture's       */
/* intra CUs                                                           */
/*   reference: kvz_intra_recon_cu (intra.c:652-706): per leaf TU      */
/*   intra_recon_tb_leaf (intra.c:590-638) and quantize_tr_residual    */
/*   (transform.c:281-406)                                             */
/* ------------------------------------------------------------------ */
/* kvz_intra_recon_cu for every intra CU of a picture, in coding order, in one asynchronous call: after
 * kvz_hip_inter_residual_frame and before kvz_hip_deblock_frame, on the same planes, the same CU array and the same coefficient
 * arrays.  Inter CUs do not depend on intra CUs, so the inter part of the picture is complete before this call; an intra TU reads
 * whatever the planes hold around it, as in the reference (there is no constrained intra prediction).
 * Arguments, sizes, the coefficient layout and the error rules are those of kvz_hip_inter_residual_frame; params is the same struct
 * (scaling_list must be 0, the qp field of the records is not read).  Planes: any base alignment and any strides >= the widths
 * (PLANES above); cus 4-byte aligned, the coefficient arrays 16-byte aligned.
 * intra_modes: DEVICE, required, two bytes per 4x4 SCU in the raster of cus: [2 i] = intra.mode, [2 i + 1] = intra.mode_chroma,
 *   the actual mode 0..34 as cu_info_t holds it (not the syntax index).  A luma TU uses the luma byte of the SCU at its own
 *   top-left -- which gives the four PUs of an NxN CU their own modes; part_size is not read.  A chroma TU uses the chroma byte
 *   of the SCU at its luma top-left; with 4x4 luma TUs that is the first SCU of the 8x8 area (transform.c:293-300, intra.c:694).
 *   A TU whose mode is above 34 is skipped: its pixels, coefficients and flags are unspecified, but no access leaves the planes.
 * Which CUs: records of type CU_INTRA with depth 0..3 whose CU lies inside the picture (the rules of the inter entries with the
 *   type swapped).  Everything that belongs to other records is left untouched: rec, coefficients, flags, costs.
 * Transform tree: luma leaf depth min(4, max(depth, tr_depth, 1)), tr_depth read from the record at the TU's own top-left SCU;
 *   prediction happens at the leaf TU size.  Chroma TUs are half as wide; with 4x4 luma TUs there is one 4x4 chroma TU per plane
 *   per 8x8 area.
 * Per TU, bit-exact with the generic strategy at bit depth 8: the reference pixels as kvz_hip_intra_build_reference_batch defines
 *   them, taken from the rec plane of that colour (availability follows position alone); kvz_intra_predict with filter_boundary
 *   for luma; kvz_quantize_residual, rdoq off, cu_is_intra = 1 (DST for 4x4 luma), under the scan of kvz_get_scan_order
 *   (encoderstate.c:1384-1398: luma TUs 8 or 4 wide and chroma TUs 4 wide scan vertically for modes 6..14 and horizontally for
 *   22..30), which matters through sign hiding.  No transform skip; a picture coded with --lossless goes through
 *   kvz_hip_intra_recon_frame_lossless (below) instead.
 * Outputs:
 *   rec planes: the reconstruction inside the intra CUs (a TU without coefficients keeps its prediction); their contents on
 *     entry are never used.
 *   coeff_y / coeff_u / coeff_v: the LCU layout of kvz_hip_inter_residual_frame; zeros for a TU without coefficients.
 *   cus[i].cbf_y of every SCU of an intra CU = has_coeffs of the covering luma leaf.
 *   cbf_out (optional): the bytes of the intra CUs' SCUs are SET to bit 0 Y, bit 1 U, bit 2 V of the covering leaf TUs.  Bits are
 *     set with atomic ORs on aligned dwords: if the array is not 4-byte aligned, up to 3 bytes in front of and behind it are
 *     accessed too (OR with 0, their values do not change) and must be mapped; the same holds for kvz_hip_inter_residual_frame.
 *   costs (optional): the record at each intra CU's top-left SCU receives ssd_*, coeff_abs_* and zero_ssd_* = the SSD of the
 *     source against the intra prediction.
 * Order: the LCUs are done in wavefronts t = lcu_x + 2 lcu_y, one launch per wavefront -- ceil(width / 64) + 2 (ceil(height / 64)
 *   - 1) launches, whatever the map holds -- and Y, U, V side by side.  Asynchronous on s; no host synchronisation, no allocation
 *   and no workspace: the call owns no device buffer (the kernel does spill a few registers per lane to the private memory that
 *   the runtime provides to any kernel).  Usable between kvz_hip_graph_begin / _end, and a captured call may be replayed after the CONTENTS of
 *   cus, intra_modes, the source and the planes changed.  A map whose records disagree inside a CU gives unspecified output
 *   inside that CU, but the call completes and no access leaves the planes or arrays.
 * A missing required pointer (intra_modes included), a misaligned cus / coeff array, a size that is not a multiple of 8, a stride
 * below the width or scaling_list != 0 returns KVZ_HIP_ERR_INVALID and nothing is written. */
KVZ_HIP_API int kvz_hip_intra_recon_frame(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                          kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                          const uint8_t *intra_modes, kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u,
                                          kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                          const kvz_hip_inter_residual_params *params, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* a QP per LCU in the picture chain                                   */
/*   reference: kvz_set_lcu_lambda_and_qp (rate_control.c:278-340,     */
/*   called at encoderstate.c:619) sets state->qp per LCU under a      */
/*   bitrate target or a ROI map; cur_cu->qp = state->qp               */
/*   (search.c:451); set_cu_qps (encoderstate.c:550-609)               */
/* ------------------------------------------------------------------ */
/* kvz_hip_inter_residual_frame and kvz_hip_intra_recon_frame with one more argument, for pictures whose QP changes from LCU to LCU
 * (rate control, --roi).  The rate-control model stays with the host and supplies the array.
 * lcu_qp: DEVICE, one int8_t per LCU in raster order over the ceil(width / 64) x ceil(height / 64) LCUs (the convention of the SAO
 *   arrays), any alignment: state->qp of each LCU.  A value outside 0..51 is clamped into 0..51 (the reference never produces one,
 *   CLIP_TO_QP), so no value makes an access leave a table.
 * Every TU is quantised and dequantised with the QP of the LCU it lies in: luma with that QP, chroma with its image under
 *   kvz_get_scaled_qp (transform.c:129-143).  Everything that depends on the QP follows it per LCU: q_bits, add and the quant factor,
 *   and the dequant scale, shift and add (quant-generic.c:40-50, :283-320), derived on the device by the function the host uses for
 *   the one-QP entries.  params->qp is ignored when lcu_qp is given.  lcu_qp == NULL: params->qp everywhere, byte for byte the old
 *   entry (it launches the old entry's kernels; kvz_hip_intra_recon_frame_qp calls the old entry, which then names itself in
 *   kvz_hip_last_error).
 * In every other respect -- planes and their alignment rules, the CU and transform tree rules, the coefficient layout, outputs,
 *   error returns, capture -- they are the entries above.  They do NOT write cus[].qp: kvz_hip_cu_qp_frame below writes it.  A
 *   captured call may be replayed after the contents of lcu_qp changed. */
KVZ_HIP_API int kvz_hip_inter_residual_frame_qp(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                                kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                                kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v,
                                                uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp,
                                                const kvz_hip_inter_residual_params *params, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_intra_recon_frame_qp(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                             kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                             const uint8_t *intra_modes, kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u,
                                             kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                             const int8_t *lcu_qp, const kvz_hip_inter_residual_params *params, kvz_hip_stream s);

typedef struct {
  int32_t start_qp;    /* state->frame->QP: last_qp at the start of every chain (encoderstate.c:729), 0..51 */
  int32_t chain_lcus;  /* LCUs per chain, in raster order: 0 = the whole picture is one chain (one slice, one tile, no WPP);
                          ceil(width / 64) = every LCU row is a chain of its own (WPP: each row is a leaf state) */
} kvz_hip_cu_qp_params; /* 8 bytes */
/* set_cu_qps (encoderstate.c:550-609) for every LCU of a picture with max_qp_delta_depth == 0 -- the quantization group is the LCU;
 * zero is the only non-negative value the reference sets (encoder.c:381): the QP map that kvz_hip_deblock_frame reads with
 * per_cu_qp = 1 (get_qp_y_pred, filter.c:263-282), and per LCU the QP predictor that the entropy coder codes cu_qp_delta against
 * (encode_coding_tree.c:511-529).  The chain for such a picture: prediction -> kvz_hip_inter_residual_frame_qp ->
 * kvz_hip_intra_recon_frame_qp -> kvz_hip_cu_qp_frame -> kvz_hip_deblock_frame (per_cu_qp = 1) -> SAO.
 * cus: DEVICE, the picture's records, 4-byte aligned; depth is read, qp is WRITTEN, type is not read.  cbf: DEVICE, the cbf_out array
 *   of the residual entries, one byte per SCU (bits 0..2), any alignment; the caller clears it once before the residual entries, so
 *   SCUs that neither entry covered stay 0.  width / height: multiples of 8, at least 8.  lcu_qp: as above (clamped into 0..51).
 *   lcu_last_qp: DEVICE, required, one int8_t per LCU, WRITTEN.  params: HOST, copied at the call.
 * The CUs of an LCU are the leaves of the walk of encoderstate.c:553-570: a node splits while the record at its top-left has a depth
 *   greater than the node's (a depth above 3 counts as 3); nodes at or beyond the right or bottom edge of the picture are left out.
 *   A CU is CODED iff any of its SCUs (inside the picture) has a non-zero cbf byte -- for a map whose records agree inside a CU this
 *   is cbf_found of encoderstate.c:572-588.
 * Per LCU, with `last` = start_qp at the first LCU of a chain and otherwise what the previous LCU of the chain leaves, and the CUs in
 *   coding order (z-order): every SCU of a CU before the first coded CU gets qp = last; the first coded CU and every CU after it get
 *   the LCU's QP; the LCU leaves last = its own QP if it has a coded CU and last unchanged otherwise.
 *   Derivation.  With max_qp_delta_depth == 0, prev_qp is reset at depth 0 only, i.e. once per LCU; cbf_found = prev_qp >= 0 holds
 *   from the first coded CU on, and those CUs keep cu->qp, which is state->qp of their LCU (search.c:451).  A CU before it gets
 *   kvz_get_cu_ref_qp (encoderstate.c:1408-1430): the group is 64 wide, its corner is the LCU's, x_qg % 64 == y_qg % 64 == 0, both
 *   predictors are last_qp and (2 last_qp + 1) >> 1 = last_qp.  *last_qp = cu->qp runs where is_last_cu_in_qg (encoderstate.h:332-342)
 *   holds and reads the qp just written: the LCU's QP once a coded CU was seen, last_qp itself before.  At a ragged edge the
 *   condition can hold for more than one CU of the LCU (right >= width or bottom >= height); a store before the first coded CU
 *   leaves last_qp as it is, a store after it writes the LCU's QP, which no later CU of the LCU reads (they are all past the first
 *   coded CU) and which the last such store writes again.  So the rule above is the reference's also at ragged edges.
 * Outputs: cus[i].qp of every SCU inside the picture; lcu_last_qp[lcu] = `last` on entry to that LCU.  (Between its launches the
 *   entry keeps its per-LCU intermediate in lcu_last_qp, so it owns no buffer.)
 * Asynchronous on s; no allocation, no host synchronisation, no atomics; three launches whose shapes depend on width, height and
 * chain_lcus only.  Usable between kvz_hip_graph_begin / _end, and a captured call may be replayed after the contents of the
 * arrays changed.  OUT OF SCOPE: tiles (a chain is a raster run of the picture) and max_qp_delta_depth > 0 (which the reference never
 * sets: encoder.c:381-383 makes it 0 or -1).
 * A NULL pointer, a misaligned cus, a size that is not a multiple of 8 or below 8, start_qp outside 0..51, a negative chain_lcus or
 * one that is neither 0 nor a multiple of ceil(width / 64) returns KVZ_HIP_ERR_INVALID and nothing is written. */
KVZ_HIP_API int kvz_hip_cu_qp_frame(kvz_hip_cu_info *cus, const uint8_t *cbf, int width, int height, const int8_t *lcu_qp,
                                    int8_t *lcu_last_qp, const kvz_hip_cu_qp_params *params, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* (2) SAO group, continued: sample adaptive offset of a whole picture */
/*   reference: sao.c:164-337, :355-400, :580-644 with                 */
/*   sao-generic.c:34-109 below them; SURVEY.md section 8(f) row 4     */
/* ------------------------------------------------------------------ */
/* ---- SAO of a whole picture: the stage after kvz_hip_deblock_frame.  Two asynchronous calls that take plane pointers,
 * strides and per-LCU arrays in raster order over the ceil(width / 64) x ceil(height / 64) LCUs (n_lcu of them) and do no
 * host work.  The mode and merge DECISION (sao_search_best_mode, sao.c:467-578, with its CABAC bit costs sao_mode_bits_*)
 * stays with the host: the ddistortion of any candidate is cnt * o * o - 2 * o * sum over the statistics below
 * (sao-generic.c:67-71, :171-178), so the host prices the searched classes, the band candidate and both merge neighbours
 * from the tables without touching a pixel.
 * Planes, for both entries: the rule of kvz_hip_deblock_frame -- planes and strides 4-byte aligned (anything else returns
 * KVZ_HIP_ERR_INVALID and writes nothing), every stride independent and >= its width, the bytes between width and stride
 * never read (nor written).  width / height multiples of 8, at least 8.  Bit depth 8. ---- */

/* Statistics of one plane of one LCU.  The block is the LCU's part of the plane as sao_search_luma / sao_search_chroma
 * (sao.c:580-644) blit it: 64 x 64 luma pixels clipped at the right and bottom picture edge to width - 64 * lcu_x by
 * height - 64 * lcu_y, half that in each direction for chroma (the smallest block is 8 x 8 luma, 4 x 4 chroma). */
typedef struct {
  int32_t edge[4][2][5];   /* [eo_class][0 sum, 1 count][category]: calc_sao_edge_dir (sao-generic.c:82-109) on the block:
                            * its interior 1 .. w-2 x 1 .. h-2 only, so no pixel of a neighbouring LCU is read */
  int32_t band[2][32];     /* [0 sum, 1 count][band]: calc_sao_bands (sao.c:247-261), every pixel of the block */
} kvz_hip_sao_lcu_stats;   /* 416 bytes */
/* The bit-independent results of sao_search_edge_sao and calc_sao_band_offsets for one plane of one LCU, in the reference's
 * integer arithmetic: offset = (sum + (cnt >> 1)) / cnt with C's truncating division, clipped to +-7 (SAO_ABS_OFFSET_MAX at
 * bit depth 8), 0 for an empty category.  For chroma the host adds the U and V records (the reference sums over buf_cnt). */
typedef struct {
  int32_t edge_offsets[4][5];  /* per eo_class and category (sao.c:368-389): categories 1-2 keep positive, 3-4 negative
                                * offsets only; [0] = 0 */
  int32_t edge_ddist[4];       /* per eo_class: sum over categories 1..4 of cnt * o * o - 2 * o * sum (sao.c:397), WITHOUT
                                * the mode bits */
  int32_t band_offsets[4];     /* calc_sao_band_offsets (sao.c:188-240).  Its loop of :213-222 compares with a best_dist that
                                * it never updates, so the offset it records for a band is the last one visited, +-1 with
                                * the sign of the rounded mean: that is what this field holds */
  int32_t band_position;       /* the first minimum over the start bands 0 .. 27 */
  int32_t band_ddist;          /* its return value */
} kvz_hip_sao_lcu_cand;      /* 120 bytes */
/* Statistics and candidates of every LCU and plane of a picture, in one launch.
 * src: HOST, copied at the call; the source picture (DEVICE planes, const), as kvz_hip_inter_residual_frame takes it; its
 *   width / height are the picture's.  rec_y / rec_u / rec_v: the deblocked reconstruction (DEVICE, const).  chroma: 0 for
 *   4:0:0 (the chroma pointers are unused), 1 for 4:2:0.
 * stats (DEVICE, required) / cands (DEVICE, optional, may be NULL): one record per (plane, LCU) at index
 *   color * n_lcu + lcu, color 0 Y, 1 U, 2 V; n_lcu records with chroma == 0, 3 * n_lcu otherwise.  Every field of every
 *   record is written; nothing is accumulated into what was there.  Integer sums: no result depends on scheduling.
 * WHAT THE STATISTICS ARE OF: the planes handed in.  The reference's live encoder calls kvz_sao_search_lcu on an LCU whose
 *   right and bottom edges are not yet deblocked (encoderstate.c:639-647, filter.c:711-779); after a whole-picture
 *   kvz_hip_deblock_frame this call sees other pixels there.  Like the three picture entries before it, this one is not wired
 *   into a live encode: parity is defined against the reference's functions applied to blocks blitted from the same planes.
 * Asynchronous on s; no host synchronisation, no allocation, no scratch memory; usable between kvz_hip_graph_begin / _end and
 * replayable after the contents of the planes changed (the launch shape depends on width, height and chroma only).
 * A NULL required pointer, a size that is not a multiple of 8 or below 8, a stride below the width or a misaligned plane or
 * stride returns KVZ_HIP_ERR_INVALID and nothing is written. */
KVZ_HIP_API int kvz_hip_sao_stats_frame(const kvz_hip_ref_picture *src, const kvz_hip_pixel *rec_y, uint32_t stride_y,
                                        const kvz_hip_pixel *rec_u, const kvz_hip_pixel *rec_v, uint32_t stride_c, int chroma,
                                        kvz_hip_sao_lcu_stats *stats, kvz_hip_sao_lcu_cand *cands, kvz_hip_stream s);
/* kvz_sao_reconstruct (sao.c:278-337) for every LCU and plane of a picture, as encoder_sao_reconstruct
 * (encoderstate.c:245-441) applies it, in one launch: dst <- SAO(rec).
 * rec_*: the deblocked planes (DEVICE, const).  sao_luma[n_lcu], sao_chroma[n_lcu]: DEVICE, 4-byte aligned, in raster order
 *   over the LCUs, as frame->sao_luma / sao_chroma hold them after kvz_sao_search_lcu -- a merged LCU carries its candidate's
 *   parameters (sao.c:684-699).  chroma: 0 for 4:0:0 (chroma planes and sao_chroma unused), 1 for 4:2:0.
 * Per pixel: filtered with the record of the LCU it lies in (x >> 6, y >> 6 luma; x >> 5, y >> 5 chroma); its neighbours
 *   are read from the deblocked plane across LCU boundaries (what the reference keeps its *_before_sao buffers for).  An
 *   edge-offset pixel whose neighbour a or b would lie outside the plane keeps its deblocked value -- per pixel, what the
 *   row and column trimming of sao.c:297-324 amounts to.  Band offset (kvz_calc_sao_offset_array, sao.c:164-180) applies
 *   everywhere; SAO_TYPE_NONE copies.  V uses band_position[1] and offsets[5..9]; Y and U use [0] and offsets[0..4].
 * dst_*: receive every pixel of the width x height (chroma: width / 2 x height / 2) planes, filtered or copied: a complete
 *   picture, the next frame's reference; the bytes between width and stride keep their contents.  Strides of their own.
 *   Out of place only: dst_* == rec_* returns KVZ_HIP_ERR_INVALID, any other overlap is a caller error.
 * Malformed records: a type other than 1 or 2, type 2 with an eo_class outside 0..3, or type 1 with the plane's
 *   band_position outside 0..31 is treated as SAO_TYPE_NONE (a copy).  No record content makes an access leave the planes
 *   or arrays.
 * Asynchronous on s; no host synchronisation, no allocation, no scratch memory; usable between kvz_hip_graph_begin / _end and
 * replayable after the contents of the planes and of the SAO arrays changed.  Errors as kvz_hip_sao_stats_frame. */
KVZ_HIP_API int kvz_hip_sao_frame(const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u,
                                  const kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_pixel *dst_y, uint32_t dst_stride_y,
                                  kvz_hip_pixel *dst_u, kvz_hip_pixel *dst_v, uint32_t dst_stride_c, int width, int height,
                                  const kvz_hip_sao_info *sao_luma, const kvz_hip_sao_info *sao_chroma, int chroma,
                                  kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Tiles in the picture chain: intra, QP map, deblocking and SAO       */
/*   reference: everything in-loop works on state->tile->frame, a      */
/*   sub-picture with its own origin and size (intra.c:334-588,        */
/*   encoderstate.c:550-609 / :729, filter.c:690-779, sao.c:278-337);  */
/*   loop_filter_across_tiles_enabled_flag = 0                         */
/*   (encoder_state-bitstream.c:501)                                   */
/* ------------------------------------------------------------------ */
#define KVZ_HIP_MAX_TILES_PER_DIM 48            /* global.h:217; counts are 1..47 */
typedef struct {
  int32_t cols, rows;                           /* 1..47 each */
  int32_t col_bd[KVZ_HIP_MAX_TILES_PER_DIM];    /* tiles_col_bd (encoder.c:472-475), in LCUs: [0] = 0, strictly increasing,
                                                   [cols] = ceil(width / 64); entries beyond [cols] are not read */
  int32_t row_bd[KVZ_HIP_MAX_TILES_PER_DIM];    /* tiles_row_bd (encoder.c:478-481): [rows] = ceil(height / 64) */
} kvz_hip_tile_grid;                            /* 392 bytes; HOST, copied at the call */
/* The four stages of the chain that depend on tiles, each for a whole tiled picture in one call: the signature of the untiled
 * entry plus the grid, placed before params where there is one, else before the stream.  The stages that do not depend on tiles
 * take a tiled picture as they are: kvz_hip_inter_recon_frame (the reference clamps against the whole picture, inter.c:328-331),
 * kvz_hip_inter_residual_frame(_qp) (per TU) and kvz_hip_sao_stats_frame (LCU interiors only).
 * ONE RULE: the result inside each tile is what the untiled entry gives for a picture that consists of that tile alone -- its
 *   planes the tile's rectangle of the planes, its CU map, modes and cbf bytes the tile's rectangle of the maps, its per-LCU
 *   values the tile's LCUs.
 * Planes, cus, intra_modes, cbf and costs stay picture-wide with their strides; the per-LCU arrays (coefficients, lcu_qp,
 *   lcu_last_qp, sao_luma, sao_chroma) stay in PICTURE RASTER ORDER over the LCUs, as with every other entry and as
 *   kvz_get_lcu_stats indexes them (encoderstate.c:1400-1406); the host's tile scan is its own business.  Alignment and stride
 *   rules are the untiled entry's.
 * grid == NULL is one tile, the whole picture: the outputs are byte for byte the untiled entry's.  A count outside 1..47,
 *   bd[0] != 0, a boundary that does not increase or a last boundary that is not the picture's LCU count returns
 *   KVZ_HIP_ERR_INVALID and nothing is written, as does every error of the untiled entry.
 * Each entry is asynchronous on s, allocates nothing, does not synchronise with the host and owns no workspace; usable between
 *   kvz_hip_graph_begin / _end.  The launch shapes depend on width, height, chroma and the grid only: a captured call replays
 *   after the CONTENTS of every device array changed.
 *
 * kvz_hip_intra_recon_frame_tiles (kvz_intra_recon_cu): the arguments of kvz_hip_intra_recon_frame_qp; lcu_qp may be NULL, which
 *   means params->qp everywhere.  Reference-pixel availability, the clipping of the above-right and below-left runs, has_left /
 *   has_top and the 128 / substitution rules are taken against the TU's tile, and no TU reads a pixel outside its tile: the
 *   tiles of a picture run side by side.  Wavefronts count from each tile's origin, t = (lcu_x - tile_x0) + 2 (lcu_y - tile_y0);
 *   all tiles share launch t, and the number of dependent launches is the maximum over the tiles of w_t + 2 (h_t - 1).
 * kvz_hip_cu_qp_frame_tiles (set_cu_qps): the rule of kvz_hip_cu_qp_frame with the chains chain_rows names; last = start_qp
 *   at the start of every chain, lcu_last_qp[lcu] = last on entry to that LCU. */
typedef struct {
  int32_t start_qp;    /* as kvz_hip_cu_qp_params */
  int32_t chain_rows;  /* 0: every tile is one chain, its LCUs in raster order inside the tile (a tile is a leaf state);
                          1: every LCU row of every tile is a chain (WPP inside tiles); anything else: KVZ_HIP_ERR_INVALID */
} kvz_hip_cu_qp_tiles_params; /* 8 bytes */
/* kvz_hip_deblock_frame_tiles: the vertical edges at 64 col_bd[i] and the horizontal edges at 64 row_bd[j], 0 < i < cols,
 *   0 < j < rows, are not filtered, in luma or in chroma; the right edge of a tile ends the horizontal edges as the right edge of
 *   the picture does (filter.c:645-656).  Everything else is kvz_hip_deblock_frame.  An unfiltered boundary decouples its two
 *   sides, so "all vertical edges, then all horizontal edges" over the picture remains the reference's order inside every tile.
 * kvz_hip_sao_frame_tiles: an edge-offset pixel whose neighbour a or b lies outside its tile keeps its deblocked value; band
 *   offset and copy are kvz_hip_sao_frame's. */
KVZ_HIP_API int kvz_hip_intra_recon_frame_tiles(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                                kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                                const uint8_t *intra_modes, kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u,
                                                kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                                const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                                const kvz_hip_inter_residual_params *params, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_cu_qp_frame_tiles(kvz_hip_cu_info *cus, const uint8_t *cbf, int width, int height, const int8_t *lcu_qp,
                                          int8_t *lcu_last_qp, const kvz_hip_tile_grid *grid,
                                          const kvz_hip_cu_qp_tiles_params *params, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_deblock_frame_tiles(kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v,
                                            uint32_t stride_c, int width, int height, const kvz_hip_cu_info *cus,
                                            const kvz_hip_tile_grid *grid, const kvz_hip_deblock_params *params, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_sao_frame_tiles(const kvz_hip_pixel *rec_y, uint32_t stride_y, const kvz_hip_pixel *rec_u,
                                        const kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_pixel *dst_y, uint32_t dst_stride_y,
                                        kvz_hip_pixel *dst_u, kvz_hip_pixel *dst_v, uint32_t dst_stride_c, int width, int height,
                                        const kvz_hip_sao_info *sao_luma, const kvz_hip_sao_info *sao_chroma, int chroma,
                                        const kvz_hip_tile_grid *grid, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Scaling lists in the picture chain: residual coding and intra recon */
/*   reference: scaling_list_t (scalinglist.h:34-41) as                */
/*   kvz_scalinglist_process leaves it (scalinglist.c:277-411); its    */
/*   use in kvz_quant (quant-generic.c:40-67, :76-77) and kvz_dequant  */
/*   (quant-generic.c:283-320); --scaling-list, --cqmfile              */
/* ------------------------------------------------------------------ */
/* The processed lists of scaling_list_t (scalinglist.h:34-41) as two dense DEVICE arrays of int32, 16-byte aligned:
 * table (size_id, list, rem) -- size_id = log2 N - 2 in 0..3, list 0..5 (0-2 intra Y/U/V, 3-5 inter Y/U/V), rem = qp_scaled % 6 --
 * is the N*N row-major values at  36 * {0, 16, 80, 336}[size_id] + (6 * list + rem) * N * N. */
#define KVZ_HIP_SL_TABLE_LEN 48960            /* 36 * (16 + 64 + 256 + 1024) values per array, 195840 bytes */
typedef struct { const int32_t *quant, *dequant; } kvz_hip_scaling_tables;   /* 16 bytes; HOST struct, copied at the call */

/* Host only: needs no device and no kvz_hip_init.  Copies the tables a Kvazaar host holds after kvz_scalinglist_process
 * (encoder->scaling_list.quant_coeff / .de_quant_coeff, [size_id][list][rem]) into two HOST arrays of KVZ_HIP_SL_TABLE_LEN values
 * in the layout above; the host uploads them with kvz_hip_memcpy_h2d.
 * size_id 3: lists 0, 1 and 3 are read and the tables of lists 2, 4 and 5 are filled with zeros -- the reference allocates two 32x32
 *   lists, aliases [3][3] to [3][1] (scalinglist.c:30, :78-95) and never sets [3][2], [3][4], [3][5], whose pointers are not
 *   dereferenced here.  No 32x32 chroma TU exists, so no kernel reads the zero tables.
 * A NULL argument or a NULL source pointer elsewhere returns KVZ_HIP_ERR_INVALID. */
KVZ_HIP_API int kvz_hip_scaling_tables_pack(const int32_t *const quant_coeff[4][6][6], const int32_t *const de_quant_coeff[4][6][6],
                                            int32_t *quant_out, int32_t *dequant_out);

/* kvz_hip_inter_residual_frame_qp and kvz_hip_intra_recon_frame_tiles with one more argument, placed before params, for pictures
 * coded with scaling lists: these two stages are the ones of the chain that quantise.  The host's three lines: pack, upload, pass.
 * tables == NULL requires params->scaling_list == 0; the call then IS the _qp / _tiles entry, byte for byte (it calls it, and that
 *   entry names itself in kvz_hip_last_error).  tables != NULL requires params->scaling_list != 0 and both pointers non-NULL and
 *   16-byte aligned.  Any mismatch returns KVZ_HIP_ERR_INVALID and nothing is written.  The entries above keep refusing
 *   scaling_list != 0.  lcu_qp == NULL means params->qp everywhere (a negative one is refused); grid == NULL means one tile.
 * Per TU N wide of plane 0 Y / 1 U / 2 V: qp = the QP of the TU's LCU, clamped into 0..51; qps = kvz_get_scaled_qp(plane, qp);
 *   rem = qps % 6; size_id = log2 N - 2; base = 0 in the intra entry and 3 in the inter entry -- it follows the CU's type, not the
 *   slice's.  Quantisation uses list base + (plane ? 1 : 0): the reference quantises V with type 2, U's list (quant-generic.c:223,
 *   :46-47), with the 64-bit product of quant-generic.c:62 (a list entry below 16 gives factors up to 26214 << 4, and
 *   |coef| * factor passes 2^32); the sign-hiding pass reads the same table (:76-77).  Dequantisation uses list base + plane (:244,
 *   :293-295) and takes both branches of :296-311: with shift = log2 N + 3, round and shift right by shift - qps / 6 while
 *   shift > qps / 6, else clip, shift left by qps / 6 - shift, clip.  q_bits and add are those of flat lists.
 * In every other respect -- planes and their alignment rules, the CU and transform-tree rules, the coefficient layout, cbf_y /
 *   cbf_out / costs, tiles, error returns, launches, capture -- they are the entries they extend.  A captured call may be replayed
 *   after the CONTENTS of the two arrays changed (the pointers are part of the capture).
 * OUT OF SCOPE: RDOQ and its error_scale, transform skip, parsing --cqmfile, signalling the lists.  Lossless coding has entries of
 * its own, kvz_hip_inter_residual_frame_lossless and kvz_hip_intra_recon_frame_lossless (below): nothing is quantised there.
 * RDOQ with its error_scale is built since as a batch entry of its own, kvz_hip_rdoq_batch with kvz_hip_rdoq_tables_pack (further
 * below); these two stages still quantise with the rdoq-off path.  Since then kvz_hip_inter_residual_frame_rdoq and
 * kvz_hip_intra_recon_frame_rdoq (further below) are the two _sl entries with kvz_rdoq as their quantiser. */
KVZ_HIP_API int kvz_hip_inter_residual_frame_sl(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                                kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                                kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v,
                                                uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp,
                                                const kvz_hip_scaling_tables *tables,
                                                const kvz_hip_inter_residual_params *params, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_intra_recon_frame_sl(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                             kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                             const uint8_t *intra_modes, kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u,
                                             kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                             const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                             const kvz_hip_scaling_tables *tables,
                                             const kvz_hip_inter_residual_params *params, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Transform skip in the picture chain: residual coding, intra recon   */
/*   reference: kvz_quantize_residual_trskip (transform.c:229-276) as  */
/*   quantize_tr_residual calls it (transform.c:348-387);              */
/*   kvz_transformskip / kvz_itransformskip (transform.c:151-181);     */
/*   kvz_get_coeff_cost below fast_residual_cost_limit                 */
/*   (rdo.c:44-45, :208-222); --transform-skip, --fast-residual-cost   */
/* ------------------------------------------------------------------ */
typedef struct {
  int32_t bit_cost;             /* (int)(state->lambda + 0.5), transform.c:244; used where lcu_bit_cost == NULL; >= 0 */
  int32_t reserved;
  const int32_t *lcu_bit_cost;  /* DEVICE, optional: one value per LCU in picture raster order (lambda follows the LCU under
                                   rate control, rate_control.c:278-340); negative values count as 0 */
} kvz_hip_trskip;               /* 16 bytes; HOST struct, copied at the call */

/* kvz_hip_inter_residual_frame_sl and kvz_hip_intra_recon_frame_sl with two more arguments, placed before params, for pictures coded
 * with --transform-skip (cfg.trskip_enable).
 * ts == NULL: the call IS the _sl entry, byte for byte (it calls it, and that entry names itself in kvz_hip_last_error);
 *   tr_skip_out is not touched.  ts != NULL: every combination of lcu_qp, grid and tables that the _sl entry accepts is accepted.
 * tr_skip_out: DEVICE, one byte per 4x4 SCU in the raster of cus, any alignment; required with ts != NULL.
 * Which TUs: the 4x4 luma leaf TUs of the CUs the entry handles -- those for which can_use_trskip holds (transform.c:348-350).
 *   Chroma TUs and larger luma TUs are coded exactly as by the _sl entry.
 * Per such TU, kvz_quantize_residual runs twice on the same source and prediction, with the same scan order, sign hiding, QP
 *   constants and scaling tables, use_trskip = 0 then 1.  The transformed trial uses the DST in the intra entry and the DCT in the
 *   inter entry.  The skipped trial is kvz_transformskip / kvz_itransformskip: coefficient = residual << 5, residual =
 *   (coefficient + 16) >> 5 (bit depth 8).  Scaling lists apply to the skipped coefficients too: quant-generic.c does not look at
 *   use_trskip when it quantises.
 * Cost of a trial, in uint32_t arithmetic that wraps as C's does:
 *     cost = kvz_pixels_calc_ssd(source, trial rec) + coeff_cost * (uint32_t)bit_cost
 *     coeff_cost = (uint32_t)(sum * (qp * 0.044407704 + 0.557323653) + 0.5)                      (doubles, rdo.c:44-45, :219-220)
 *   sum = kvz_coeff_abs_sum of the trial's 16 coefficients; qp = state->qp of the TU's LCU, the luma QP and not the scaled one: the
 *   clamped lcu_qp value, or params->qp.  Every multiply and add rounds on its own, as on the host (no fused multiply-add).
 *   bit_cost = lcu_bit_cost[LCU] where the array is given (a negative value counts as 0), else ts->bit_cost.
 * Decision: the transformed trial wins ties (noskip.cost <= skip.cost, transform.c:260).  The winner's reconstruction, coefficients
 *   and has_coeffs become the TU's and feed cus[].cbf_y, cbf_out and costs exactly as the one trial of the _sl entry does: ssd_y and
 *   coeff_abs_y are the winner's, zero_ssd_y is against the prediction and does not change.  A winner without coefficients keeps
 *   the prediction and writes zeros.  In the intra entry a later TU reads the winner's pixels, as it reads any reconstruction.
 * tr_skip_out[scu] = 1 or 0 for every SCU covered by such a TU: what cur_pu->tr_skip holds at transform.c:387.  The bytes of all
 *   other SCUs are left untouched; the host clears the array once, as it does cbf_out.
 * Equals the reference where cfg.trskip_enable is set and state->qp < cfg.fast_residual_cost_limit (--fast-residual-cost N) holds
 *   for every LCU.  At or above the limit the reference prices coefficients with CABAC on the live context state
 *   (get_coeff_cabac_cost): kvz_hip_inter_residual_frame_ts_cabac and kvz_hip_intra_recon_frame_ts_cabac (below) are these entries
 *   with that rule, and kvz_hip_coeff_cost_batch is the count for any TU of the coefficient arrays they write.  OUT OF SCOPE: RDOQ
 *   and the transform-skip term of the intra rough search (search_intra.c:105-167).  Lossless coding switches transform skip off (encoder.c:623-628) and has entries of its own:
 *   kvz_hip_inter_residual_frame_lossless and kvz_hip_intra_recon_frame_lossless (below).  RDOQ is built since as a batch entry of its
 *   own, kvz_hip_rdoq_batch (further below); these stages do not call it.  The _rdoq entries further below do, without transform skip.
 * Errors: ts != NULL with tr_skip_out == NULL, with bit_cost < 0 while lcu_bit_cost == NULL, or with lcu_bit_cost not 4-byte
 *   aligned returns KVZ_HIP_ERR_INVALID and nothing is written; so does every error of the _sl entry.
 * Launches and capture: asynchronous, no allocation, no synchronisation with the host, usable between kvz_hip_graph_begin / _end.
 *   The launch shapes are those of the _sl entry: the same launch count, the same intra wavefront count.  A captured call may be
 *   replayed after the CONTENTS of lcu_bit_cost changed.  The ABI version stays 4. */
KVZ_HIP_API int kvz_hip_inter_residual_frame_ts(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                                kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                                kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v,
                                                uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp,
                                                const kvz_hip_scaling_tables *tables, const kvz_hip_trskip *ts, uint8_t *tr_skip_out,
                                                const kvz_hip_inter_residual_params *params, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_intra_recon_frame_ts(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                             kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                             const uint8_t *intra_modes, kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u,
                                             kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                             const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                             const kvz_hip_scaling_tables *tables, const kvz_hip_trskip *ts, uint8_t *tr_skip_out,
                                             const kvz_hip_inter_residual_params *params, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Coefficient pricing with CABAC: the counting coder                  */
/*   reference: get_coeff_cabac_cost (rdo.c:158-197), the branch of    */
/*   kvz_get_coeff_cost (rdo.c:208-222) at or above                    */
/*   cfg.fast_residual_cost_limit -- the default, the limit being 0    */
/*   (cfg.c:82) -- over kvz_encode_coeff_nxn in counting mode          */
/*   (encode_coding_tree.c:49-345) with context.c:303-385 and          */
/*   cabac.c:91-282                                                    */
/* ------------------------------------------------------------------ */
/* What the counting coder reads of state->cabac (cabac.h:41-88).  The count (23 - bits_left) + 8 * num_buffered_bytes is the number
 * of renormalisation shifts plus the number of bypass bins: a function of `range` and these context bytes, never of `low`.
 * range: cabac.range, 256..510.
 * ctx[0..135]: the 136 contiguous bytes of cabac_data_t.ctx from cu_sig_coeff_group_model[0] through cu_abs_model_chroma[1], in
 *   the reference's order (one memcpy from &cabac.ctx.cu_sig_coeff_group_model[0]); ctx[136] / ctx[137]:
 *   transform_skip_model_luma / _chroma; ctx[138..139]: spare, not read.
 * Bytes are uc_state (state << 1 | mps).  The result is specified for 0..125, the values the reference's coder produces; any other
 *   value is read as (value >> 1) & 63 for the state and cannot cause an access outside a table. */
typedef struct {
  uint16_t range;
  uint16_t reserved;
  uint8_t ctx[140];
} kvz_hip_coeff_ctx;            /* 144 bytes; DEVICE array, 2-byte aligned */

/* One TU of kvz_hip_coeff_cost_batch.
 * offset: in coefficients from `coeffs`, to width * width contiguous row-major values; a multiple of 4 (the reference reads four
 *   coefficients at a time).  A TU of the picture chain's coeff_y / coeff_u / coeff_v arrays is addressed by its z-order offset
 *   (LCU * 4096 or 1024 + 16 * z-order index of its first 4x4 block) unchanged.
 * width: 4 / 8 / 16 / 32.  type: 0 (luma) or 2 (chroma), the reference's `type`, which also indexes
 *   cu_sig_coeff_group_model[type].  scan_mode: 0 (diagonal), 1 (horizontal), 2 (vertical), 1 and 2 only at width <= 8:
 *   kvz_get_scan_order produces nothing else.  tr_skip: 0 / 1, the value of the transform_skip_flag bin that is coded at width 4
 *   with trskip_enable (kvz_get_coeff_cost passes 0, rdo.c:194).  ctx_index: the TU's set in ctx_sets. */
typedef struct {
  uint32_t offset;
  uint8_t width, type, scan_mode, tr_skip;
  uint32_t ctx_index;
} kvz_hip_coeff_cost_desc;      /* 12 bytes; DEVICE array, 4-byte aligned */

typedef struct {
  int32_t signhide;             /* cfg.signhide_enable */
  int32_t trskip_enable;        /* cfg.trskip_enable */
  int32_t lossless;             /* cfg.lossless: no sign is hidden (encode_coding_tree.c:261-262) */
  int32_t reserved;
} kvz_hip_coeff_cost_params;    /* 16 bytes; HOST struct, copied at the call */

/* bits_out[i] = get_coeff_cabac_cost of TU descs[i] (rdo.c:158-197): 0 when all its coefficients are zero, else the bits that
 * kvz_encode_coeff_nxn produces in counting mode, started from range and contexts of ctx_sets[descs[i].ctx_index].  A set is never
 * written: every TU is priced on a private copy, as the reference copies its state (rdo.c:177-178), so the result does not depend
 * on the order or the grouping of the descriptors.  Every branch that counting mode reaches is covered: the transform_skip_flag
 * bin, the last position's prefixes and suffixes with x and y swapped for the vertical scan, coded_sub_block_flag with its inferred
 * first and last cases, sig_coeff_flag with kvz_context_calc_pattern_sig_ctx / kvz_context_get_sig_ctx_inc and the inferred flag,
 * the greater-1 run with c1 and ctx_set, the one greater-2 flag, the signs with sign hiding, and kvz_cabac_write_coeff_remain with
 * the Rice parameter capped at 4.  The crypto branches are not reached in counting mode.
 * coeffs (8-byte aligned), descs, ctx_sets and bits_out (4-byte aligned) are DEVICE; params is HOST.
 * A descriptor outside the rules above, or with ctx_index >= n_sets, is skipped and its bits_out left untouched.
 * Errors (KVZ_HIP_ERR_INVALID, nothing written): a missing pointer with n > 0, n_sets == 0, a misaligned array, n above 2^31 - 1.
 *   n == 0 is KVZ_HIP_OK and nothing is looked at.
 * Launches and capture: two launches (the 4x4 TUs a lane each, the larger ones a wave each), asynchronous on s, no work memory,
 *   no allocation, no synchronisation with the host; usable between kvz_hip_graph_begin / _end, and a captured call may be
 *   replayed after the CONTENTS of coeffs, descs and ctx_sets changed.  The ABI version stays 4.
 * This is the coeff_bits term of kvz_cu_rd_cost_luma / _chroma (search.c:300, :369-370) as the reference computes it by default;
 *   the chain's coeff_abs_* sums are that term only under --fast-residual-cost.  OUT OF SCOPE: RDOQ (its lambda, error_scale and
 *   full state have no reachable reference entry), the transform-tree flag bits of the rd cost and the intra rough search's
 *   transform-skip term.  That sentence on RDOQ did not last: kvz_rdoq reads of its state only lambda, qp, the contexts, bitdepth,
 *   scaling_list and cfg.signhide_enable, a fabricated state reaches it, and RDOQ is now built as kvz_hip_rdoq_batch (further below),
 *   which reads this section's kvz_hip_coeff_ctx beside a kvz_hip_rdoq_state.
 * Any `range` and any context byte is memory-safe: range is used as (range >> 6) & 3 where it indexes, a byte as (byte >> 1) & 63.
 * Both launches run over the whole list whatever its mix and pass over the other class's descriptors, which costs a descriptor
 *   read each; a caller with many TUs of one class loses nothing by sorting them into calls of their own. */
KVZ_HIP_API int kvz_hip_coeff_cost_batch(const kvz_hip_coeff *coeffs, const kvz_hip_coeff_cost_desc *descs, size_t n,
                                         const kvz_hip_coeff_ctx *ctx_sets, uint32_t n_sets,
                                         const kvz_hip_coeff_cost_params *params, uint32_t *bits_out, kvz_hip_stream s);

/* How the two transform-skip stages price coefficients when the reference does it with CABAC.
 * ctx_sets: DEVICE, n_sets records, 2-byte aligned.  lcu_ctx: DEVICE, optional, 2-byte aligned: one set index per LCU in picture
 *   raster order; NULL means set 0 everywhere.  The search of an LCU runs on the state the previous LCU's coding left, so a set per
 *   LCU is the reference's granularity.  An index >= n_sets is used as n_sets - 1: nothing is read outside the table.
 * fast_limit: cfg.fast_residual_cost_limit (--fast-residual-cost N; 0 by default, cfg.c:82). */
typedef struct {
  const kvz_hip_coeff_ctx *ctx_sets;
  uint32_t n_sets;
  int32_t fast_limit;
  const uint16_t *lcu_ctx;
} kvz_hip_coeff_pricing;        /* 24 bytes; HOST struct, copied at the call */

/* kvz_hip_inter_residual_frame_ts and kvz_hip_intra_recon_frame_ts with one more argument, placed before params: the pricing rule of
 * kvz_get_coeff_cost (rdo.c:208-222) as the reference applies it inside kvz_quantize_residual_trskip (transform.c:229-276).
 * pricing == NULL: the call IS the _ts entry, byte for byte (it calls it, and that entry names itself in kvz_hip_last_error).
 * Otherwise everything of the _ts contract holds except coeff_cost of a trial, which becomes per TU the rule of rdo.c:214:
 *   if the QP of the TU's LCU (the clamped lcu_qp value, or params->qp) is >= fast_limit, coeff_cost is get_coeff_cabac_cost
 *   (rdo.c:158-197) of the trial's 16 coefficients -- the count kvz_hip_coeff_cost_batch returns -- on the LCU's set, with type 0,
 *   the TU's scan order (diagonal in the inter entry, kvz_get_scan_order of the intra mode in the intra entry), signhide from
 *   params, trskip_enable 1, lossless 0 and the transform_skip_flag bin 0 for BOTH trials (rdo.c:188-194 passes 0 whatever the
 *   trial is); a trial without coefficients costs 0 bits.  Otherwise coeff_cost is the estimate, as in the _ts entry.
 *   Cost, tie rule, winner, tr_skip_out, cbf, costs, launch count and capture rules are exactly the _ts entry's; a captured call
 *   may also be replayed after the CONTENTS of ctx_sets and lcu_ctx changed.
 * Errors beyond the _ts entry's (KVZ_HIP_ERR_INVALID, nothing written): pricing != NULL with ts == NULL, with ctx_sets == NULL or
 *   not 2-byte aligned, with n_sets == 0, or with a misaligned lcu_ctx.
 * The multi-picture _frames_ts entries take no pricing yet.  OUT OF SCOPE: RDOQ, the transform-tree flag bits of the rd cost and
 *   the transform-skip term of the intra rough search.  The ABI version stays 4.  RDOQ is built since as a batch entry of its own,
 *   kvz_hip_rdoq_batch (further below); these stages do not call it.  The _rdoq entries further below do, without
 *   transform skip. */
KVZ_HIP_API int kvz_hip_inter_residual_frame_ts_cabac(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                                      kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c,
                                                      kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u,
                                                      kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                                      const int8_t *lcu_qp, const kvz_hip_scaling_tables *tables,
                                                      const kvz_hip_trskip *ts, uint8_t *tr_skip_out,
                                                      const kvz_hip_coeff_pricing *pricing,
                                                      const kvz_hip_inter_residual_params *params, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_intra_recon_frame_ts_cabac(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                                   kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                                   const uint8_t *intra_modes, kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u,
                                                   kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                                   const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                                   const kvz_hip_scaling_tables *tables, const kvz_hip_trskip *ts, uint8_t *tr_skip_out,
                                                   const kvz_hip_coeff_pricing *pricing,
                                                   const kvz_hip_inter_residual_params *params, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Lossless coding in the picture chain: residual and intra stages     */
/*   reference: the `if (cfg->lossless)` branch of                     */
/*   quantize_tr_residual (transform.c:354-369) over bypass_transquant */
/*   (transform.c:73-100) and rdpcm (transform.c:109-123);             */
/*   intra_recon_tb_leaf (intra.c:590-638); --lossless,                */
/*   --implicit-rdpcm                                                  */
/* ------------------------------------------------------------------ */
typedef struct {
  int32_t chroma;          /* 0: 4:0:0 (U / V pointers unused), 1: 4:2:0 */
  int32_t implicit_rdpcm;  /* encoder->cfg.implicit_rdpcm */
  int32_t reserved[2];     /* must be 0 */
} kvz_hip_lossless;        /* 16 bytes; HOST struct, copied at the call */

/* kvz_hip_inter_residual_frame and kvz_hip_intra_recon_frame_tiles for a picture coded with --lossless (cfg.lossless): the same
 * arguments without params, lcu_qp, tables and transform skip -- there is no QP, no scaling table and no transform skip, because
 * nothing is transformed or quantised, and encoder.c:623-628 switches sign hiding, transform skip, deblocking and SAO off under
 * --lossless: the chain of a lossless picture is prediction -> these two entries.
 * The lossy entries set the rules and they hold here unchanged: argument meanings, the plane, alignment and stride rules (PLANES:
 *   any base alignment, any strides >= the widths; cus 4-byte aligned, the coefficient arrays 16-byte aligned), which CUs an entry
 *   owns (CU_INTER / CU_INTRA records with depth 0..3 whose CU lies inside the picture), the transform tree (tr_depth read from the
 *   map; chroma TUs half as wide, one 4x4 chroma TU per plane per 8x8 area under 4x4 luma TUs), the LCU coefficient layout, cus[].cbf_y,
 *   cbf_out and costs, and "everything that belongs to other records is left untouched".  No access leaves the planes or arrays,
 *   whatever the map holds.
 * kvz_hip_inter_residual_frame_lossless, per TU (bypass_transquant): coeff[x + y * w] = source - prediction, the w * w values at the
 *   TU's z-order slot in row-major order; rec = source; has_coeffs = any value non-zero.  rec_* hold the PREDICTION on entry, as for
 *   the lossy entry.  There is no RDPCM for inter CUs, whatever implicit_rdpcm says (transform.c:362: cur_pu->type == CU_INTRA).
 * kvz_hip_intra_recon_frame_lossless, per TU (intra_recon_tb_leaf, then the same bypass): the reference pixels as
 *   kvz_hip_intra_build_reference_batch defines them -- with a grid, by the tile rule of kvz_hip_intra_recon_frame_tiles -- TAKEN
 *   FROM THE SOURCE PLANE of that colour.  The rec planes on entry are never read, not even outside the intra CUs.  The reason: in
 *   the reference a lossless picture's reconstruction is its source (encoder_set_source_picture, encoderstate.c:1125-1127:
 *   rec = kvz_image_copy_ref(frame); bypass_transquant writes rec = ref for every TU), so every reference pixel an intra TU reads
 *   equals the source pixel at that place, whatever was coded before it, and availability follows position alone.  The stage has no
 *   dependency between TUs and no wavefront.  kvz_intra_predict runs with filter_boundary = luma && !implicit_rdpcm (intra.c:621);
 *   coeff = source - prediction, rec = source.  With implicit_rdpcm a TU whose mode is 10 gets horizontal DPCM, c[y][x] -= c[y][x - 1]
 *   for x >= 1, and a TU whose mode is 26 the vertical one, c[y][x] -= c[y - 1][x] for y >= 1 (transform.c:109-123; the reference walks
 *   from the bottom right, so every subtraction sees the unmodified neighbour).  "Mode" is the luma byte of intra_modes for a luma TU
 *   and the chroma byte for a chroma TU (transform.c:315-316): a chroma TU in mode 10 or 26 gets DPCM too.  The reference takes
 *   has_coeffs before the DPCM; DPCM is invertible, so that equals "any STORED value non-zero".  A TU whose mode is above 34 is skipped:
 *   nothing is written for it, its cbf_out bit is 0 and it adds nothing to the costs.
 * costs, both entries: ssd_* = 0 (the reconstruction is the source); zero_ssd_* = the SSD of the source against the prediction;
 *   coeff_abs_* = the sum of |coeff| as stored, i.e. after DPCM.  search.c:580 does not apply the zero-coefficient alternative
 *   (cu_zero_coeff_cost) under lossless: zero_ssd_* is there for the caller's own use.  Integer sums: the result does not depend on
 *   scheduling.
 * cbf_out: the bytes of the owned CUs' SCUs are SET, as by the lossy entries, but with one plain byte store each: the workgroup that
 *   owns an LCU owns all three planes of it, so no dword around the array is touched and cbf_out may have any alignment.
 * tiles (intra entry): may be NULL = one tile, the whole picture, byte for byte.  The inter entry does not depend on tiles.
 * Launches: each entry is ONE kernel launch, Y, U and V together, whatever the picture size, the grid and the map hold: a workgroup
 *   per LCU.  Asynchronous on s, no host synchronisation, no allocation, no workspace; usable between kvz_hip_graph_begin / _end, and a
 *   captured call may be replayed after the CONTENTS of cus, intra_modes, the source and the planes changed.
 * Errors: a NULL ll, a non-zero reserved field, a missing required pointer (intra_modes included, and U / V with chroma = 1), a
 *   misaligned cus or coefficient array, a size that is not a multiple of 8, a stride below the width or an invalid tile grid returns
 *   KVZ_HIP_ERR_INVALID and nothing is written.
 * OUT OF SCOPE: the search side of implicit_rdpcm (search_intra.c:419), PCM, bit depths above 8.  The ABI version stays 4. */
KVZ_HIP_API int kvz_hip_inter_residual_frame_lossless(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                                      kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c,
                                                      kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u,
                                                      kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                                      const kvz_hip_lossless *ll, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_intra_recon_frame_lossless(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y,
                                                   kvz_hip_pixel *rec_u, kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus,
                                                   const uint8_t *intra_modes, kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u,
                                                   kvz_hip_coeff *coeff_v, uint8_t *cbf_out, kvz_hip_inter_residual_cost *costs,
                                                   const kvz_hip_tile_grid *tiles, const kvz_hip_lossless *ll, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Rate-distortion optimised quantisation (RDOQ) of a list of TUs      */
/*   reference: kvz_rdoq (rdo.c:548-881) with kvz_get_ic_rate          */
/*   (rdo.c:233-278), kvz_get_coded_level (rdo.c:297-339),             */
/*   get_rate_last / calc_last_bits (rdo.c:350-395) and                */
/*   kvz_rdoq_sign_hiding (rdo.c:405-539), as kvz_quantize_residual    */
/*   calls it under cfg.rdoq_enable (quant-generic.c:214-221); the     */
/*   error scale of kvz_scalinglist_process (scalinglist.c:339-356);   */
/*   --rdoq, on at preset medium and slower                            */
/* ------------------------------------------------------------------ */
/* The two tables RDOQ reads per coefficient, as DEVICE arrays of KVZ_HIP_SL_TABLE_LEN values in the layout of
 * kvz_hip_scaling_tables: table (size_id, list, rem) at 36 * {0, 16, 80, 336}[size_id] + (6 * list + rem) * N * N.
 * quant: scaling_list.quant_coeff, 16-byte aligned -- the array kvz_hip_scaling_tables_pack already produces.
 * err_scale: scaling_list.error_scale, the encoder's own doubles (scalinglist.c:339-356), 8-byte aligned.
 * RDOQ reads both for flat lists too (rdo.c:563-564), so the tables are always required. */
typedef struct { const int32_t *quant; const double *err_scale; } kvz_hip_rdoq_tables;   /* 16 bytes; HOST struct, copied at the call */

/* Host only: needs no device and no kvz_hip_init.  Copies scaling_list.quant_coeff and scaling_list.error_scale
 * ([size_id][list][rem]) into two HOST arrays of KVZ_HIP_SL_TABLE_LEN values in the layout above; quant_out equals what
 * kvz_hip_scaling_tables_pack writes.  The size-3 rule of that function holds: lists 0, 1 and 3 are read, the tables of lists 2, 4
 * and 5 are filled with zeros.  A NULL argument or a NULL source pointer elsewhere returns KVZ_HIP_ERR_INVALID. */
KVZ_HIP_API int kvz_hip_rdoq_tables_pack(const int32_t *const quant_coeff[4][6][6], const double *const error_scale[4][6][6],
                                         int32_t *quant_out, double *err_out);

/* What kvz_rdoq reads of the encoder state beyond the 136 context bytes of kvz_hip_coeff_ctx: one record per context set,
 * index-parallel to the kvz_hip_coeff_ctx array (`range` and the transform-skip bytes of that record are not read).
 * lambda: state->lambda, finite and above 0: the result is specified for such values alone (the reference divides by it, rdo.c:420-421).
 *   Any other value -- zero, negative, infinite, NaN -- is memory-safe, because nothing is indexed with a cost, but what dest receives is
 *   then unspecified.  qp: state->qp, 0..51; a TU whose record holds another value is skipped.
 * root_cbf: cabac.ctx.cu_qt_root_cbf_model; qt_cbf_luma / qt_cbf_chroma: cabac.ctx.qt_cbf_model_luma / _chroma (cabac.h:61-62, :84).
 * A context byte, here and in kvz_hip_coeff_ctx, is read as (byte >> 1) & 63 for the state and byte & 1 for the MPS, like the
 *   counting coder: no value can index outside a table. */
typedef struct {
  double lambda;
  int8_t qp;
  uint8_t root_cbf;
  uint8_t qt_cbf_luma[4];
  uint8_t qt_cbf_chroma[4];
  uint8_t reserved[6];
} kvz_hip_rdoq_state;           /* 24 bytes; DEVICE array, 8-byte aligned */

/* One TU of kvz_hip_rdoq_batch.
 * src_offset / dst_offset: in coefficients from `coef` / `dest`, to width * width contiguous row-major values; multiples of 4.  A TU
 *   of the picture chain's coefficient arrays is addressed by its z-order offset unchanged (see kvz_hip_coeff_cost_desc).
 * width: 4 / 8 / 16 / 32.  type: 0 (luma) or 2 (chroma).  scan_mode: 0..2, 1 and 2 only at width <= 8.
 * block_type: 1 = CU_INTRA, 2 = CU_INTER (cu.h:39-41).  tr_depth: 0..3, the depth kvz_quantize_residual hands to kvz_rdoq.
 * ctx_index: the TU's record in ctx_sets and in states; 16 bits, as the set indices of kvz_hip_coeff_pricing.lcu_ctx are, which
 *   keeps the record at 16 bytes. */
typedef struct {
  uint32_t src_offset;
  uint32_t dst_offset;
  uint8_t width, type, scan_mode, block_type;
  uint8_t tr_depth;
  uint8_t reserved;
  uint16_t ctx_index;
} kvz_hip_rdoq_desc;            /* 16 bytes; DEVICE array, 4-byte aligned */

typedef struct {
  int32_t signhide;             /* cfg.signhide_enable */
  int32_t reserved[3];
} kvz_hip_rdoq_params;          /* 16 bytes; HOST struct, copied at the call */

/* dest at descs[i].dst_offset receives exactly what kvz_rdoq (rdo.c:548-881) leaves in dest_coeff for the TU at descs[i].src_offset:
 * bit depth 8, state->qp, state->lambda and the contexts of record ctx_index, and the tables of (log2 N - 2,
 * (block_type == CU_INTRA ? 0 : 3) + (type ? 1 : 0), qp_scaled % 6) with qp_scaled = kvz_get_scaled_qp(type, qp, 0).  All N * N
 * values are written: the reference's first loop zeroes everything behind the last position it finds, and an all-zero TU comes
 * out all zero.  coef and dest must not overlap.
 * Arithmetic: every cost is an IEEE binary64 value computed in the reference's operation order, each multiplication, addition and
 *   division rounded on its own (no fused multiply-add: the reference's object code holds none); block_uncoded_cost and base_cost
 *   are summed in scan order by one lane.  |coef| * q is taken as a 64-bit product and then clamped as at rdo.c:629, which equals
 *   the reference wherever its int32 product is defined.
 * Covered: kvz_get_coded_level over max_abs_level and max_abs_level - 1, kvz_get_ic_rate with its escape-code loop, the c1 / c2 /
 *   ctx_set / Rice-parameter updates, the zeroing of coefficient groups (rdo.c:759-812), the last-position search (:815-864) with
 *   the root-cbf branch for inter luma and the qt-cbf branch otherwise, x and y swapped for the vertical scan, the clean-up
 *   (:866-876), and kvz_rdoq_sign_hiding when params->signhide and abs_sum >= 2.  Context sets are never written: kvz_rdoq prices
 *   with them and updates none, so the result does not depend on the order or the grouping of the descriptors.
 * coef and dest (8-byte aligned), descs (4-byte aligned), ctx_sets (2-byte aligned) and states (8-byte aligned) are DEVICE, and so
 *   are the two arrays of tables; tables and params are HOST.
 * A descriptor outside the rules above, with ctx_index >= n_sets, or whose state holds a qp outside 0..51, is skipped and its dest is
 *   left untouched.
 * Errors (KVZ_HIP_ERR_INVALID, nothing written): a missing pointer with n > 0 (the pointers inside tables included), n_sets == 0, a
 *   misaligned array, n above 2^31 - 1.  n == 0 is KVZ_HIP_OK and nothing is looked at.
 * Launches and capture: two launches (the 4x4 TUs a lane each, the larger ones a wave each), asynchronous on s, no work memory, no
 *   allocation, no synchronisation with the host; usable between kvz_hip_graph_begin / _end, and a captured call may be replayed
 *   after the CONTENTS of coef, descs, ctx_sets, states and the tables changed.  The ABI version stays 4.
 * This is a batch entry of its own, as kvz_hip_coeff_cost_batch was before its stages.  OUT OF SCOPE: RDOQ inside the _ts /
 *   _frames_ts stages of the picture chain, RDOQ in the drop-in's quantize_residual (it needs the live CABAC state through an
 *   accessor and keeps calling the host's kvz_rdoq), bit depths above 8. */
KVZ_HIP_API int kvz_hip_rdoq_batch(const kvz_hip_coeff *coef, kvz_hip_coeff *dest, const kvz_hip_rdoq_desc *descs, size_t n,
                                   const kvz_hip_coeff_ctx *ctx_sets, const kvz_hip_rdoq_state *states, uint32_t n_sets,
                                   const kvz_hip_rdoq_tables *tables, const kvz_hip_rdoq_params *params, kvz_hip_stream s);

/* ---- RDOQ inside the two single-picture residual stages of the picture chain ----
 * kvz_quantize_residual calls kvz_rdoq instead of kvz_quant where cfg.rdoq_enable && (width > 4 || !cfg.rdoq_skip)
 * (quant-generic.c:214-221): every TU at preset medium and slower.  What the two entries below read for that, beside the arguments of
 * the _sl entries.  Offsets in front of the fields.
 * ctx_sets / states: the context sets and, index-parallel to them, the states (lambda and the nine cbf context bytes).  states[].qp is
 *   NOT read by these entries: a TU is handed the QP of its LCU, exactly the value the _sl entry quantises that TU with.
 * lcu_ctx: one set index per LCU in raster order, or NULL: set 0 everywhere.  An index >= n_sets is used as n_sets - 1, the rule of
 *   kvz_hip_coeff_pricing.
 * tables: quant and err_scale as kvz_hip_rdoq_tables_pack lays them out; RDOQ reads both for flat lists too, so they are always
 *   required.  rdoq_skip: cfg.rdoq_skip -- the 4x4 TUs keep the plain quantiser. */
typedef struct {
  const kvz_hip_coeff_ctx  *ctx_sets;   /*  0: DEVICE, n_sets records, 2-byte aligned */
  const kvz_hip_rdoq_state *states;     /*  8: DEVICE, n_sets records, 8-byte aligned, index-parallel to ctx_sets */
  const uint16_t           *lcu_ctx;    /* 16: DEVICE, optional: one set index per LCU, raster order; NULL = set 0 */
  kvz_hip_rdoq_tables       tables;     /* 24: quant + err_scale, DEVICE, as kvz_hip_rdoq_tables_pack lays them out; always required */
  uint32_t                  n_sets;     /* 40: the records in ctx_sets and in states */
  int32_t                   rdoq_skip;  /* 44: cfg.rdoq_skip: 4x4 TUs keep the plain quantiser */
} kvz_hip_rdoq_source;          /* 48 bytes; HOST struct, copied at the call */

/* kvz_hip_inter_residual_frame_sl and kvz_hip_intra_recon_frame_sl with `rdoq` placed before params.
 * rdoq == NULL: the call is the _sl entry, byte for byte; it calls that entry, which then names itself in kvz_hip_last_error.
 * Otherwise everything of the _sl contract holds -- lcu_qp, the optional tables, tiles in the intra entry, which CUs are owned, the
 *   transform tree, the LCU coefficient layout, cbf_y, cbf_out, costs, and nothing outside the owned records is touched -- and only the
 *   quantiser of a TU changes: where width > 4 || !rdoq_skip its levels are what kvz_rdoq leaves, as kvz_hip_rdoq_batch defines them;
 *   every other TU takes the _sl quantiser with its own sign hiding.
 * What kvz_rdoq is handed: type 0 for Y and 2 for U and V; scan_mode the TU's scan order (diagonal in the inter entry,
 *   kvz_get_scan_order of the intra mode in the intra entry); block_type from the CU (CU_INTER / CU_INTRA); qp the QP of the TU's LCU;
 *   lambda, the nine cbf context bytes and the contexts from states[set] and ctx_sets[set] with set = lcu_ctx[lcu]; signhide from
 *   params; the quant and error-scale tables from rdoq->tables.  The optional `tables` argument keeps its _sl meaning: it serves
 *   dequantisation and the plain quantiser of the skipped 4x4 TUs.
 * tr_depth: tr_depth - depth + (part_size == SIZE_NxN ? 1 : 0) of the record at the TU's own top-left SCU (the cur_pu of
 *   transform.c:437; quant-generic.c:218-219), clamped into 0..3 so that no map can index outside qt_cbf_model_chroma[4]; a reference
 *   encode never leaves that range.
 * After the levels, as quant-generic.c:227-270: has_coeffs is set when any level is non-zero; dequantisation, inverse transform,
 *   reconstruction and clipping run only then, otherwise the prediction stands; ssd_*, zero_ssd_* and coeff_abs_* keep their
 *   definitions, taken over the RDOQ levels.
 * Errors beyond the _sl entry's (KVZ_HIP_ERR_INVALID, nothing written): ctx_sets, states, tables.quant or tables.err_scale NULL;
 *   n_sets == 0; ctx_sets or lcu_ctx not 2-byte aligned; states or err_scale not 8-byte aligned; quant not 16-byte aligned.
 * Any lambda, context byte or table value is memory-safe, as in the batch entry; the result is specified for finite lambda > 0 only.
 * Launches: asynchronous on s, no allocation, no workspace, no host synchronisation.  The inter entry: the init launch of the _sl
 *   entry (with cbf_out or costs) and four launches, one per TU width, a wave per TU (with rdoq_skip the 4x4 launch is the _sl
 *   entry's).  The intra entry: the launches of the _sl entry, one per step of the wavefront, a wave per LCU and plane; the serial
 *   recursion of kvz_rdoq runs on one lane inside every step.  Launch shapes depend on the sizes only, and in the intra entry on the
 *   grid.  Usable between kvz_hip_graph_begin / _end; a captured call may be replayed after the CONTENTS of every array changed.
 *   The ABI version stays 4.
 * OUT OF SCOPE: transform skip together with RDOQ (these entries take no kvz_hip_trskip), the multi-picture _frames / _frames_ts
 *   entries, the drop-in's quantize_residual, lossless, bit depths above 8, a recursion on more than one lane.  Since then the
 *   multi-picture form exists as entries of its own: the _frames_rdoq entries further below. */
KVZ_HIP_API int kvz_hip_inter_residual_frame_rdoq(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                                  kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, kvz_hip_coeff *coeff_y,
                                                  kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                                  kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp, const kvz_hip_scaling_tables *tables,
                                                  const kvz_hip_rdoq_source *rdoq, const kvz_hip_inter_residual_params *params, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_intra_recon_frame_rdoq(const kvz_hip_ref_picture *src, kvz_hip_pixel *rec_y, uint32_t stride_y, kvz_hip_pixel *rec_u,
                                               kvz_hip_pixel *rec_v, uint32_t stride_c, kvz_hip_cu_info *cus, const uint8_t *intra_modes,
                                               kvz_hip_coeff *coeff_y, kvz_hip_coeff *coeff_u, kvz_hip_coeff *coeff_v, uint8_t *cbf_out,
                                               kvz_hip_inter_residual_cost *costs, const int8_t *lcu_qp, const kvz_hip_tile_grid *grid,
                                               const kvz_hip_scaling_tables *tables, const kvz_hip_rdoq_source *rdoq,
                                               const kvz_hip_inter_residual_params *params, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Several independent pictures through the residual stages at once    */
/*   reference: the pictures the encoder keeps in flight (--owf):      */
/*   every picture under --period 1, the pictures of the highest       */
/*   temporal layer of a GOP 8                                         */
/* ------------------------------------------------------------------ */
#define KVZ_HIP_MAX_CHAIN_PICTURES 16
/* One picture of a multi-picture call: the arguments of kvz_hip_inter_residual_frame_qp / kvz_hip_intra_recon_frame_qp as a record.
 * Every pointer in it is DEVICE memory; the record itself is HOST memory, copied at the call.  Offsets in front of the fields. */
typedef struct {
  kvz_hip_ref_picture src;              /*   0: the source picture; its width / height are the picture's */
  kvz_hip_pixel *rec_y, *rec_u, *rec_v; /*  40, 48, 56 */
  uint32_t stride_y, stride_c;          /*  64, 68 */
  kvz_hip_cu_info *cus;                 /*  72 */
  const uint8_t *intra_modes;           /*  80: read by kvz_hip_intra_recon_frames only; kvz_hip_inter_residual_frames ignores it */
  kvz_hip_coeff *coeff_y, *coeff_u, *coeff_v;   /* 88, 96, 104 */
  uint8_t *cbf_out;                     /* 112: optional */
  kvz_hip_inter_residual_cost *costs;   /* 120: optional */
  const int8_t *lcu_qp;                 /* 128: optional; NULL = params.qp in every LCU */
  kvz_hip_inter_residual_params params; /* 136: qp, slice_is_intra, signhide, scaling_list (must be 0), chroma */
} kvz_hip_chain_picture;                /* 160 bytes */
/* kvz_hip_inter_residual_frame_qp and kvz_hip_intra_recon_frame_qp for n_pictures (0..KVZ_HIP_MAX_CHAIN_PICTURES) pictures that do not
 * depend on each other, in one asynchronous call.  A launch of the single-picture intra entry is one wave per LCU row and plane -- 51
 * waves at 1080p -- and the launches of one picture depend on each other; independent pictures share the launches instead, as the
 * tiles of one picture do in kvz_hip_intra_recon_frame_tiles.
 * THE RULE: for every picture i and every output array, the result is byte for byte what kvz_hip_inter_residual_frame_qp /
 *   kvz_hip_intra_recon_frame_qp leaves when called with the fields of pictures[i] -- lcu_qp == NULL included, which means that
 *   picture's params.qp in every LCU (not clamped, as in the one-QP entries; the values of an array are clamped into 0..51).
 *   Everything those entries define holds per picture: which CUs are handled and the transform tree, scans and sign hiding, the
 *   coefficient layout, cbf_y written back into cus, cbf_out and costs, the alignment and stride rules, and "everything that belongs
 *   to other records is left untouched".  Pictures of one call may differ in size, chroma format (4:0:0 next to 4:2:0), QP, signhide
 *   and slice_is_intra, and in whether they carry lcu_qp, cbf_out and costs.
 * Independence is the caller's promise: no output of one record may be an input or an output of another; sources may be shared.
 *   Records whose rec_y, cus or coeff_y base pointers coincide are refused.  Any other overlap is a caller error with unspecified
 *   output, but no access leaves a record's own arrays.
 * Errors: n_pictures == 0 is a no-op that returns KVZ_HIP_OK (pictures may then be NULL).  KVZ_HIP_ERR_INVALID: n_pictures below 0 or
 *   above KVZ_HIP_MAX_CHAIN_PICTURES, pictures == NULL, or any record that the single-picture entry would refuse -- a missing pointer,
 *   a misaligned cus / coefficient / costs array, a bad size or stride, scaling_list != 0, a negative params.qp without lcu_qp.  Every
 *   record is checked before anything is launched: on refusal nothing is written for any picture, and kvz_hip_last_error() names the
 *   index of the offending record ("picture 2").
 * Execution: asynchronous on s; no host synchronisation, no allocation, no workspace -- the call owns no device buffer; the records
 *   travel in the kernel arguments (152 / 136 bytes per picture) and a workgroup reads its own with scalar loads.  Usable between
 *   kvz_hip_graph_begin / _end.  The launch shapes depend only on the sizes, the chroma flags and the presence of cbf_out / costs: a
 *   captured call may be replayed after the CONTENTS of every device array changed.
 * Launches: kvz_hip_intra_recon_frames makes max over the pictures of ceil(width / 64) + 2 (ceil(height / 64) - 1) wavefront launches,
 *   plus one init launch if any picture has cbf_out or costs; launch t holds wave t of every picture.  kvz_hip_inter_residual_frames
 *   makes the single entry's launches (one per transform size, plus the init launch), each covering all pictures.
 * LEFT OUT ON PURPOSE: pictures with tiles, scaling lists or transform skip and pictures coded with --lossless stay with their
 *   single-picture entries (_tiles, _sl, _ts, _lossless) -- for tiles, scaling lists and transform skip see kvz_hip_*_frames_ts
 *   below, which take them.  Behind these two stages, the QP map, deblocking and SAO of several pictures are kvz_hip_cu_qp_frames,
 *   kvz_hip_deblock_frames, kvz_hip_sao_stats_frames and kvz_hip_sao_frames further below.  Prediction of several pictures
 *   (kvz_hip_inter_recon_frame) is
 *   kvz_hip_inter_recon_frames at the end of these sections: sixteen tables of reference pictures do not fit the kernel arguments,
 *   so its records index one shared pool of reference pictures (see there).  The ABI version stays 4. */
KVZ_HIP_API int kvz_hip_inter_residual_frames(const kvz_hip_chain_picture *pictures, int n_pictures, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_intra_recon_frames(const kvz_hip_chain_picture *pictures, int n_pictures, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Several independent pictures with tiles, scaling lists and          */
/*   transform skip through the residual stages at once                */
/*   reference: the pictures in flight (--owf) of an encode run with   */
/*   --tiles, --scaling-list / --cqmfile or --transform-skip           */
/* ------------------------------------------------------------------ */
/* The tile boundaries of the records of one call travel in the kernel arguments, packed into one shared pool of this many 16-bit
 * values: the sum of cols + rows + 2 over the records that carry a grid must not exceed it.  Sixteen pictures of 7 x 7 tiles use all
 * of it, fourteen pictures of 8 x 8 tiles 252; records and pool together stay below the 4 KB that a kernel's arguments may take. */
#define KVZ_HIP_CHAIN_TILE_BOUNDS 256
/* One picture of kvz_hip_*_frames_ts: the arguments of kvz_hip_inter_residual_frame_ts / kvz_hip_intra_recon_frame_ts as a record.
 * The record is HOST memory, copied at the call, and so is what grid and ts point to.  Offsets in front of the fields. */
typedef struct {
  kvz_hip_chain_picture pic;        /*   0: as for kvz_hip_*_frames; pic.params.scaling_list != 0 exactly when tables are given */
  const kvz_hip_tile_grid *grid;    /* 160: HOST, optional, copied at the call; NULL = one tile.  Read by the intra entry only */
  kvz_hip_scaling_tables tables;    /* 168: both NULL = flat lists; else both DEVICE, non-NULL, 16-byte aligned */
  const kvz_hip_trskip *ts;         /* 184: HOST, optional, copied at the call; NULL = no transform skip */
  uint8_t *tr_skip_out;             /* 192: DEVICE, one byte per SCU; required with ts, not touched without */
} kvz_hip_chain_picture_ts;         /* 200 bytes */
/* kvz_hip_inter_residual_frame_ts and kvz_hip_intra_recon_frame_ts for n_pictures (0..KVZ_HIP_MAX_CHAIN_PICTURES) pictures that do
 * not depend on each other, in one asynchronous call: the wavefronts of all tiles of all pictures share the launches of the intra stage.
 * THE RULE: for every picture i and every output array (the rec planes, the coefficients, cus[].cbf_y, cbf_out, costs, tr_skip_out),
 *   the result is byte for byte what kvz_hip_inter_residual_frame_ts / kvz_hip_intra_recon_frame_ts leaves when called with the fields
 *   of pictures[i].  Everything those entries define holds per picture: the tile rule for an intra TU's neighbours, the tables a TU
 *   takes, the two trials of a 4x4 luma TU and their price, the clamping of lcu_qp, which bytes of tr_skip_out are written.  Pictures
 *   of one call may differ in size, chroma format, QP, signhide and slice_is_intra; in their tile grid, tiled pictures beside untiled
 *   ones included; in whether they carry lcu_qp, lcu_bit_cost, cbf_out and costs; and in which tables they point to.
 * ONE RESTRICTION: a call is homogeneous in the two options that select a kernel instantiation.  Either every record carries tables
 *   or none does; either every record carries ts or none does (both are encoder-wide settings: --scaling-list, --transform-skip).  A
 *   record that differs from record 0 in either is refused.  Tiles are no such option: a record with grid == NULL stands beside
 *   tiled ones.
 * No options at all: when no record carries tables or ts -- and, for the intra entry, no record carries a grid -- the call IS
 *   kvz_hip_inter_residual_frames / kvz_hip_intra_recon_frames on the embedded records, byte for byte (it calls it, and that entry
 *   names itself in kvz_hip_last_error).
 * Independence is the caller's promise, as for kvz_hip_*_frames.  Records whose rec_y, cus, coeff_y or (with ts) tr_skip_out base
 *   pointers coincide are refused; tables, lcu_qp and lcu_bit_cost are inputs and may be shared.
 * Errors: those of kvz_hip_*_frames (n_pictures == 0 is a no-op), and per record what the _ts single entry refuses: an invalid grid
 *   (intra entry); ts without tr_skip_out; a negative bit_cost without lcu_bit_cost; a lcu_bit_cost that is not 4-byte aligned; one
 *   table NULL or not 16-byte aligned; pic.params.scaling_list != 0 without tables or 0 with them; a negative params.qp without lcu_qp.
 *   Also: the homogeneity rule; shared outputs; and (intra entry) a record whose grid no longer fits the pool of
 *   KVZ_HIP_CHAIN_TILE_BOUNDS boundaries.  Every record is checked before anything is launched: a refusal returns
 *   KVZ_HIP_ERR_INVALID, writes nothing for any picture, and kvz_hip_last_error() names the record's index ("picture 2") -- for the
 *   pool, the record at which it overflowed.
 * Execution: asynchronous on s; no host synchronisation, no allocation, no workspace -- the call owns no device buffer.  The records
 *   (200 / 176 bytes per picture) and the pool travel in the kernel arguments and are read with scalar loads.  Usable between
 *   kvz_hip_graph_begin / _end.  The launch shapes depend only on the sizes, the chroma flags, the grids and the presence of cbf_out /
 *   costs: a captured call may be replayed after the CONTENTS of every device array changed.
 * Launches: kvz_hip_intra_recon_frames_ts makes max over the pictures of (max over the picture's tiles of w_t + 2 (h_t - 1)) wavefront
 *   launches, w_t x h_t the tile in LCUs, plus one init launch if any picture has cbf_out or costs.  kvz_hip_inter_residual_frames_ts
 *   makes the single entry's launches (one per transform size, plus the init launch), each covering all pictures.
 * LEFT OUT ON PURPOSE: a call that mixes pictures with and without tables, or with and without ts (a kernel that takes both paths at
 *   run time would carry the code of both); pictures coded with --lossless (one launch each already); prediction of several
 *   pictures (the QP map, deblocking and SAO of several pictures are kvz_hip_cu_qp_frames, kvz_hip_deblock_frames,
 *   kvz_hip_sao_stats_frames and kvz_hip_sao_frames below) in these entries -- it is an entry of its own,
 *   kvz_hip_inter_recon_frames further below; RDOQ.  The ABI version stays 4.  (RDOQ exists as the batch entry kvz_hip_rdoq_batch,
 *   above; inside these stages it is still to come.)  Since then it came, as entries of their own: the _frames_rdoq entries below. */
KVZ_HIP_API int kvz_hip_inter_residual_frames_ts(const kvz_hip_chain_picture_ts *pictures, int n_pictures, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_intra_recon_frames_ts(const kvz_hip_chain_picture_ts *pictures, int n_pictures, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Several independent pictures with RDOQ through the residual stages  */
/*   reference: the pictures in flight (--owf) of an encode at preset  */
/*   medium and slower, where cfg.rdoq_enable is set                   */
/* ------------------------------------------------------------------ */
/* One picture of kvz_hip_*_frames_rdoq: the arguments of kvz_hip_inter_residual_frame_rdoq / kvz_hip_intra_recon_frame_rdoq as a
 * record.  The record is HOST memory, copied at the call, and so is what grid and rdoq point to.  Offsets in front of the fields. */
typedef struct {
  kvz_hip_chain_picture pic;          /*   0: as for kvz_hip_*_frames; pic.params.scaling_list != 0 exactly when tables are given */
  const kvz_hip_tile_grid *grid;      /* 160: HOST, optional, copied at the call; NULL = one tile.  Read by the intra entry only */
  kvz_hip_scaling_tables tables;      /* 168: both NULL = flat lists; else both DEVICE, non-NULL, 16-byte aligned */
  const kvz_hip_rdoq_source *rdoq;    /* 184: HOST, copied at the call; what it points to is DEVICE memory */
} kvz_hip_chain_picture_rdoq;         /* 192 bytes */
/* kvz_hip_inter_residual_frame_rdoq and kvz_hip_intra_recon_frame_rdoq for n_pictures (0..KVZ_HIP_MAX_CHAIN_PICTURES) pictures that do
 * not depend on each other, in one asynchronous call.  With RDOQ the serial recursion of kvz_rdoq runs on one lane inside every step
 * of the intra wavefront, and a launch of one picture leaves the rest of the device idle for that time: pictures in flight fill it.
 * THE RULE: for every picture i and every output array (the rec planes, the coefficients, cus[].cbf_y, cbf_out, costs), the result is
 *   byte for byte what kvz_hip_inter_residual_frame_rdoq / kvz_hip_intra_recon_frame_rdoq leaves when called with the fields of
 *   pictures[i].  Everything those entries define holds per picture: which TUs take kvz_rdoq and which keep the plain quantiser; the
 *   context set of the TU's LCU, an index >= n_sets used as n_sets - 1; tr_depth from the record at the TU's own top-left SCU; the QP
 *   of the LCU; sign hiding; the tile rule for an intra TU's neighbours; the tables a TU takes.  Pictures of one call may differ in
 *   size, chroma format (4:0:0 beside 4:2:0), QP, signhide and slice_is_intra; in their tile grid, tiled pictures beside untiled ones
 *   included; in whether they carry lcu_qp, cbf_out and costs; in which scaling tables they point to; and in their ctx_sets, states,
 *   lcu_ctx and n_sets: every picture has its own CABAC contexts and lambdas.
 * ONE RESTRICTION: a call is homogeneous, after the model of kvz_hip_*_frames_ts.  Either every record carries tables or none does;
 *   either every record carries rdoq or none does; and every record's rdoq->rdoq_skip, rdoq->tables.quant and rdoq->tables.err_scale
 *   equal those of record 0.  All of them are encoder-wide (--scaling-list, --rdoq, --rdoq-skip, the lists the tables were packed
 *   from).  The options select the kernel instantiation -- rdoq_skip also which 4x4 kernel the inter entry launches -- and the RDOQ
 *   tables travel once per call because a pair of pointers per record would pass the 4 KB that a kernel's arguments may take.  A
 *   record that differs from record 0 is refused.
 * No rdoq at all: when no record carries rdoq, the call IS kvz_hip_inter_residual_frames_ts / kvz_hip_intra_recon_frames_ts on the
 *   same fields with ts == NULL, byte for byte (it calls it, and that entry names itself in kvz_hip_last_error).
 * Independence is the caller's promise, as for kvz_hip_*_frames.  Records whose rec_y, cus or coeff_y base pointers coincide are
 *   refused; the tables, lcu_qp and everything rdoq points to are inputs and may be shared.
 * Errors: those of kvz_hip_*_frames_ts (n_pictures == 0 is a no-op), and per record what the _rdoq single entry refuses: ctx_sets,
 *   states, tables.quant or tables.err_scale NULL; n_sets == 0; ctx_sets or lcu_ctx not 2-byte aligned; states or err_scale not 8-byte
 *   aligned; quant not 16-byte aligned.  Also: the homogeneity rule; shared outputs; and (intra entry) a record whose grid no longer
 *   fits the pool of KVZ_HIP_CHAIN_TILE_BOUNDS boundaries.  The order per record: homogeneity, the record's own checks, its grid and
 *   the grid's place in the pool, the outputs of the earlier records.  Every record is checked before anything is launched: a
 *   refusal returns KVZ_HIP_ERR_INVALID, writes nothing for any picture, and kvz_hip_last_error() names the record's index
 *   ("picture 2") -- for the pool, the record at which it overflowed.
 * Execution: asynchronous on s; no host synchronisation, no allocation, no workspace -- the call owns no device buffer.  The records
 *   (208 / 184 bytes per picture), the pool and the shared RDOQ tables travel in the kernel arguments and are read with scalar
 *   loads.  Usable between kvz_hip_graph_begin / _end.  The launch shapes depend only on the sizes, the chroma flags, the grids,
 *   rdoq_skip and the presence of cbf_out / costs: a captured call may be replayed after the CONTENTS of every device array changed,
 *   the context sets and states included.
 * Launches: kvz_hip_intra_recon_frames_rdoq makes the wavefront launches of kvz_hip_intra_recon_frames_ts -- max over the pictures of
 *   (max over the picture's tiles of w_t + 2 (h_t - 1)) -- plus one init launch if any picture has cbf_out or costs; a wave per LCU
 *   and plane.  kvz_hip_inter_residual_frames_rdoq makes the init launch and one launch per TU width, each covering all pictures,
 *   a wave per TU; with rdoq_skip the 4x4 launch is that of kvz_hip_inter_residual_frames_ts.
 * OUT OF SCOPE: transform skip together with RDOQ (the record has no ts), a call that mixes pictures with and without rdoq or with
 *   different RDOQ tables, the drop-in's quantize_residual, lossless, bit depths above 8, a recursion on more than one lane.  The
 *   single-picture entries and every older kernel are unchanged.  The ABI version stays 4. */
KVZ_HIP_API int kvz_hip_inter_residual_frames_rdoq(const kvz_hip_chain_picture_rdoq *pictures, int n_pictures, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_intra_recon_frames_rdoq(const kvz_hip_chain_picture_rdoq *pictures, int n_pictures, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Several independent pictures through the QP map, deblocking and     */
/*   SAO at once: the stages behind kvz_hip_*_frames(_ts)              */
/*   reference: set_cu_qps (encoderstate.c:550-609), filter.c:690-779  */
/*   and sao.c:278-337, :580-644 of the pictures in flight (--owf)     */
/* ------------------------------------------------------------------ */
/* One picture of kvz_hip_cu_qp_frames, kvz_hip_deblock_frames, kvz_hip_sao_stats_frames and kvz_hip_sao_frames: the arguments of
 * kvz_hip_cu_qp_frame_tiles, kvz_hip_deblock_frame_tiles, kvz_hip_sao_stats_frame and kvz_hip_sao_frame_tiles as ONE record, so that
 * a host fills it once and hands it to the four calls.  Each entry reads its own fields and ignores the rest ([Q] the QP map, [D]
 * deblocking, [T] the statistics, [S] SAO; width, height and chroma are read by all four).  Every pointer is DEVICE memory except
 * grid, which is HOST memory like the record itself, both copied at the call.  Offsets in front of the fields; no implicit padding. */
typedef struct {
  int32_t width, height;                /*   0, 4: the picture; the size and stride rules are the single-picture entries' */
  int32_t chroma;                       /*   8: 0 = 4:0:0 (the u / v planes and sao_chroma are unused), 1 = 4:2:0 */
  int32_t reserved;                     /*  12: not read */
  kvz_hip_ref_picture src;              /*  16: [T] the source planes; src.width / src.height must equal width / height */
  kvz_hip_pixel *rec_y, *rec_u, *rec_v; /*  56, 64, 72: [D] deblocked in place; [T] [S] read */
  uint32_t stride_y, stride_c;          /*  80, 84: of rec_y and of rec_u / rec_v */
  kvz_hip_pixel *dst_y, *dst_u, *dst_v; /*  88, 96, 104: [S] written */
  uint32_t dst_stride_y, dst_stride_c;  /* 112, 116: of dst_y and of dst_u / dst_v */
  kvz_hip_cu_info *cus;                 /* 120: [Q] cus[].qp written; [D] read */
  const uint8_t *cbf;                   /* 128: [Q] one byte per SCU */
  const int8_t *lcu_qp;                 /* 136: [Q] */
  int8_t *lcu_last_qp;                  /* 144: [Q] written */
  kvz_hip_sao_lcu_stats *stats;         /* 152: [T] written */
  kvz_hip_sao_lcu_cand *cands;          /* 160: [T] written; optional */
  const kvz_hip_sao_info *sao_luma;     /* 168: [S] */
  const kvz_hip_sao_info *sao_chroma;   /* 176: [S] with chroma */
  const kvz_hip_tile_grid *grid;        /* 184: [Q] [D] [S] HOST, optional, copied at the call; NULL = one tile */
  kvz_hip_deblock_params deblock;       /* 192: [D]; deblock.chroma must equal chroma, in every entry */
  kvz_hip_cu_qp_tiles_params cu_qp;     /* 256: [Q] start_qp, chain_rows */
} kvz_hip_filter_picture;               /* 264 bytes */
/* kvz_hip_cu_qp_frame_tiles, kvz_hip_deblock_frame_tiles, kvz_hip_sao_stats_frame and kvz_hip_sao_frame_tiles for n_pictures
 * (0..KVZ_HIP_MAX_CHAIN_PICTURES) pictures that do not depend on each other, in one asynchronous call each.  The stages are a few
 * short launches per picture and bound by them; independent pictures share the launches, the picture being one more grid dimension.
 * THE RULE: for every picture i and every output array, the result is byte for byte what the single-picture entry leaves when called
 *   with the fields of pictures[i]: kvz_hip_cu_qp_frame_tiles (cus[].qp, lcu_last_qp), kvz_hip_deblock_frame_tiles (the rec planes),
 *   kvz_hip_sao_frame_tiles (the dst planes), and kvz_hip_sao_stats_frame (stats, cands), which has no tiled form.  grid == NULL is
 *   one tile, byte for byte the untiled entry; with grid == NULL, cu_qp.chain_rows 0 and 1 mean what chain_lcus = 0 and chain_lcus =
 *   ceil(width / 64) mean in kvz_hip_cu_qp_frame.  Pictures of one call may differ in size, chroma format (4:0:0 beside 4:2:0), tile
 *   grid (tiled beside untiled), chain_rows, every field of deblock, and in whether they carry cands.  There is no homogeneity rule:
 *   the kernels always take a grid, one tile for NULL, so no option selects an instantiation.
 * Independence is the caller's promise, as for kvz_hip_*_frames: no output of one record may be an input or an output of another;
 *   inputs may be shared.  Records whose output base pointers coincide are refused: rec_y (kvz_hip_deblock_frames), dst_y
 *   (kvz_hip_sao_frames), cus or lcu_last_qp (kvz_hip_cu_qp_frames), stats (kvz_hip_sao_stats_frames).
 * Errors: n_pictures == 0 is a no-op that returns KVZ_HIP_OK (pictures may then be NULL).  KVZ_HIP_ERR_INVALID: n_pictures below 0 or
 *   above KVZ_HIP_MAX_CHAIN_PICTURES, pictures == NULL, any record that the single-picture entry would refuse (a missing pointer, a
 *   misaligned plane, cus or per-LCU array, a bad size or stride, kvz_hip_sao_frames' dst == rec, start_qp outside 0..51, chain_rows
 *   other than 0 and 1), an invalid grid, deblock.chroma != chroma, src.width / src.height that differ from width / height, shared
 *   outputs, and a record whose grid no longer fits the pool of KVZ_HIP_CHAIN_TILE_BOUNDS boundaries that the grids of a call share
 *   (cols + rows + 2 values per record with a grid).  Every record is checked before anything is launched: a refusal writes nothing
 *   for any picture, and kvz_hip_last_error() names the record's index ("picture 2") -- for the pool, the record at which it
 *   overflowed.
 * Execution: asynchronous on s; no host synchronisation, no allocation, no workspace, no atomics on memory -- the call owns no device
 *   buffer.  The records (64 / 120 / 96 / 120 bytes per picture for the four entries) and the pool travel in the kernel arguments,
 *   below 4 KB, and are read with scalar loads.  Usable between kvz_hip_graph_begin / _end.  The launch shapes depend only on the
 *   sizes, the chroma flags, the grids, chain_rows and the presence of cands: a captured call may be replayed after the CONTENTS of
 *   every device array changed.
 * Launches: the single entries' own, each covering all pictures -- 3 for kvz_hip_cu_qp_frames, 2 for kvz_hip_deblock_frames, 1 for
 *   kvz_hip_sao_stats_frames, 1 for kvz_hip_sao_frames.  A launch is sized for the largest picture of the call; the surplus
 *   workgroups of a smaller picture leave at once.
 * LEFT OUT ON PURPOSE: prediction of several pictures (kvz_hip_inter_recon_frame: each picture brings a table of up to sixteen
 *   40-byte reference pictures, and sixteen such tables do not fit the 4 KB of kernel arguments; a reference pool that the records
 *   share is a design of its own: kvz_hip_inter_recon_frames below); pictures coded with --lossless, whose chain ends before
 *   deblocking; the SAO mode / merge decision
 *   and RDOQ, which stay with the host.  The ABI version stays 4.  (RDOQ as a batch entry: kvz_hip_rdoq_batch, above.) */
KVZ_HIP_API int kvz_hip_cu_qp_frames(const kvz_hip_filter_picture *pictures, int n_pictures, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_deblock_frames(const kvz_hip_filter_picture *pictures, int n_pictures, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_sao_stats_frames(const kvz_hip_filter_picture *pictures, int n_pictures, kvz_hip_stream s);
KVZ_HIP_API int kvz_hip_sao_frames(const kvz_hip_filter_picture *pictures, int n_pictures, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* Several independent pictures through motion compensation at once:   */
/*   the stage in front of kvz_hip_*_frames(_ts), over one shared      */
/*   pool of reference pictures                                        */
/*   reference: kvz_inter_recon_cu (inter.c:492-540) of the pictures   */
/*   in flight (--owf), which share most of their references           */
/* ------------------------------------------------------------------ */
/* The reference pictures of all records of one call: the pictures in flight of a GOP name few distinct pictures, so the records index
 * ONE pool instead of bringing a table each -- sixteen tables of sixteen 40-byte pictures would not fit a kernel's arguments. */
#define KVZ_HIP_RECON_POOL_PICTURES 48
/* One picture of kvz_hip_inter_recon_frames: the arguments of kvz_hip_inter_recon_frame as a record, its table of reference pictures
 * as indices into the pool.  The record is HOST memory, copied at the call.  Offsets in front of the fields; no implicit padding. */
typedef struct {
  kvz_hip_pixel *pred_y, *pred_u, *pred_v;  /*  0,  8, 16: DEVICE destination planes */
  uint32_t stride_y, stride_c;              /* 24, 28 */
  int32_t width, height;                    /* 32, 36 */
  const kvz_hip_cu_info *cus;               /* 40: DEVICE */
  uint8_t refs[16];                         /* 48: pool index of this picture's reference picture i */
  kvz_hip_inter_recon_params params;        /* 64: chroma, n_refs, ref_LX -- as for the single entry */
} kvz_hip_recon_picture;                    /* 104 bytes, no implicit padding */
/* kvz_hip_inter_recon_frame for n_pictures (0..KVZ_HIP_MAX_CHAIN_PICTURES) pictures that do not depend on each other, in one
 * asynchronous call and one launch: a batch of P or B pictures goes from the CU map to SAO in one call per stage.
 * THE RULE: for every picture i, the three destination planes are byte for byte what kvz_hip_inter_recon_frame leaves when called
 *   with the record's fields and a table refs[k] = pool[pictures[i].refs[k]] for k < params.n_refs.  Everything the single entry
 *   defines holds per picture: which CUs and PUs are predicted or skipped, "pixels of anything else are left untouched",
 *   picture-wide coordinates, and unspecified output inside a CU whose records disagree.  Pictures of one call may differ in size,
 *   chroma format (4:0:0 beside 4:2:0), n_refs and ref_LX, and two records may name the same pool pictures in a different order.
 * Pool: pool is HOST memory, copied at the call, n_pool in 1..KVZ_HIP_RECON_POOL_PICTURES.  A pool picture that no record names is
 *   ignored entirely: its fields are not looked at.  A pool picture named by a record must have the record's width and height and
 *   a valid y / stride_y; if the record is 4:2:0 it must also have valid u, v and stride_c.  The same pool picture may serve a
 *   4:0:0 record without chroma planes.  refs[k] for k >= n_refs is not read.
 * Independence is the caller's promise: no destination plane may be a pool plane or a plane of another record.  Records whose
 *   pred_y bases coincide are refused, and so is a record whose pred_y / pred_u / pred_v base equals the y / u / v base of a pool
 *   picture named by any record.  Any other overlap is a caller error with unspecified output, but no access leaves a record's
 *   own arrays.
 * Errors: n_pictures == 0 is a no-op that returns KVZ_HIP_OK (pictures and pool may then be NULL).  KVZ_HIP_ERR_INVALID: n_pictures
 *   outside 0..KVZ_HIP_MAX_CHAIN_PICTURES; n_pool outside 1..KVZ_HIP_RECON_POOL_PICTURES when n_pictures > 0; a NULL table; any
 *   record the single entry would refuse (a missing pointer, a misaligned cus, a bad size or stride, n_refs outside 1..16);
 *   refs[k] >= n_pool for a k < n_refs; a named pool picture of another size or with missing planes; the aliasing cases above.
 *   Every record is checked before anything is launched: on refusal nothing is written for any picture, and kvz_hip_last_error()
 *   names the index of the offending record ("picture 2").  Without a device the entry returns KVZ_HIP_ERR_NO_DEVICE before it
 *   looks at anything.
 * Execution: one launch covers all pictures -- the sum over the pictures of ceil(tiles / 4) workgroups, a tile being a 16x16 luma
 *   block of its picture; a workgroup never spans two pictures.
 *   Asynchronous on s; no host synchronisation, no allocation, no workspace -- the call owns no device buffer.  Records and pool
 *   travel in the kernel arguments (88 bytes per picture with its reference lists resolved to pool indices, 40 per pool picture:
 *   3336 bytes, below 4 KB) and are read with scalar loads; no atomics, no barriers.  Usable between kvz_hip_graph_begin / _end.  The launch shape depends only on the sizes: a captured call
 *   may be replayed after the CONTENTS of the CU arrays and of every plane changed.
 * LEFT OUT ON PURPOSE: a per-PU entry over the pool (kvz_hip_inter_recon_batch stays single-picture); more than
 *   KVZ_HIP_RECON_POOL_PICTURES distinct references in one call (split the call).  The ABI version stays 4. */
KVZ_HIP_API int kvz_hip_inter_recon_frames(const kvz_hip_recon_picture *pictures, int n_pictures,
                                           const kvz_hip_ref_picture *pool, int n_pool, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* nal group and the last stage of the picture chain: the checksum of  */
/*   the decoded-picture-hash SEI and the per-plane squared error      */
/*   reference: array_checksum (strategies-nal.h:34-55,                */
/*   nal-generic.c:45-69) as kvz_image_checksum calls it per plane     */
/*   (nal.c:65-74, encoder_state-bitstream.c:894-944), and the SSE     */
/*   behind the PSNR (encmain.c:101-129)                               */
/* ------------------------------------------------------------------ */
/* THE ARITHMETIC, bit depth 8.  For a plane of width x height pixels with row stride `stride`:
 *   checksum = ( sum over y, x of  data[y * stride + x] ^ mask(x, y) )  mod 2^32
 *   mask(x, y) = ((x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8)) & 255
 * x, y are the plane's own coordinates (chroma coordinates for a chroma plane); the SEI carries the 32 bits big-endian.
 *   sse = sum of (src - rec)^2 per plane, an exact integer (the reference accumulates in double, exact below 2^53).
 * MD5 IS LEFT OUT ON PURPOSE: array_md5 is one serial dependency chain per plane (64-byte blocks, each needing the state the
 *   block before it left), so a GPU has nothing to run side by side; and array_md5_generic (nal-generic.c:29-43) hashes
 *   width * height CONTIGUOUS bytes and ignores stride, so it is not a function of a plane in the sense of every entry here.
 *   No array_md5 is registered: the selector keeps generic for it. */
typedef struct { uint32_t checksum[3]; uint32_t sse[3]; } kvz_hip_lcu_hash;       /* 24 bytes; Y, U, V of one LCU */
typedef struct { uint32_t checksum[3]; uint32_t n_lcu; uint64_t sse[3]; } kvz_hip_picture_hash;  /* 40 bytes */
/* kvz_hip_lcu_hash: checksum[c] is the LCU's share of plane c's sum, taken with PICTURE coordinates in the mask, so the sum of
 *   the records modulo 2^32 is the plane's checksum; sse[c] is the LCU's share of the squared error (4096 * 255^2 < 2^32).
 *   An LCU is 64 x 64 luma and 32 x 32 chroma pixels, clipped at the right and bottom picture edge.  The planes a picture does
 *   not have (4:0:0) and sse without a source are written as 0: every field of every record is written.
 * kvz_hip_picture_hash: the sums over the LCU records; n_lcu the number of records summed; sse in 64 bits.
 *
 * (a) kvz_hip_picture_hash_frame: the hash of one reconstructed picture, the stage after kvz_hip_sao_frame (with --lossless, after
 *   the intra stage).  Size, stride, alignment and chroma rules are those of kvz_hip_sao_stats_frame: planes and strides 4-byte
 *   aligned, strides >= the width, width / height multiples of 8, at least 8, at most 16384; chroma 0 for 4:0:0 (the chroma
 *   pointers are unused), 1 for 4:2:0.  The bytes between width and stride and below height are never read.
 *   src: HOST, copied at the call, DEVICE planes; NULL or src->y == NULL means checksum only (sse 0); otherwise src->width /
 *     src->height must equal width / height.
 *   lcu_out: DEVICE, required, 4-byte aligned, n_lcu = ceil(width / 64) * ceil(height / 64) records in raster order over the LCUs
 *     -- the first launch's output.  out: DEVICE, required, 8-byte aligned, one record.
 *   Two launches: one workgroup per LCU reads every byte once (16-byte row loads where base and stride are 16-byte aligned, dwords
 *     otherwise) and writes its record; one workgroup then sums the records.  No atomics on memory, no allocation, no buffer
 *     owned by the call, nothing to clear beforehand, and no result depends on the order in which workgroups run.
 *   Asynchronous on s; usable between kvz_hip_graph_begin / _end; the launch shapes depend on width, height and chroma only, so a
 *     captured call may be replayed after the CONTENTS of the planes changed.
 *   Errors: KVZ_HIP_ERR_INVALID for a missing pointer, a bad size or stride or a misaligned plane or record array; nothing is
 *     written.  Without a device KVZ_HIP_ERR_NO_DEVICE before anything is looked at. */
KVZ_HIP_API int kvz_hip_picture_hash_frame(const kvz_hip_ref_picture *src, const kvz_hip_pixel *rec_y, uint32_t stride_y,
                                           const kvz_hip_pixel *rec_u, const kvz_hip_pixel *rec_v, uint32_t stride_c, int width,
                                           int height, int chroma, kvz_hip_lcu_hash *lcu_out, kvz_hip_picture_hash *out,
                                           kvz_hip_stream s);
/* One picture of kvz_hip_picture_hash_frames: the arguments of kvz_hip_picture_hash_frame as a record (kvz_hip_filter_picture is
 * full and fixed).  HOST memory, copied at the call; every pointer is DEVICE memory.  Offsets in front of the fields; no implicit
 * padding. */
typedef struct {
  int32_t width, height;                      /*  0,  4 */
  int32_t chroma;                             /*  8: 0 = 4:0:0, 1 = 4:2:0 */
  int32_t reserved;                           /* 12: not read */
  kvz_hip_ref_picture src;                    /* 16: src.y == NULL: checksum only; else src.width / src.height = width / height */
  const kvz_hip_pixel *rec_y, *rec_u, *rec_v; /* 56, 64, 72 */
  uint32_t stride_y, stride_c;                /* 80, 84 */
  kvz_hip_lcu_hash *lcu_out;                  /* 88: written, n_lcu records */
  kvz_hip_picture_hash *out;                  /* 96: written, one record */
} kvz_hip_hash_picture;                       /* 104 bytes */
/* (b) kvz_hip_picture_hash_frames: kvz_hip_picture_hash_frame for n_pictures (0..KVZ_HIP_MAX_CHAIN_PICTURES) pictures in the same two
 *   launches, the picture being one more grid dimension; 0 is a no-op.
 *   THE RULE: per picture, lcu_out and out hold byte for byte what kvz_hip_picture_hash_frame leaves for the record's fields.
 *   Pictures may differ in size, chroma format and in whether they carry src.  The records (96 bytes per picture) travel in the
 *   kernel arguments.  Every record is checked before anything is launched: a refusal (KVZ_HIP_ERR_INVALID) names the record in
 *   kvz_hip_last_error() ("picture 2") and writes nothing.  Records that share lcu_out or out are refused.  Everything else as (a). */
KVZ_HIP_API int kvz_hip_picture_hash_frames(const kvz_hip_hash_picture *pictures, int n_pictures, kvz_hip_stream s);
/* (c) the strategy's contract, for arbitrary planes: array_checksum of up to KVZ_HIP_MAX_HASH_PLANES planes in two launches.
 *   planes: HOST records, copied at the call; data is DEVICE memory.  width, height in 1..65536, any stride >= width, any base
 *     alignment (16-byte loads where a row segment is 16-byte aligned, dwords where it is 4-byte aligned, bytes otherwise);
 *     no byte outside the width x height pixels is read.
 *   block_sums: DEVICE scratch, 4-byte aligned, the sum over the planes of kvz_hip_array_checksum_blocks(width, height) values (one
 *     per 64 x 64 block; a host-only helper that needs no device and returns 0 for a size out of range).  Every value used is
 *     written first: nothing to clear.
 *   checksums: DEVICE, 4-byte aligned, n_planes values, the checksum of plane i at [i], in the host's byte order.
 *   n_planes == 0 is a no-op.  Asynchronous on s; no allocation, no atomics on memory; usable between kvz_hip_graph_begin / _end.
 *   Errors as (a); a refusal names the record ("plane 2"). */
#define KVZ_HIP_MAX_HASH_PLANES 48
typedef struct {
  const kvz_hip_pixel *data;                  /*  0: DEVICE */
  int32_t width, height;                      /*  8, 12 */
  uint32_t stride;                            /* 16 */
  uint32_t reserved;                          /* 20: not read */
} kvz_hip_hash_plane;                         /* 24 bytes */
KVZ_HIP_API size_t kvz_hip_array_checksum_blocks(int width, int height);
KVZ_HIP_API int kvz_hip_array_checksum_batch(const kvz_hip_hash_plane *planes, int n_planes, uint32_t *block_sums,
                                             uint32_t *checksums, kvz_hip_stream s);

/* ------------------------------------------------------------------ */
/* (1) strategy registration -- the drop-in boundary                   */
/* ------------------------------------------------------------------ */
/* kvz_strategyselector_register (strategyselector.h:87, strategyselector.c:216-256) */
typedef int (*kvz_hip_register_fn)(void *opaque, const char *type, const char *strategy_name, int priority, void *fptr);
/* By default the hooks call the process's own kvz_strategyselector_register
 * (resolved at load time from the host encoder).  A host that links the
 * selector with hidden visibility passes it explicitly. */
KVZ_HIP_API void kvz_hip_set_registrar(kvz_hip_register_fn fn);
/* Number of per-call strategy invocations that launched GPU work since load (all threads):
 * lets a host or test confirm the "hip" pointers are the ones its encoder is calling. */
KVZ_HIP_API unsigned long long kvz_hip_dropin_calls(void);

/* Accessors for the opaque encoder_state_t the quant strategies receive
 * (encoderstate.h; quant-generic.c:40-50).  Supplied by the few lines of glue
 * compiled inside Kvazaar; without them the quant group
 * registers only coeff_abs_sum. */
typedef struct {
  int (*qp)(const void *state);
  int (*slice_is_intra)(const void *state);
  int (*signhide_enable)(const void *state);
  int (*scaling_list_enable)(const void *state);
  const int32_t *(*quant_coeff)(const void *state, int log2_tr_size, int list_type, int qp_rem);
  const int32_t *(*dequant_coeff)(const void *state, int log2_tr_size, int list_type, int qp_rem);
  int (*rdoq_enable)(const void *state);
  /* cu_info_t fields used by quantize_residual (quant-generic.c:197-225) */
  int (*cu_is_intra)(const void *cur_cu);
  /* optional (may be NULL): planes of hi_prec_buf_t (image.h:38-46) and of lcu_t.rec (cu.h:287-325)
   * for inter_recon_bipred; without them that one function stays on the CPU strategy */
  const int16_t *(*hi_prec_y)(const void *hi_prec_buf);
  const int16_t *(*hi_prec_u)(const void *hi_prec_buf);
  const int16_t *(*hi_prec_v)(const void *hi_prec_buf);
  kvz_hip_pixel *(*lcu_rec_y)(void *lcu);
  kvz_hip_pixel *(*lcu_rec_u)(void *lcu);
  kvz_hip_pixel *(*lcu_rec_v)(void *lcu);
  /* What quantize_residual needs when cfg.rdoq_enable (quant-generic.c:214-221).  kvz_rdoq (rdo.c:548) is the
   * encoder's CABAC-context dependent quantiser -- control plane, not part of this library; like the avx2 strategy,
   * the hip quantize_residual calls the host's own function between the transform (or transform skip) and the
   * dequantisation.  quantize_residual is registered only when rdoq_enable and these four are all supplied, or when
   * rdoq_enable itself is NULL (= the host vouches that RDOQ is never on); likewise quant / dequant /
   * quantize_residual need quant_coeff and dequant_coeff whenever scaling_list_enable is supplied.  A group function
   * that is not registered stays on the host's next-best strategy -- nothing diverges or aborts at run time. */
  int (*rdoq_skip)(const void *state);                 /* cfg.rdoq_skip */
  int (*cu_rdoq_tr_depth)(const void *cur_cu);         /* tr_depth - depth + (part_size == SIZE_NxN) */
  int (*cu_type)(const void *cur_cu);                  /* cur_cu->type, handed to kvz_rdoq as block_type */
  void (*rdoq)(void *state, kvz_hip_coeff *coef, kvz_hip_coeff *dest_coeff, int32_t width, int32_t height,
               int8_t type, int8_t scan_mode, int8_t block_type, int8_t tr_depth);
} kvz_hip_state_accessors;
KVZ_HIP_API void kvz_hip_set_state_accessors(const kvz_hip_state_accessors *acc);

#define KVZ_HIP_STRATEGY_NAME "hip"
#define KVZ_HIP_STRATEGY_PRIORITY 50     /* avx2 = 40 (picture-avx2.c:1232) */

/* Same shape as kvz_strategy_register_picture_avx2 (picture-avx2.c:1224):
 * registers every function of the group under the type strings of
 * STRATEGIES_<GROUP>_EXPORTS, name "hip", priority 50; only for bitdepth 8.
 * Returns 1 on success, 0 on failure. */
KVZ_HIP_API int kvz_strategy_register_picture_hip(void *opaque, uint8_t bitdepth);
KVZ_HIP_API int kvz_strategy_register_dct_hip(void *opaque, uint8_t bitdepth);
KVZ_HIP_API int kvz_strategy_register_quant_hip(void *opaque, uint8_t bitdepth);
KVZ_HIP_API int kvz_strategy_register_ipol_hip(void *opaque, uint8_t bitdepth);
KVZ_HIP_API int kvz_strategy_register_intra_hip(void *opaque, uint8_t bitdepth);   /* strategies-intra.h:52-55 */
KVZ_HIP_API int kvz_strategy_register_sao_hip(void *opaque, uint8_t bitdepth);     /* strategies-sao.h:64-69 */
/* strategies-nal.h:34-55: array_checksum only, with the reference's signature (host pointers, any stride and alignment, complete
 * on return, four bytes big-endian and nothing else of the output array).  array_md5 is not registered (see the nal group above). */
KVZ_HIP_API int kvz_strategy_register_nal_hip(void *opaque, uint8_t bitdepth);

#ifdef __cplusplus
}
#endif
#endif /* KVZ_HIP_H_ */
