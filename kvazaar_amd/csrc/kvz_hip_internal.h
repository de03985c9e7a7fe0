// Internal declarations shared by the HIP translation units of libkvzhip.so.
// gfx950 (MI355X, CDNA4) only: wave64, 256 CUs, 160 KiB LDS/CU.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/kvz_hip.h"
#include "tuning.h"                             // the kvz_hip_set_tuning knobs: tuning<tune::key>(), tuning_or<tune::key>(dflt)

typedef uint8_t u8;
typedef uint32_t u32;
typedef int16_t i16;
typedef int32_t i32;

namespace kvzhip {

// ---- context (api.hip) ----
int ctx_device();                               // the calling thread's current device (-1: none initialised)
bool ctx_ready();
bool ctx_enter();                               // ready, and the calling thread's HIP device = its kvz_hip device
hipStream_t ctx_stream(kvz_hip_stream s);      // NULL -> library default stream; counts as an operation on it (event_alias.h)
hipEvent_t launch_carrier(hipStream_t st);     // the event launch_carried() binds to the dispatch, or NULL: launch as ever
void launch_uncarry(hipStream_t st);           // that launch failed: nothing was carried
void set_error(const char *what, hipError_t e);
void set_error_msg(const char *what);
int invalid_arg(const char *entry);             // records "<entry>: invalid argument" and returns KVZ_HIP_ERR_INVALID
int num_cus();
int stream_on_current_device(kvz_hip_stream s, const char *entry);   // KVZ_HIP_ERR_INVALID for a stream of another device

// ---- rectangle copies (halo.hip) ----
// checks rects[0 .. n) as kvz_hip_copy_rects_batch documents and copies them in one launch on st; errors are reported as `entry`'s
int copy_rects_launch(const kvz_hip_rect_copy *rects, int n, hipStream_t st, const char *entry);

#define KVZ_CHECK_CTX()                         \
  do {                                          \
    if (!kvzhip::ctx_enter()) {                 \
      if (kvz_hip_init(-1) != KVZ_HIP_OK || !kvzhip::ctx_enter()) return KVZ_HIP_ERR_NO_DEVICE; \
    }                                           \
  } while (0)

#define KVZ_CHECK_LAUNCH(name)                               \
  do {                                                       \
    hipError_t e__ = hipGetLastError();                      \
    if (e__ != hipSuccess) {                                 \
      kvzhip::set_error(name, e__);                          \
      return KVZ_HIP_ERR_RUNTIME;                            \
    }                                                        \
  } while (0)

// Workgroup cap of a grid-stride launch from a "*_wgs_per_cu" value; a value of 0 counts as 1 (a grid of zero
// workgroups would not run at all).
static inline size_t wg_cap(long long per_cu) { return (size_t)num_cus() * (size_t)(per_cu > 0 ? per_cu : 1); }

// Grid sizing for streaming kernels: enough workgroups to fill 256 CUs several
// times over, capped so that grid-stride loops amortise the launch.
static inline unsigned stream_grid(size_t work_items, unsigned items_per_block, unsigned max_blocks_per_cu = 128)
{
  size_t need = (work_items + items_per_block - 1) / items_per_block;
  size_t cap = wg_cap(max_blocks_per_cu);
  if (need < 1) need = 1;
  return (unsigned)(need < cap ? need : cap);
}

#if defined(__HIPCC__)

// The launch of an entry that enqueues ONE kernel and nothing behind it, on the stream its ctx_stream() call returned.  When the
// caller recorded an event just before the entry, the record that will follow can ride on this dispatch (api.hip,
// kvz_hip_event_record): the launch then binds a carrier event to the dispatch packet, whose completion signal supplies the
// end timestamp and the ordering point.  Otherwise, and always inside a capture, this is hipLaunchKernelGGL.
template <typename T> struct launch_arg { typedef T type; };
template <typename... KArgs>
static inline void launch_carried(void (*kernel)(KArgs...), dim3 grid, dim3 block, unsigned lds, hipStream_t st,
                                  typename launch_arg<KArgs>::type... args)
{
  if (hipEvent_t stop = launch_carrier(st)) {
    hipExtLaunchKernelGGL(kernel, grid, block, lds, st, nullptr, stop, 0, args...);
    if (hipPeekAtLastError() != hipSuccess) launch_uncarry(st);      // the entry's KVZ_CHECK_LAUNCH reports it; the event was never bound
  } else hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

// ---- device helpers ----

// DPP cross-lane moves (no LDS traffic).  quad_perm / row_half_mirror / row_mirror.
template <int CTRL>
__device__ __forceinline__ u32 dpp_mov(u32 v)
{
  return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// Sum over aligned groups of L consecutive lanes (L power of two <= 64); every
// lane of the group ends up with the group's sum.
template <int L>
__device__ __forceinline__ u32 group_sum(u32 v)
{
  if (L >= 2) v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  if (L >= 4) v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  if (L >= 8) v += dpp_mov<0x141>(v);   // row_half_mirror
  if (L >= 16) v += dpp_mov<0x140>(v);  // row_mirror
  if (L >= 32) v += (u32)__shfl_xor((int)v, 16, 64);
  if (L >= 64) v += (u32)__shfl_xor((int)v, 32, 64);
  return v;
}

// Ordering point between two phases of ONE wave that exchange data through its private LDS slice.
// The hardware executes a wave's DS operations in order, so no s_barrier is needed; this only stops
// the compiler from moving LDS accesses across the phase boundary.
__device__ __forceinline__ void wave_lds_fence()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Streaming (touched once) 16-byte global accesses.  The nontemporal policy keeps once-used lines from displacing
// useful ones: measured on MI355X (tools/bw_probe.hip) a copy-shaped kernel moves 6.0-6.4 TB/s with both hints
// against 5.5-5.75 TB/s without, a read-only stream 6.9-7.0 against 6.3.
typedef unsigned int kvz_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_stream_u4(const void *p)
{
  const kvz_u32x4 v = __builtin_nontemporal_load((const kvz_u32x4 *)p);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream_u4(void *p, uint4 v)
{
  const kvz_u32x4 w = { v.x, v.y, v.z, v.w };
  __builtin_nontemporal_store(w, (kvz_u32x4 *)p);
}

// Every outstanding vector-memory operation of the wave has completed; nothing is scheduled across it.
// Why the streaming kernels place this by hand: gfx950 counts vector loads AND stores in one counter (vmcnt), and loads and
// stores complete out of order with each other -- once a store is in flight, "wait for that earlier load" can only be
// expressed as vmcnt(0), which also waits for the stores and for any younger prefetch.  Left to the compiler, a
// load-compute-store loop with a prefetch waits at its top for the stores it has just issued (or even for the prefetch it
// has just issued).  The kernels put the iteration's one vmcnt(0) right BEFORE its first store instead: what is
// outstanding there is the prefetch, issued a stretch of arithmetic earlier, and the previous iteration's stores.
__device__ __forceinline__ void wait_vmem_all()
{
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0); expcnt and lgkmcnt left alone (gfx9 encoding)
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// kvz_fast_clip_16bit_to_pixel (picture-generic.c:30-48): int16 argument,
// any bit outside 0..255 => low byte of (-v >> 15).
__device__ __forceinline__ u8 fast_clip16(i16 v)
{
  int x = v;
  return (x & ~255) ? (u8)((-x) >> 15) : (u8)x;
}
// kvz_fast_clip_32bit_to_pixel (picture-generic.c:52-70)
__device__ __forceinline__ u8 fast_clip32(i32 v)
{
  return (v & ~255) ? (u8)(((i32)(0u - (u32)v)) >> 31) : (u8)v;
}

#endif  // __HIPCC__

}  // namespace kvzhip
