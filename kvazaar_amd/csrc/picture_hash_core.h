// picture_hash_core.h -- the checksum of the decoded-picture-hash SEI and the squared error of a reconstructed picture: the kernels
// of kvz_hip_picture_hash_frame(s) and kvz_hip_array_checksum_batch (picture_hash.hip instantiates them).
//
// Reference: array_checksum_generic (nal-generic.c:45-69): the sum modulo 2^32 of data[y * stride + x] ^ mask(x, y) with
// mask(x, y) = ((x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8)) & 255; the SSE of encmain.c:101-129 (compute_psnr).
//
// A work item takes one 16-byte segment of a row (x a multiple of 16 in plane coordinates) as four packed dwords.  For a 4-aligned x
// the masks of four neighbouring pixels are base * 0x01010101 ^ 0x03020100 with base = mask(x, y), since only the two low bits of
// x & 255 differ between them; the byte sum of a dword is v_sad_u8 against 0, and (a - b)^2 summed over a dword is
// dot4(a, a) + dot4(b, b) - 2 dot4(a, b) with v_dot4_u32_u8.  Bytes outside the plane are never loaded and count as 0 on both sides.
// A 64 x 64 block is 256 segments, one per work item; the sums go through DPP inside a wave and through LDS across the four waves,
// and leave through ordinary stores: one record per block, summed by a second launch with one workgroup per picture (or plane).  No
// atomics on memory, nothing to clear, and integer sums: no result depends on the order in which workgroups run.
#pragma once

#include "kvz_hip_internal.h"
#include "chain_host.h"

namespace {

using namespace kvzhip;
typedef unsigned long long u64;

// the nb (0..16) bytes at p as four dwords: byte j of the segment in bits 8 (j & 3) of v[j >> 2], every other byte 0.  Nothing outside
// the nb bytes is read: one 16-byte load where the segment is whole and 16-byte aligned, dwords with a byte tail where it is 4-byte
// aligned, bytes otherwise.
__device__ __forceinline__ void load_seg(const u8 *p, int nb, u32 (&v)[4])
{
  v[0] = v[1] = v[2] = v[3] = 0;
  if (nb <= 0) return;
  const uintptr_t at = (uintptr_t)p;
  if (nb == 16 && !(at & 15)) {
    const uint4 q = *(const uint4 *)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else if (!(at & 3)) {
    const int nd = nb >> 2;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nd) v[k] = *(const u32 *)(p + 4 * k);
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j >= 4 * nd && j < nb) v[j >> 2] |= (u32)p[j] << (8 * (j & 3));
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < nb) v[j >> 2] |= (u32)p[j] << (8 * (j & 3));
  }
}

// 0xFF for each of the bytes of dword k that lie inside a segment of nb bytes
__device__ __forceinline__ u32 seg_valid(int nb, int k)
{
  const int n = nb - 4 * k;
  return n >= 4 ? 0xFFFFFFFFu : (n <= 0 ? 0u : (1u << (8 * n)) - 1u);
}

// the masks of the pixels x .. x + 3 of row y, x a multiple of 4
__device__ __forceinline__ u32 mask4(int x, int y)
{
  return (u32)((x ^ y ^ (x >> 8) ^ (y >> 8)) & 255) * 0x01010101u ^ 0x03020100u;
}

// one segment: nb bytes of row y from column x on, at rp (and at sp where there is a source)
__device__ __forceinline__ void seg_hash(const u8 *rp, const u8 *sp, int nb, int x, int y, u32 &cs, u32 &sse)
{
  u32 r[4];
  load_seg(rp, nb, r);
#pragma unroll
  for (int k = 0; k < 4; ++k) cs = __builtin_amdgcn_sad_u8((r[k] ^ mask4(x + 4 * k, y)) & seg_valid(nb, k), 0u, cs);
  if (sp) {
    u32 o[4];
    load_seg(sp, nb, o);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u32 sq = __builtin_amdgcn_udot4(r[k], r[k], __builtin_amdgcn_udot4(o[k], o[k], 0u, false), false);
      sse += sq - 2u * __builtin_amdgcn_udot4(r[k], o[k], 0u, false);
    }
  }
}

__device__ __forceinline__ u64 wave_sum64(u64 v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const u32 lo = (u32)__shfl_xor((int)(u32)v, m, 64), hi = (u32)__shfl_xor((int)(u32)(v >> 32), m, 64);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}

// ---- a picture: one workgroup per LCU, then one per picture ----
struct hash_args {
  const u8 *rec[3], *src[3];                // [1], [2] null for 4:0:0; src[0] null: checksum only
  u32 rec_stride[2], src_stride[2];         // [0] luma, [1] chroma
  int width, height, lcus_x, n_lcu;
  kvz_hip_lcu_hash *lcu_out;
  kvz_hip_picture_hash *out;
};
template <int N> struct hash_batch { hash_args p[N]; };
static_assert(sizeof(hash_args) == 96 && sizeof(hash_batch<KVZ_HIP_MAX_CHAIN_PICTURES>) <= 4096, "the records travel in the kernel arguments");

// grid (LCUs of the largest picture, pictures).  All four waves take the 64 x 64 luma block, four segments to a row; wave 0 then takes
// the 32 x 32 block of U and wave 1 that of V, two segments to a row.
template <int N>
__global__ __launch_bounds__(256) void picture_hash_lcu_kernel(hash_batch<N> b)
{
  const hash_args a = b.p[blockIdx.y];
  if ((int)blockIdx.x >= a.n_lcu) return;
  __shared__ u32 s_part[4][4];              // per wave: luma checksum, luma sse, chroma checksum, chroma sse
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ly = (int)blockIdx.x / a.lcus_x, lx = (int)blockIdx.x - ly * a.lcus_x;
  u32 cs = 0, sse = 0, cs_c = 0, sse_c = 0;
  {
    const int x = lx * 64 + (tid & 3) * 16, y = ly * 64 + (tid >> 2);
    const int nb = y < a.height ? min(max(a.width - x, 0), 16) : 0;
    seg_hash(a.rec[0] + (size_t)y * a.rec_stride[0] + x, a.src[0] ? a.src[0] + (size_t)y * a.src_stride[0] + x : nullptr, nb, x, y, cs, sse);
  }
  if (a.rec[1] && wave < 2) {
    const u8 *rec = wave ? a.rec[2] : a.rec[1], *src = a.src[0] ? (wave ? a.src[2] : a.src[1]) : nullptr;
    const int x = lx * 32 + (lane & 1) * 16, y = ly * 32 + (lane >> 1);
    const int nb = y < (a.height >> 1) ? min(max((a.width >> 1) - x, 0), 16) : 0;
    seg_hash(rec + (size_t)y * a.rec_stride[1] + x, src ? src + (size_t)y * a.src_stride[1] + x : nullptr, nb, x, y, cs_c, sse_c);
  }
  cs = group_sum<64>(cs); sse = group_sum<64>(sse); cs_c = group_sum<64>(cs_c); sse_c = group_sum<64>(sse_c);
  if (lane == 0) { s_part[wave][0] = cs; s_part[wave][1] = sse; s_part[wave][2] = cs_c; s_part[wave][3] = sse_c; }
  __syncthreads();
  if (tid < 6) {
    // the record as six dwords: checksum Y U V, sse Y U V
    const int c = tid < 3 ? tid : tid - 3, f = tid < 3 ? 0 : 1;
    const u32 v = c == 0 ? s_part[0][f] + s_part[1][f] + s_part[2][f] + s_part[3][f] : s_part[c - 1][2 + f];
    ((u32 *)(a.lcu_out + blockIdx.x))[tid] = v;
  }
}

// grid (pictures): the picture's record from its LCU records
template <int N>
__global__ __launch_bounds__(256) void picture_hash_sum_kernel(hash_batch<N> b)
{
  const hash_args a = b.p[blockIdx.x];
  __shared__ u32 s_cs[4][3];
  __shared__ u64 s_se[4][3];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  u32 cs[3] = { 0, 0, 0 };
  u64 se[3] = { 0, 0, 0 };
  for (int i = tid; i < a.n_lcu; i += 256) {
    const u32 *r = (const u32 *)(a.lcu_out + i);
#pragma unroll
    for (int c = 0; c < 3; ++c) { cs[c] += r[c]; se[c] += r[3 + c]; }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    cs[c] = group_sum<64>(cs[c]);
    se[c] = wave_sum64(se[c]);
    if (lane == 0) { s_cs[wave][c] = cs[c]; s_se[wave][c] = se[c]; }
  }
  __syncthreads();
  if (tid < 3) {
    a.out->checksum[tid] = s_cs[0][tid] + s_cs[1][tid] + s_cs[2][tid] + s_cs[3][tid];
    a.out->sse[tid] = s_se[0][tid] + s_se[1][tid] + s_se[2][tid] + s_se[3][tid];
  }
  if (tid == 3) a.out->n_lcu = (u32)a.n_lcu;
}

// ---- arbitrary planes: one workgroup per 64 x 64 block, then one per plane ----
struct plane_args {
  const u8 *data;
  int width, height;
  u32 stride;
  int y0;                                   // the plane's first row in the coordinates of the mask (a band of a larger plane)
  u32 first_block, n_blocks;                // where the plane's values stand in block_sums
  int blocks_x, pad;
};
struct plane_batch {
  plane_args p[KVZ_HIP_MAX_HASH_PLANES];
  u32 *block_sums, *checksums;
  int n_planes, pad;
};
static_assert(sizeof(plane_args) == 40 && sizeof(plane_batch) <= 4096, "the records travel in the kernel arguments");

// grid (blocks of all planes)
__global__ __launch_bounds__(256) void array_checksum_block_kernel(plane_batch b)
{
  __shared__ u32 s_part[4];
  const u32 blk = blockIdx.x;
  int i = 0;
  for (int k = 1; k < b.n_planes; ++k)
    if (b.p[k].first_block <= blk) i = k;   // first_block ascends
  const plane_args a = b.p[i];
  const int tid = (int)threadIdx.x, local = (int)(blk - a.first_block);
  const int by = local / a.blocks_x, bx = local - by * a.blocks_x;
  const int x = bx * 64 + (tid & 3) * 16, y = by * 64 + (tid >> 2);
  const int nb = y < a.height ? min(max(a.width - x, 0), 16) : 0;
  u32 cs = 0, unused = 0;
  seg_hash(a.data + (size_t)y * a.stride + x, nullptr, nb, x, a.y0 + y, cs, unused);
  cs = group_sum<64>(cs);
  if ((tid & 63) == 0) s_part[tid >> 6] = cs;
  __syncthreads();
  if (tid == 0) b.block_sums[blk] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// grid (planes)
__global__ __launch_bounds__(256) void array_checksum_sum_kernel(plane_batch b)
{
  __shared__ u32 s_part[4];
  const plane_args a = b.p[blockIdx.x];
  const int tid = (int)threadIdx.x;
  u32 cs = 0;
  for (u32 i = (u32)tid; i < a.n_blocks; i += 256) cs += b.block_sums[a.first_block + i];
  cs = group_sum<64>(cs);
  if ((tid & 63) == 0) s_part[tid >> 6] = cs;
  __syncthreads();
  if (tid == 0) b.checksums[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

}  // namespace
