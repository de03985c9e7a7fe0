// lcu_layout.h -- what the whole-picture residual entries (inter_residual.hip, intra_recon.hip) share about planes and the
// coefficient arrays: the z-order of lcu->coeff, bits of cbf_out and rows of pixels at any address.
#pragma once

#include "kvz_hip_internal.h"

using namespace kvzhip;

namespace {

// bits of a (4 bits) to the even positions
__device__ __forceinline__ u32 spread4(u32 a) { a = (a | (a << 2)) & 0x33u; return (a | (a << 1)) & 0x55u; }
// xy_to_zorder (cu.h:373-410) in units of 4x4 blocks: x, y = block coordinates inside the LCU
__device__ __forceinline__ u32 zorder_blk(u32 x, u32 y) { return spread4(x) | (spread4(y) << 1); }

// cbf_out is a byte array that several TUs of different planes set bits of: OR into the dword that holds the byte.  For an array that
// is not 4-byte aligned the dwords of its first and last bytes reach up to 3 bytes beyond it; those bytes are OR-ed with 0.
__device__ __forceinline__ void or_byte(u8 *base, size_t i, u32 bits)
{
  const uintptr_t p = (uintptr_t)(base + i);
  atomicOr((u32 *)(p & ~(uintptr_t)3), bits << (8 * (p & 3)));
}

// a row of N pixels at ANY address (PLANES in kvz_hip.h), as dwords
template <int N>
__device__ __forceinline__ void load_row(const u8 *p, u32 (&w)[N / 4]) { __builtin_memcpy(w, p, N); }
template <int N>
__device__ __forceinline__ void store_row(u8 *p, const u32 (&w)[N / 4]) { __builtin_memcpy(p, w, N); }
__device__ __forceinline__ int byte_of(const u32 *w, int x) { return (int)((w[x >> 2] >> (8 * (x & 3))) & 255u); }

}  // namespace
