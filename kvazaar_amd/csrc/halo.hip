// halo.hip -- batched 2-D rectangle copies (kvz_hip_copy_rects_batch): the data movement of the tile halo exchange
// (kvz_hip_tile_halo_exchange in api.hip, kvazaar_amd/shard.py exchange_tile_halo_into).
//
// The work of one batch is flattened over the whole grid as (rect, row, 16-byte chunk): the column strips of a tile halo are
// only `margin` bytes wide (80 luma, 40 chroma) and ~1000 rows tall, so a row per wave would leave most lanes idle.  The rects
// are a kernel argument, so a launch uploads nothing.  Each rect carries the widest access its pointers and strides allow
// (16, 8, 4 or 1 bytes); a chunk that runs past the end of its row finishes with narrower accesses.
#include "kvz_hip_internal.h"

namespace kvzhip {

namespace {

constexpr int kThreads = 256;

struct rect_batch {
  kvz_hip_rect_copy r[KVZ_HIP_MAX_RECTS];
  uint32_t first[KVZ_HIP_MAX_RECTS + 1];    // first[i]: index of rect i's first chunk; first[n] = all chunks of the batch
  uint32_t chunks_per_row[KVZ_HIP_MAX_RECTS];
  uint32_t align[KVZ_HIP_MAX_RECTS];        // 16, 8, 4 or 1: the access width src, dst and both strides allow
  int32_t n;                                // non-empty rects
};

__global__ __launch_bounds__(kThreads) void copy_rects_kernel(const rect_batch b)
{
  const uint32_t total = b.first[b.n];
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < total; i += gridDim.x * kThreads) {
    int k = 0;
    while (k + 1 < b.n && i >= b.first[k + 1]) ++k;
    const kvz_hip_rect_copy &r = b.r[k];
    const uint32_t j = i - b.first[k];
    const uint32_t cpr = b.chunks_per_row[k];
    const uint32_t row = j / cpr;
    const uint32_t off = (j - row * cpr) * 16u;
    const uint32_t left = (uint32_t)r.w - off;
    const int bytes = left < 16u ? (int)left : 16;
    const u8 *s = (const u8 *)r.src + (size_t)row * r.src_stride + off;
    u8 *d = (u8 *)r.dst + (size_t)row * r.dst_stride + off;
    const uint32_t al = b.align[k];
    if (al == 16 && bytes == 16) {
      *(uint4 *)d = *(const uint4 *)s;
      continue;
    }
    int c = 0;
    if (al >= 8)
      for (; c + 8 <= bytes; c += 8) *(uint2 *)(d + c) = *(const uint2 *)(s + c);
    if (al >= 4)
      for (; c + 4 <= bytes; c += 4) *(uint32_t *)(d + c) = *(const uint32_t *)(s + c);
    for (; c < bytes; ++c) d[c] = s[c];
  }
}

uint32_t access_width(uintptr_t bits)
{
  if ((bits & 15u) == 0) return 16;
  if ((bits & 7u) == 0) return 8;
  if ((bits & 3u) == 0) return 4;
  return 1;
}

}  // namespace

int copy_rects_launch(const kvz_hip_rect_copy *rects, int n, hipStream_t st, const char *entry)
{
  if (n < 0 || n > KVZ_HIP_MAX_RECTS || (n > 0 && !rects)) return invalid_arg(entry);
  rect_batch b{};
  uint64_t total = 0;
  for (int i = 0; i < n; ++i) {
    const kvz_hip_rect_copy &r = rects[i];
    if (r.w < 0 || r.h < 0) return invalid_arg(entry);
    if (r.w == 0 || r.h == 0) continue;
    if (!r.src || !r.dst || (r.h > 1 && (r.src_stride < (uint32_t)r.w || r.dst_stride < (uint32_t)r.w))) return invalid_arg(entry);
    const uint32_t cpr = ((uint32_t)r.w + 15u) / 16u;
    b.r[b.n] = r;
    b.first[b.n] = (uint32_t)total;
    b.chunks_per_row[b.n] = cpr;
    b.align[b.n] = access_width((uintptr_t)r.src | (uintptr_t)r.dst | (uintptr_t)(r.h > 1 ? r.src_stride | r.dst_stride : 0u));
    total += (uint64_t)cpr * (uint64_t)r.h;
    if (total >= (1ull << 31)) return invalid_arg(entry);       // keeps the grid-stride index clear of wrapping
    ++b.n;
  }
  b.first[b.n] = (uint32_t)total;
  if (total == 0) return KVZ_HIP_OK;
  // one chunk per thread; a batch larger than 8 workgroups per CU strides over the grid
  const unsigned grid = stream_grid((size_t)total, kThreads, 8);
  copy_rects_kernel<<<grid, kThreads, 0, st>>>(b);
  KVZ_CHECK_LAUNCH(entry);
  return KVZ_HIP_OK;
}

}  // namespace kvzhip

using namespace kvzhip;

extern "C" int kvz_hip_copy_rects_batch(const kvz_hip_rect_copy *rects, int n, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  const int rc = stream_on_current_device(s, "kvz_hip_copy_rects_batch");
  if (rc != KVZ_HIP_OK) return rc;
  return copy_rects_launch(rects, n, ctx_stream(s), "kvz_hip_copy_rects_batch");
}
