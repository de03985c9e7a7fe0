// cu_qp.hip -- the QP map of a picture whose QP changes per LCU, for gfx950 (kvz_hip_cu_qp_frame): what set_cu_qps
// (encoderstate.c:550-609) leaves in cu_array->qp for the deblocking filter (get_qp_y_pred, filter.c:263-282), and the QP
// predictor of every LCU that the entropy coder codes cu_qp_delta against (encode_coding_tree.c:511-529), between
// kvz_hip_intra_recon_frame_qp and kvz_hip_deblock_frame with per_cu_qp = 1.
//
// Reference: set_cu_qps with max_qp_delta_depth == 0 -- the quantization group is the LCU -- over kvz_get_cu_ref_qp
// (encoderstate.c:1408-1430) and is_last_cu_in_qg (encoderstate.h:332-342).  With the group at the LCU's corner both predictors of
// kvz_get_cu_ref_qp are last_qp, so a CU before the first coded CU of its LCU gets last_qp, the first coded CU and every CU after
// it keep the LCU's QP (prev_qp >= 0 from there on), and *last_qp = cu->qp at the group's last CU stores the LCU's QP if the LCU
// has a coded CU and last_qp itself otherwise.  A ragged edge can make is_last_cu_in_qg true for more than one CU; each such store
// writes one of these two values in the same order, so the rule holds there too (the header states the derivation in full).
//
// Three launches of fixed shape, no atomics:
//   1. per LCU: the z-order index of its first coded CU; lcu_last_qp[lcu] = the LCU's QP if there is one, else -1
//   2. per chain: the exclusive scan "QP of the last LCU before this one that has a coded CU, else start_qp" over lcu_last_qp,
//      in place -- one workgroup per chain walks it in runs of 256 with a carry
//   3. per LCU: the first coded CU again (256 records and flags, cheaper than a buffer the call would have to own) and the qp byte
//      of every SCU
#include "kvz_hip_internal.h"
#include "quant_core.h"

using namespace kvzhip;

namespace {

static_assert(sizeof(kvz_hip_cu_qp_params) == 8 && sizeof(kvz_hip_cu_info) == 20, "layouts documented in kvz_hip.h");

struct cu_qp_args {
  u32 *cus;                      // records as five dwords; depth is byte 1, qp byte 6
  const u8 *cbf;                 // one byte per SCU
  const int8_t *lcu_qp;
  int8_t *lcu_last_qp;
  int cus_stride, lcus_x;
  int width, height;
};

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}

// Thread tid of 256 is SCU (tid & 15, tid >> 4) of the LCU at (X0, Y0).  -> the z-order index (of the top-left SCU) of the CU that
// holds this SCU, walking down from the LCU as set_cu_qps does: a node splits while the record at its top-left has a depth beyond
// the node's (a depth above 3 counts as 3).  The top-left of a node that holds an SCU of the picture lies inside the picture.
// first: the smallest such index among the SCUs of the picture with a non-zero flag, 256 if there is none.  All 256 threads call.
__device__ __forceinline__ int cu_of_scu(const cu_qp_args &a, int X0, int Y0, bool &inside, int &first, int *s_min)
{
  const int tid = threadIdx.x, ux = tid & 15, uy = tid >> 4;
  const int sx0 = X0 >> 2, sy0 = Y0 >> 2;
  inside = X0 + 4 * ux < a.width && Y0 + 4 * uy < a.height;
  int nx = 0, ny = 0, key = 256;
  if (inside) {
    int size = 16;
    for (int d = 0; d < 3; ++d) {
      const u32 head = a.cus[((size_t)(sy0 + ny) * a.cus_stride + sx0 + nx) * 5];
      if (min((int)((head >> 8) & 255u), 3) <= d) break;
      size >>= 1;
      if (ux >= nx + size) nx += size;
      if (uy >= ny + size) ny += size;
    }
    key = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) key |= (((nx >> b) & 1) << (2 * b)) | (((ny >> b) & 1) << (2 * b + 1));
  }
  const bool coded = inside && a.cbf[(size_t)(sy0 + uy) * a.cus_stride + sx0 + ux] != 0;
  const int m = wave_min(coded ? key : 256);
  if ((tid & 63) == 0) s_min[tid >> 6] = m;
  __syncthreads();
  first = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
  return key;
}

__global__ __launch_bounds__(256) void cu_qp_first_kernel(cu_qp_args a)
{
  __shared__ int s_min[4];
  const int lcu_x = blockIdx.x, lcu_y = blockIdx.y;
  bool inside;
  int first;
  cu_of_scu(a, 64 * lcu_x, 64 * lcu_y, inside, first, s_min);
  if (threadIdx.x == 0) {
    const size_t lcu = (size_t)lcu_y * a.lcus_x + lcu_x;
    a.lcu_last_qp[lcu] = (int8_t)(first < 256 ? clip_lcu_qp(a.lcu_qp[lcu]) : -1);
  }
}

// v[i] on entry: the QP that LCU i leaves as last_qp, or -1 if it leaves last_qp as it found it.  On return: last_qp on entry to
// LCU i.  "The last value that is not negative" is associative, so it scans.
__global__ __launch_bounds__(256) void cu_qp_chain_kernel(int8_t *v, int n_lcu, int chain_lcus, int start_qp)
{
  __shared__ int s_tot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int begin = blockIdx.x * chain_lcus, end = min(n_lcu, begin + chain_lcus);
  int carry = start_qp;
  for (int base = begin; base < end; base += 256) {
    const int i = base + tid;
    int incl = i < end ? (int)v[i] : -1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off && incl < 0) incl = t;
    }
    if (lane == 63) s_tot[wave] = incl;
    __syncthreads();
    int before = -1, total = -1;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int t = s_tot[w];
      if (t >= 0) {
        total = t;
        if (w < wave) before = t;
      }
    }
    int excl = __shfl_up(incl, 1, 64);
    if (lane == 0 || excl < 0) excl = before;
    if (i < end) v[i] = (int8_t)(excl >= 0 ? excl : carry);
    if (total >= 0) carry = total;
    __syncthreads();                                   // s_tot is written again
  }
}

__global__ __launch_bounds__(256) void cu_qp_write_kernel(cu_qp_args a)
{
  __shared__ int s_min[4];
  const int lcu_x = blockIdx.x, lcu_y = blockIdx.y, tid = threadIdx.x;
  bool inside;
  int first;
  const int key = cu_of_scu(a, 64 * lcu_x, 64 * lcu_y, inside, first, s_min);
  if (!inside) return;
  const size_t lcu = (size_t)lcu_y * a.lcus_x + lcu_x;
  const int qp = key < first ? (int)a.lcu_last_qp[lcu] : clip_lcu_qp(a.lcu_qp[lcu]);
  const size_t scu = (size_t)(16 * lcu_y + (tid >> 4)) * a.cus_stride + 16 * lcu_x + (tid & 15);
  ((u8 *)a.cus)[scu * 20 + 6] = (u8)qp;
}

}  // namespace

extern "C" {

int kvz_hip_cu_qp_frame(kvz_hip_cu_info *cus, const uint8_t *cbf, int width, int height, const int8_t *lcu_qp, int8_t *lcu_last_qp,
                        const kvz_hip_cu_qp_params *params, kvz_hip_stream s)
{
  KVZ_CHECK_CTX();
  if (!cus || !cbf || !lcu_qp || !lcu_last_qp || !params || ((uintptr_t)cus & 3)) return kvzhip::invalid_arg(__func__);
  if (width < 8 || height < 8 || ((width | height) & 7) || width > 16384 || height > 16384) return kvzhip::invalid_arg(__func__);
  const int lcus_x = (width + 63) >> 6, lcus_y = (height + 63) >> 6, n_lcu = lcus_x * lcus_y;
  if (params->start_qp < 0 || params->start_qp > 51 || params->chain_lcus < 0 || params->chain_lcus % lcus_x) return kvzhip::invalid_arg(__func__);
  const int chain = params->chain_lcus ? params->chain_lcus : n_lcu;
  cu_qp_args a;
  a.cus = (u32 *)cus; a.cbf = cbf; a.lcu_qp = lcu_qp; a.lcu_last_qp = lcu_last_qp;
  a.cus_stride = width >> 2; a.lcus_x = lcus_x;
  a.width = width; a.height = height;
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on width, height and chain_lcus alone
  hipLaunchKernelGGL(cu_qp_first_kernel, dim3((unsigned)lcus_x, (unsigned)lcus_y), dim3(256), 0, st, a);
  KVZ_CHECK_LAUNCH("cu_qp_first_kernel");
  hipLaunchKernelGGL(cu_qp_chain_kernel, dim3((unsigned)((n_lcu + chain - 1) / chain)), dim3(256), 0, st, lcu_last_qp, n_lcu, chain, params->start_qp);
  KVZ_CHECK_LAUNCH("cu_qp_chain_kernel");
  hipLaunchKernelGGL(cu_qp_write_kernel, dim3((unsigned)lcus_x, (unsigned)lcus_y), dim3(256), 0, st, a);
  KVZ_CHECK_LAUNCH("cu_qp_write_kernel");
  return KVZ_HIP_OK;
}

}  // extern "C"
