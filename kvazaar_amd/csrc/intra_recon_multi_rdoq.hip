// intra_recon_multi_rdoq.hip -- kvz_hip_intra_recon_frames_rdoq: kvz_hip_intra_recon_frame_rdoq (intra_recon_rdoq.hip) for up to
// sixteen pictures that do not depend on each other, in one call.  With RDOQ a step of the wavefront holds the serial recursion of
// kvz_rdoq on one lane of every wave, and a launch of one picture is at most a wave per LCU row and plane: the rest of the device idles
// for exactly that time.  Here launch t holds wave t of every tile of every picture, as in intra_recon_multi_ts.hip, and the call makes
// as many dependent launches as the largest tile of any picture alone.
//
// The kernels are the two instantiations of intra_recon_core.h whose argument is the table of per-picture records with the pool of
// tile boundaries and the call's RDOQ tables (intra_batch_rdoq<SL>): flat lists or tables.  A wave builds its rdoq_source from its
// picture's record -- every picture has its own context sets, states and set index per LCU -- and stages that picture's set of its LCU
// (rdoq_lcu<true>::stage); from there on it is the single-picture kernel, hence the same bytes.  The kernels have this translation
// unit to themselves, so that the other kernels are compiled as they always were, and it is compiled with -ffp-contract=off
// (Makefile) as rdoq.hip is.
#include "rdoq_stage.h"
#include "intra_recon_core.h"

#pragma clang fp contract(off)

namespace {

// intra_recon_init_kernel for every picture that has cbf_out or costs: grid (blocks of the largest such picture, pictures)
__global__ __launch_bounds__(256) void intra_recon_init_multi_rdoq_kernel(intra_batch_rdoq_data b)
{
  const intra_pic_rdoq &a = b.p[blockIdx.y];
  if (!a.cbf_out && !a.cost) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cus_stride * (a.height >> 2)) return;
  zero_cu_outputs(a, i, intra_cu_rule());
}

template <bool SL>
int launch_waves(const intra_batch_rdoq_data &d, int waves, dim3 grid, hipStream_t st)
{
  intra_batch_rdoq<SL> b;
  static_cast<intra_batch_rdoq_data &>(b) = d;
  for (int t = 0; t < waves; ++t) {
    hipLaunchKernelGGL((intra_recon_wave_kernel<intra_batch_rdoq<SL>>), grid, dim3(WG), 0, st, b, t);
    KVZ_CHECK_LAUNCH("intra_recon_wave_kernel");
  }
  return KVZ_HIP_OK;
}

}  // namespace

extern "C" {

int kvz_hip_intra_recon_frames_rdoq(const kvz_hip_chain_picture_rdoq *pictures, int n_pictures, kvz_hip_stream s)
{
  KVZ_CHAIN_PROLOGUE(pictures, n_pictures);
  bool any = false;
  for (int i = 0; i < n_pictures; ++i) any = any || pictures[i].rdoq;
  if (!any) {
    // no record carries rdoq: the entry without it on the same fields, launching that entry's kernels
    kvz_hip_chain_picture_ts plain[KVZ_HIP_MAX_CHAIN_PICTURES];
    for (int i = 0; i < n_pictures; ++i) plain[i] = { pictures[i].pic, pictures[i].grid, pictures[i].tables, nullptr, nullptr };
    return kvz_hip_intra_recon_frames_ts(plain, n_pictures, s);
  }
  const kvz_hip_rdoq_source *first = pictures[0].rdoq;
  const bool lists = pictures[0].tables.quant || pictures[0].tables.dequant, skip = first && first->rdoq_skip != 0;
  intra_batch_rdoq_data b;
  __builtin_memset(&b, 0, sizeof b);
  uint16_t bounds[KVZ_HIP_CHAIN_TILE_BOUNDS];
  int waves = 0, groups = 0, planes = 1, init_scus = 0, used = 0;
  // every record is checked before anything is launched: a refused call writes nothing
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture_rdoq &r = pictures[i];
    const kvz_hip_chain_picture &p = r.pic;
    // homogeneity and the record's own checks, its grid and the grid's place in the pool, then the outputs of the earlier records: the
    // order decides which reason a record with two defects reports
    const char *why = chain_record_rdoq_why(pictures, i, true, lists, skip);
    kvz_hip_tile_grid g;
    pic_tiles t;
    if (!why && !tile_grid_make(r.grid, p.src.width, p.src.height, &g)) why = "invalid tile grid";
    if (!why && !tile_pool_add(r.grid, g, bounds, used, &t)) why = "the tile grids of the call exceed KVZ_HIP_CHAIN_TILE_BOUNDS boundaries at this record";
    if (!why) why = chain_record_rdoq_shared(pictures, i);
    if (why) return refuse_picture(__func__, i, why);
    intra_pic_rdoq &a = b.p[i];
    fill(a, p, clip_lcu_qp(p.params.qp));                                     // the single-picture entry clamps the picture's QP too
    if (lists) { a.quant = r.tables.quant; a.dequant = r.tables.dequant; }
    // (record 0 without rdoq passes its own checks; the call is then refused at the first record that carries one)
    if (r.rdoq) { a.sets = r.rdoq->ctx_sets; a.states = r.rdoq->states; a.lcu_ctx = r.rdoq->lcu_ctx; a.n_sets = r.rdoq->n_sets; }
    // the kernel reads cols == 0 as "no grid": a picture without one keeps the zeros, where pic_tiles says one tile
    if (r.grid) { a.cols = t.cols; a.rows = t.rows; a.col_at = t.col_at; a.row_at = t.row_at; }
    waves = max(waves, tile_grid_waves(g));
    groups = max(groups, (int)t.lcus_y * g.cols);
    if (a.chroma) planes = 3;
    if (p.cbf_out || p.costs) init_scus = max(init_scus, (a.width >> 2) * (a.height >> 2));
  }
  tile_pool_pack(bounds, used, b.bd);
  b.quant = first->tables.quant; b.err_scale = first->tables.err_scale; b.skip = skip;
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags, the grids and the presence of cbf_out / costs alone
  if (init_scus) {
    hipLaunchKernelGGL(intra_recon_init_multi_rdoq_kernel, dim3((unsigned)((init_scus + 255) / 256), (unsigned)n_pictures), dim3(256), 0, st, b);
    KVZ_CHECK_LAUNCH("intra_recon_init_multi_rdoq_kernel");
  }
  const dim3 grid((unsigned)groups, (unsigned)planes, (unsigned)n_pictures);
  return lists ? launch_waves<true>(b, waves, grid, st) : launch_waves<false>(b, waves, grid, st);
}

}  // extern "C"
