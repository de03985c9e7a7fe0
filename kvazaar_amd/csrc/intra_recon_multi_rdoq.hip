// intra_recon_multi_rdoq.hip -- kvz_hip_intra_recon_frames_rdoq: kvz_hip_intra_recon_frame_rdoq (intra_recon_rdoq.hip) for up to
// sixteen pictures that do not depend on each other, in one call.  With RDOQ a step of the wavefront holds the serial recursion of
// kvz_rdoq on one lane of every wave, and a launch of one picture is at most a wave per LCU row and plane: the rest of the device idles
// for exactly that time.  Here launch t holds wave t of every tile of every picture, as in intra_recon_multi_ts.hip, and the call makes
// as many dependent launches as the largest tile of any picture alone.
//
// The kernels are the two instantiations of intra_recon_core.h whose argument is the table of per-picture records with the pool of
// tile boundaries and the call's RDOQ tables (intra_batch_rdoq<SL>): flat lists or tables; behind them init_pictures_kernel
// (frame_sources.h) on the same table.  A wave builds its rdoq_source from its picture's record -- every picture has its own context
// sets, states and set index per LCU -- and stages that picture's set of its LCU (rdoq_lcu<true>::stage); from there on it is the
// single-picture kernel, hence the same bytes.  The kernels have this translation unit to themselves, so that the other kernels are
// compiled as they always were, and it is compiled with -ffp-contract=off (Makefile) as rdoq.hip is.  The records are checked, the
// pool filled and the launches sized by the walk that the six multi-picture entries of the residual stages share (chain_records_why,
// chain_host.h).
#include "rdoq_stage.h"
#include "intra_recon_core.h"

#pragma clang fp contract(off)

namespace {

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
  chain_tiles tiles;
  chain_plan plan;
  int at;
  // every record is checked before anything is launched: a refused call writes nothing
  if (const char *why = chain_records_why(pictures, n_pictures, true, &tiles, &plan, &at)) return refuse_picture(__func__, at, why);
  const kvz_hip_rdoq_source *first = pictures[0].rdoq;                          // not NULL: some record carries one and the call is homogeneous
  const bool lists = pictures[0].tables.quant || pictures[0].tables.dequant;
  intra_batch_rdoq_data b;
  __builtin_memset(&b, 0, sizeof b);
  for (int i = 0; i < n_pictures; ++i) {
    const kvz_hip_chain_picture_rdoq &r = pictures[i];
    fill(b.p[i], r.pic, clip_lcu_qp(r.pic.params.qp));                          // the single-picture entry clamps the picture's QP too
    fill_lists(b.p[i], r.tables);
    fill_rdoq(b.p[i], *r.rdoq);
    fill_tiles(b.p[i], r.grid, tiles.pic[i]);
  }
  tile_pool_pack(tiles.bounds, tiles.used, b.bd);
  b.quant = first->tables.quant; b.err_scale = first->tables.err_scale; b.skip = first->rdoq_skip != 0;
  hipStream_t st = ctx_stream(s);
  // the launch sequence depends on the sizes, the chroma flags, the grids and the presence of cbf_out / costs alone
  if (int e = init_pictures<intra_cu_rule>(b, plan.init_scus, n_pictures, st)) return e;
  const dim3 grid((unsigned)plan.groups, (unsigned)plan.planes, (unsigned)n_pictures);
  return lists ? launch_waves<true>(b, plan.waves, grid, st) : launch_waves<false>(b, plan.waves, grid, st);
}

}  // extern "C"
