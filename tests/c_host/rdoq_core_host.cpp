// rdoq_core_host.cpp -- kvazaar_amd/csrc/rdoq_core.h run as a host program: the arithmetic the RDOQ kernels execute, compiled for the CPU.
// TEST INFRASTRUCTURE (tests/test_rdoq_model.py).  The test copies rdoq_core.h, coeff_cabac_core.h and cabac_tables.h next to a stub
// kvz_hip_internal.h that defines the few device words they use (__device__, __constant__, __clz, ...) and builds this file with
// -ffp-contract=off; one thread plays every lane in turn, with the arrays contiguous (a wave's TU) or lane-interleaved (a lane's 4x4 TU).
#include "rdoq_core.h"
using namespace kvzhip;
static int scaled_qp(int type, int qp)
{
  const unsigned char chroma_scale[58] = {
     0, 1, 2, 3, 4, 5, 6, 7, 8, 9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,29,30,31,32,
    33,33,34,34,35,35,36,36,37,37,38,39,40,41,42,43,44,45,46,47,48,49,50,51 };
  if (type == 0) return qp;
  int q = qp < 0 ? 0 : (qp > 57 ? 57 : qp);
  return chroma_scale[q];
}
template <int S>
static void run(const i16 *coef, i16 *dest, int width, int type, int scan_mode, int block_type, int tr_depth, int qp, double lambda,
                const u8 *ctx136, const u8 *state9, const i32 *quant, const double *err_scale, int signhide)
{
  const int n2 = width * width, off = S == 1 ? 0 : 5;
  std::vector<double> c0(n2 * S, -1e300), cc(n2 * S, -1e300), cs(n2 * S, -1e300), cg(64 * S, -1e300);
  std::vector<i32> ld(n2 * S, 12345678), sig(n2 * S, 12345678), inc(n2 * S, 12345678), dec(n2 * S, 12345678), qd(n2 * S, 12345678), lx(12 * S), ly(12 * S);
  std::vector<i16> dst(n2 * S, 0x5a5a), cf(n2 * S);
  for (int i = 0; i < n2; ++i) cf[i * S + off] = coef[i];
  rdoq_mem<S> m = { c0.data() + off, cc.data() + off, cs.data() + off, cg.data() + off, ld.data() + off, sig.data() + off, inc.data() + off, dec.data() + off,
                    qd.data() + off, lx.data() + off, ly.data() + off, dst.data() + off, cf.data() + off };
  rdoq_tu t;
  t.log2w = width == 4 ? 2 : width == 8 ? 3 : width == 16 ? 4 : 5;
  t.type = type; t.scan_mode = scan_mode; t.intra = block_type == 1; t.tr_depth = tr_depth;
  t.qp_scaled = scaled_qp(type, qp);
  t.q_bits = 14 + t.qp_scaled / 6 + (15 - 8 - t.log2w);
  t.signhide = signhide; t.lambda = lambda;
  rdoq_ctx ctx = { ctx136, state9 };
  rdoq_scan sc = rdoq_make_scan(t.log2w, scan_mode);
  int last = -1;
  for (int s = 0; s < n2; ++s) { const int blk = sc.blk(s); if (rdoq_prepare(m, blk, quant[blk], err_scale[blk], t.q_bits) > 0) last = s; }
  int best = 0;
  if (last >= 0) best = rdoq_recursion(m, ctx, sc, t, err_scale, last);
  u32 abs_sum = 0;
  for (int s = 0; s < n2; ++s) abs_sum += rdoq_finish(m, sc.blk(s), s, best);
  if (signhide && abs_sum >= 2) {
    const int last_cg = (best - 1) >> 4;
    // every group from the same state, as lanes would: groups are independent
    for (int g = 0; g <= last_cg; ++g) rdoq_sign_hide_group(m, sc, g, last_cg, rdoq_rd_factor(t.qp_scaled, lambda));
  }
  for (int i = 0; i < n2; ++i) dest[i] = dst[i * S + off];
}
extern "C" void rdoq_core_host(int strided, const i16 *coef, i16 *dest, int width, int type, int scan_mode, int block_type, int tr_depth, int qp, double lambda,
                         const u8 *ctx136, const u8 *state9, const i32 *quant, const double *err_scale, int signhide)
{
  if (strided) run<64>(coef, dest, width, type, scan_mode, block_type, tr_depth, qp, lambda, ctx136, state9, quant, err_scale, signhide);
  else run<1>(coef, dest, width, type, scan_mode, block_type, tr_depth, qp, lambda, ctx136, state9, quant, err_scale, signhide);
}
