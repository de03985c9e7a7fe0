/*
 * ref_quant_rdoq.c -- glue that runs the COMPILED REFERENCE's kvz_quantize_residual (quant-generic.c:180-273, or the variant the
 * reference's strategy selector picked) on one TU with cfg.rdoq_enable = 1, so that the reference itself decides between kvz_rdoq and
 * kvz_quant (:214-225) and derives tr_depth from the cu_info_t it is handed (:218-219).  TEST INFRASTRUCTURE ONLY; this file contains
 * no reference code, it calls it through the reference's own headers and links against oracle/_ref/libkvzref.so
 * (tests/ref_quant_rdoq.py compiles it; the library is loaded and its strategies selected before anything here runs).
 *
 * The state is fabricated as in ref_rdoq.c: zeroed structures, kvz_scalinglist_init / kvz_scalinglist_process for the flat or the default
 * lists, the context bytes, lambda and QP copied in by the caller; on top of it the slice type that kvz_quant reads of the frame,
 * cfg.rdoq_enable = 1, cfg.rdoq_skip and cfg.signhide_enable, and a cu_info_t carrying type, depth, tr_depth and part_size.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cabac.h"
#include "context.h"
#include "cu.h"
#include "encoder.h"
#include "encoderstate.h"
#include "rdo.h"
#include "scalinglist.h"
#include "strategies/strategies-quant.h"

static encoder_control_t g_ctrl[2];      /* [0] flat lists, [1] the default lists */
static int g_ready[2];
static encoder_state_t g_state;
static encoder_state_config_frame_t g_frame;

static encoder_control_t *ctrl(int default_lists)
{
  encoder_control_t *c = &g_ctrl[default_lists ? 1 : 0];
  if (!g_ready[default_lists ? 1 : 0]) {
    memset(c, 0, sizeof(*c));
    c->bitdepth = 8;
    kvz_scalinglist_init(&c->scaling_list);
    if (default_lists) { c->scaling_list.enable = 1; c->scaling_list.use_default_list = 1; }
    kvz_scalinglist_process(&c->scaling_list, 8);
    g_ready[default_lists ? 1 : 0] = 1;
  }
  return c;
}

int quant_rdoq_ref_ctx_bytes(void) { return (int)sizeof(g_state.cabac.ctx); }

/* cfg: { rdoq_enable, rdoq_skip, signhide, default_lists, slice_is_intra }; cu: { type, depth, tr_depth, part_size };
 * tu: { width, color, scan_order }.  ref_in, pred_in, rec_out: width * width pixels, stride width.  -> has_coeffs */
int quant_rdoq_ref_run(const uint8_t *ctx, double lambda, int qp, const int32_t *cfg, const int32_t *cu_fields, const int32_t *tu,
                       const uint8_t *ref_in, const uint8_t *pred_in, uint8_t *rec_out, int16_t *coeff_out)
{
  encoder_control_t *c = ctrl(cfg[3]);
  const int width = tu[0];
  kvz_pixel ref[32 * 32] __attribute__((aligned(64))), pred[32 * 32] __attribute__((aligned(64))), rec[32 * 32] __attribute__((aligned(64)));
  coeff_t out[32 * 32] __attribute__((aligned(64)));
  cu_info_t cu;
  c->cfg.rdoq_enable = cfg[0];
  c->cfg.rdoq_skip = cfg[1];
  c->cfg.signhide_enable = cfg[2];
  memset(&g_state, 0, sizeof(g_state));
  memset(&g_frame, 0, sizeof(g_frame));
  g_frame.slicetype = cfg[4] ? KVZ_SLICE_I : KVZ_SLICE_P;
  g_state.encoder_control = c;
  g_state.frame = &g_frame;
  g_state.lambda = lambda;
  g_state.qp = (int8_t)qp;
  memcpy(&g_state.cabac.ctx, ctx, sizeof(g_state.cabac.ctx));
  memset(&cu, 0, sizeof(cu));
  cu.type = (uint8_t)cu_fields[0];
  cu.depth = (uint8_t)cu_fields[1];
  cu.tr_depth = (uint8_t)cu_fields[2];
  cu.part_size = (uint8_t)cu_fields[3];
  memcpy(ref, ref_in, (size_t)width * width);
  memcpy(pred, pred_in, (size_t)width * width);
  memcpy(rec, rec_out, (size_t)width * width);
  memcpy(out, coeff_out, sizeof(coeff_t) * width * width);
  const int has = kvz_quantize_residual(&g_state, &cu, width, (color_t)tu[1], (coeff_scan_order_t)tu[2], 0, width, width, ref, pred, rec, out);
  memcpy(rec_out, rec, (size_t)width * width);
  memcpy(coeff_out, out, sizeof(coeff_t) * width * width);
  return has;
}
