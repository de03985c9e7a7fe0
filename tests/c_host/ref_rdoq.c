/*
 * ref_rdoq.c -- glue that runs the COMPILED REFERENCE's kvz_rdoq (rdo.c:548-881) on one TU.  TEST INFRASTRUCTURE ONLY; this file
 * contains no reference code, it calls it through the reference's own headers and links against oracle/_ref/libkvzref.so, which
 * exports kvz_rdoq, kvz_scalinglist_init / _process, kvz_init_contexts and kvz_entropy_bits (tests/ref_rdoq.py compiles it).
 *
 * kvz_rdoq has no caller-independent entry in the reference, but it reads of its encoder_state_t only lambda, qp, cabac.ctx and,
 * through encoder_control, bitdepth, scaling_list and cfg.signhide_enable.  So the state here is fabricated the way
 * oracle/ref_harness.c:48-55 fabricates one: zeroed structures, kvz_scalinglist_init / kvz_scalinglist_process for quant_coeff and
 * error_scale (flat lists, or scaling_list.enable = use_default_list = 1 for the default lists and a non-uniform error_scale),
 * and the context bytes copied in by the caller.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cabac.h"
#include "context.h"
#include "encoder.h"
#include "encoderstate.h"
#include "rdo.h"
#include "scalinglist.h"

static encoder_control_t g_ctrl[2];      /* [0] flat lists, [1] the default lists */
static int g_ready[2];
static encoder_state_t g_state;

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

int rdoq_ref_ctx_bytes(void) { return (int)sizeof(g_state.cabac.ctx); }

/* what byte of the context block a model lies at: 0 root cbf, 1 qt cbf luma, 2 qt cbf chroma, 3 sig coeff group */
int rdoq_ref_ctx_offset(int which)
{
  const uint8_t *base = (const uint8_t *)&g_state.cabac.ctx;
  switch (which) {
    case 0: return (int)((const uint8_t *)&g_state.cabac.ctx.cu_qt_root_cbf_model - base);
    case 1: return (int)((const uint8_t *)&g_state.cabac.ctx.qt_cbf_model_luma[0] - base);
    case 2: return (int)((const uint8_t *)&g_state.cabac.ctx.qt_cbf_model_chroma[0] - base);
    default: return (int)((const uint8_t *)&g_state.cabac.ctx.cu_sig_coeff_group_model[0] - base);
  }
}

/* kvz_init_contexts (context.c:209) for a slice type (0 B, 1 P, 2 I) and QP: the whole context block */
void rdoq_ref_init_contexts(int qp, int slice, uint8_t *out)
{
  memset(&g_state, 0, sizeof(g_state));
  kvz_init_contexts(&g_state, (int8_t)qp, (int8_t)slice);
  memcpy(out, &g_state.cabac.ctx, sizeof(g_state.cabac.ctx));
}

void rdoq_ref_run(const uint8_t *ctx, double lambda, int qp, int signhide, int default_lists, const int16_t *coef, int16_t *dest,
                  int width, int type, int scan_mode, int block_type, int tr_depth)
{
  encoder_control_t *c = ctrl(default_lists);
  coeff_t in[32 * 32] __attribute__((aligned(64))), out[32 * 32] __attribute__((aligned(64)));
  c->cfg.signhide_enable = signhide;
  memset(&g_state, 0, sizeof(g_state));
  g_state.encoder_control = c;
  g_state.lambda = lambda;
  g_state.qp = (int8_t)qp;
  memcpy(&g_state.cabac.ctx, ctx, sizeof(g_state.cabac.ctx));
  memcpy(in, coef, sizeof(coeff_t) * width * width);
  memcpy(out, dest, sizeof(coeff_t) * width * width);          /* the caller's fill shows what kvz_rdoq does not write */
  kvz_rdoq(&g_state, in, out, width, width, (int8_t)type, (int8_t)scan_mode, (int8_t)block_type, (int8_t)tr_depth);
  memcpy(dest, out, sizeof(coeff_t) * width * width);
}

const int32_t *rdoq_ref_quant_table(int default_lists, int size_id, int list, int rem)
{ return ctrl(default_lists)->scaling_list.quant_coeff[size_id][list][rem]; }

const double *rdoq_ref_err_table(int default_lists, int size_id, int list, int rem)
{ return ctrl(default_lists)->scaling_list.error_scale[size_id][list][rem]; }

uint32_t rdoq_ref_entropy_bits(int i) { return kvz_entropy_bits[i & 127]; }
