// rdoq_host.h -- the host side of kvz_hip_rdoq_batch: what the entry requires of its arguments.
// Host only, as coeff_cost_host.h is: pointers are compared and never followed (tables and params are HOST structs and are read),
// so a plain C++17 compiler takes this header with kvz_hip.h alone (tests/test_rdoq_abi.py runs it that way).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kvz_hip.h"

namespace {

static_assert(sizeof(kvz_hip_rdoq_tables) == 16 && sizeof(kvz_hip_rdoq_state) == 24 && sizeof(kvz_hip_rdoq_desc) == 16 &&
              sizeof(kvz_hip_rdoq_params) == 16, "layout documented in kvz_hip.h");

// kvz_hip_rdoq_batch with n > 0: why the call is refused, or nullptr
inline const char *rdoq_batch_why(const kvz_hip_coeff *coef, const kvz_hip_coeff *dest, const kvz_hip_rdoq_desc *descs, size_t n,
                                  const kvz_hip_coeff_ctx *ctx_sets, const kvz_hip_rdoq_state *states, uint32_t n_sets,
                                  const kvz_hip_rdoq_tables *tables, const kvz_hip_rdoq_params *params)
{
  if (!coef || !dest || !descs || !ctx_sets || !states || !tables || !params) return "a pointer is null";
  if (!tables->quant || !tables->err_scale) return "a table is null";
  if (n_sets == 0) return "n_sets is 0";
  if (n > 0x7fffffffu) return "n above 2^31 - 1";
  if (((uintptr_t)coef & 7) || ((uintptr_t)dest & 7) || ((uintptr_t)descs & 3) || ((uintptr_t)ctx_sets & 1) || ((uintptr_t)states & 7))
    return "coef, dest or states not 8-byte, descs not 4-byte or ctx_sets not 2-byte aligned";
  if (((uintptr_t)tables->quant & 15) || ((uintptr_t)tables->err_scale & 7)) return "quant not 16-byte or err_scale not 8-byte aligned";
  return nullptr;
}

}  // namespace
