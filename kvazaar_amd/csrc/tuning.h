// tuning.h -- the knobs of kvz_hip_set_tuning / KVZ_HIP_TUNE, declared once.  Host only and free of HIP: a plain C++ compiler takes
// it, and tests/test_tuning_host.py runs it under the sanitizers.
//
// KVZ_TUNE_KEYS is the one list: enumerator (the key string is its spelling), default, meaning.  The enum, the key names, the
// defaults and the override storage all come from it, and the comment above kvz_hip_set_tuning in include/kvz_hip.h is held to it by
// the same test.  A launcher reads a knob by enumerator -- an array index and a relaxed load, no string compare:
//   tuning<tune::sad_wgs_per_cu>()           the stored value, or the table's default when none (or a negative one) is stored
//   tuning_or<tune::dct_wgs_per_cu>(dflt)    the same for a key whose default belongs to the call site (TUNE_PER_SITE in the table)
//   tuning_is_set(tune::service_spin_us)     whether a value >= 0 is stored
// Taking the wrong one of the first two for a key does not compile.  A stored 0 is a value; any negative value means "default".
// Only kvz_hip_set_tuning and the KVZ_HIP_TUNE parser look a key up by name (tune_find).
#pragma once

#include <atomic>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

namespace kvzhip {

constexpr int TUNE_PER_SITE = INT_MIN;      // no default in the table: each reader passes its own to tuning_or()

// "*_wgs_per_cu": workgroups per CU that cap a streaming grid; 0 counts as 1 (wg_cap, stream_grid)
#define KVZ_TUNE_KEYS(X) \
  X(sad_wgs_per_cu,          256,           "SAD batch kernels") \
  X(satd8_wgs_per_cu,        256,           "8x8 SATD batch kernel") \
  X(dct32_wgs_per_cu,        4096,          "32x32 forward transform (one block per wave at any batch size)") \
  X(idct32_wgs_per_cu,       96,            "32x32 inverse transform") \
  X(dct_wgs_per_cu,          TUNE_PER_SITE, "LDS butterfly transforms; sites: 8x8 160, 16x16 48, other sizes 16") \
  X(qr32_wgs_per_cu,         8,             "32x32 matrix-core tile kernel of quantize_residual") \
  X(qr_wgs_per_cu,           TUNE_PER_SITE, "LDS butterfly quantize_residual; sites: 8x8 64, other sizes 16") \
  X(dct16_wgs_per_cu,        128,           "16x16 forward transform") \
  X(idct16_wgs_per_cu,       64,            "16x16 inverse transform") \
  X(qr16_wgs_per_cu,         8,             "16x16 matrix-core tile kernel of quantize_residual") \
  X(qr4_lane_kernel,         1,             "0: 4x4 quantize_residual on the LDS butterfly kernel instead of the lane kernel") \
  X(sao_edge_fast,           1,             "0: SAO edge statistics on the general kernel instead of the packed-accumulator one") \
  X(intra_rough_waves,       TUNE_PER_SITE, "waves per workgroup of the rough intra search; sites: 4x4 8, other sizes 4") \
  X(pair_wave_kernel,        1,             "0: frame-level pair batches of up to 4096 descriptors on the workgroup kernels, not a wave each") \
  X(qr4_wgs_per_cu,          96,            "4x4 lane kernel of quantize_residual") \
  X(quant_wgs_per_cu,        256,           "quant and dequant") \
  X(qr8_reg_kernel,          1,             "0: 8x8 quantize_residual on the LDS butterfly kernel instead of the register kernel") \
  X(qr8_wgs_per_cu,          TUNE_PER_SITE, "8x8 quantize_residual; sites: the matrix-core tile kernel 8, the register kernel 32") \
  X(qr_tile_kernel,          1,             "0: no matrix-core tile kernels for quantize_residual (32x32, 16x16, 8x8)") \
  X(dct4_tile,               1,             "0: 4x4 transforms on the LDS butterfly kernel instead of the tile kernel") \
  X(dct4_wgs_per_cu,         192,           "4x4 forward tile transform") \
  X(idct4_wgs_per_cu,        64,            "4x4 inverse tile transform") \
  X(wg_chunk_min_wgs,        4096,          "sampling / fractional search: up to 64 descriptors per workgroup once the list would give more workgroups than this; 0: always one") \
  X(pair_satd_threads,       256,           "threads per workgroup of the descriptor SATD kernel: a multiple of 64 from 64 to 512") \
  X(qr8_tile_kernel,         1,             "0: 8x8 TUs of quantize_residual on the register kernel instead of sixteen to a matrix-core tile") \
  X(qr_tile_pipe,            1,             "0: the tile kernels' wait on vector memory left to the compiler, not placed before the first store") \
  X(pipe,                    0,             "1: that hand placement in the 4x4 / 8x8 register kernels, where it measured slower") \
  X(dct_pipe,                0,             "1: that hand placement in the 32x32 transform, where it measured slower") \
  X(sample8_wave,            1,             "0: 8x8 luma blocks of the sampling entry on the general path") \
  X(full_qsad,               1,             "0: the service's exhaustive search prices with v_sad_u8 on aligned operands, not v_qsad_pk_u16_u8") \
  X(service_streams,         8,             "launch streams of the launch-per-batch way") \
  X(service_inflight,        4,             "batches in the air of the launch-per-batch way") \
  X(service_workers,         64,            "resident workgroups of the search service; 0: a launch per batch") \
  X(service_linger_us,       2000,          "how long the workers stay without work") \
  X(service_life_ms,         20,            "how long the workers stay at most") \
  X(service_spin_us,         TUNE_PER_SITE, "how long a caller polls before it naps; site: 100; set at all, it also switches the crowded waits off") \
  X(service_ticket_base_k,   0,             "tests: first ticket of the ring, times 1024") \
  X(service_push,            1,             "0: the workers read units from host memory even where a large BAR lets the host write device memory") \
  X(service_nap_us,          10,            "a nap of a caller that waits with more callers than cores") \
  X(service_spin_crowded_us, 5,             "how long such a caller polls before it naps") \
  X(event_fence,             0,             "release scope of the ABI's events: 0 none, 1 device, 2 (or more) system") \
  X(event_alias,             1,             "0: every event record is a packet of its own, none rides on the launch before it") \
  X(cost_store_nt,           1,             "0: the 8x8 SAD / SATD batch kernels store costs with the default cache policy, not nontemporal")

#define KVZ_TUNE_ENUM(name, dflt, doc) name,
enum class tune : int { KVZ_TUNE_KEYS(KVZ_TUNE_ENUM) count_ };
#undef KVZ_TUNE_ENUM
constexpr int TUNE_COUNT = (int)tune::count_;

#define KVZ_TUNE_KEY(name, dflt, doc) #name,
constexpr const char *tune_key[TUNE_COUNT] = { KVZ_TUNE_KEYS(KVZ_TUNE_KEY) };
#undef KVZ_TUNE_KEY
#define KVZ_TUNE_DEFAULT(name, dflt, doc) dflt,
constexpr int tune_default[TUNE_COUNT] = { KVZ_TUNE_KEYS(KVZ_TUNE_DEFAULT) };
#undef KVZ_TUNE_DEFAULT
// what kvz_hip_set_tuning stored per key; negative: nothing, the default holds
#define KVZ_TUNE_UNSET(name, dflt, doc) {-1},
inline std::atomic<int> tune_value[TUNE_COUNT] = { KVZ_TUNE_KEYS(KVZ_TUNE_UNSET) };
#undef KVZ_TUNE_UNSET

inline int tune_stored(tune k) { return tune_value[(int)k].load(std::memory_order_relaxed); }
inline bool tuning_is_set(tune k) { return tune_stored(k) >= 0; }

template <tune K> inline int tuning()
{
  static_assert(tune_default[(int)K] != TUNE_PER_SITE, "this key's default is per call site: tuning_or<key>(default)");
  const int v = tune_stored(K);
  return v >= 0 ? v : tune_default[(int)K];
}
template <tune K> inline int tuning_or(int dflt)
{
  static_assert(tune_default[(int)K] == TUNE_PER_SITE, "this key's default is in the table: tuning<key>()");
  const int v = tune_stored(K);
  return v >= 0 ? v : dflt;
}

// index of `key` in the table, -1 for NULL or a string that is no key
inline int tune_find(const char *key)
{
  if (!key) return -1;
  for (int i = 0; i < TUNE_COUNT; ++i) if (!std::strcmp(tune_key[i], key)) return i;
  return -1;
}

// KVZ_HIP_TUNE="key=value,key=value": split at ',' and at the first '=' of a pair, the value through atoi; a pair without '=' or with
// an unknown key is skipped, later pairs win.  `store` has TUNE_COUNT elements.
inline void tune_apply_env(const char *text, std::atomic<int> *store)
{
  const std::string all(text);
  size_t pos = 0;
  while (pos < all.size()) {
    size_t end = all.find(',', pos);
    if (end == std::string::npos) end = all.size();
    const std::string kv = all.substr(pos, end - pos);
    const size_t eq = kv.find('=');
    const int i = eq == std::string::npos ? -1 : tune_find(kv.substr(0, eq).c_str());
    if (i >= 0) store[i].store(std::atoi(kv.c_str() + eq + 1), std::memory_order_relaxed);
    pos = end + 1;
  }
}

}  // namespace kvzhip
