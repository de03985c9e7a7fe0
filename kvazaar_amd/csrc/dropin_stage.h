// dropin_stage.h -- the layout rules of the drop-in's staging buffer (strategy.hip), stated once.  Host only and free of HIP: a plain
// C++ compiler takes it, and tests/test_dropin_stage_host.py runs it under the sanitizers.
//
// A strategy call stages its operands in one buffer that exists twice with the same layout, in pinned host memory and in device
// memory (or once, when the kernels use the pinned buffer directly).  The rules:
//   - every slot begins on a 16-byte boundary (the batch entries refuse misaligned buffers);
//   - a call is a sequence of phases; within a phase the inputs are taken first and the outputs after them, so the inputs of a phase
//     are one contiguous byte range: the range to upload.  An input after an output is refused until next_phase();
//   - the range to download is the span from the first to the last of the output slots asked for;
//   - a take that would cross the capacity fails.  Nothing here aborts: the caller decides what a failure means.
// Only the slot handles carry a type.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace kvzhip {

constexpr size_t STAGE_ALIGN = 16;
inline size_t stage_align_up(size_t v) { return (v + STAGE_ALIGN - 1) & ~(STAGE_ALIGN - 1); }

struct stage_range { size_t off, bytes; };

// `count` elements of T at byte offset `off` of the staging buffer
template <typename T> struct stage_slot {
  size_t off = 0, count = 0;
  size_t bytes() const { return count * sizeof(T); }
  size_t end() const { return off + bytes(); }
  T *host(uint8_t *host_base) const { return (T *)(host_base + off); }
  T *dev(uint8_t *dev_base) const { return (T *)(dev_base + off); }
};

enum stage_status { STAGE_OK = 0, STAGE_OVERFLOW, STAGE_INPUT_AFTER_OUTPUT };

class stage_layout {
 public:
  explicit stage_layout(size_t capacity) : cap(capacity) {}

  template <typename T> stage_status in(size_t n, stage_slot<T> *s)
  {
    if (has_out) return STAGE_INPUT_AFTER_OUTPUT;
    if (!take(n, s)) return STAGE_OVERFLOW;
    if (!has_in) in_lo = s->off;
    has_in = true;
    in_hi = s->end();
    return STAGE_OK;
  }
  template <typename T> stage_status out(size_t n, stage_slot<T> *s)
  {
    if (!take(n, s)) return STAGE_OVERFLOW;
    has_out = true;
    return STAGE_OK;
  }
  // what follows may read what the device wrote so far: inputs may be taken again
  void next_phase() { has_in = has_out = false; in_lo = in_hi = off; }

  // the inputs of the current phase
  stage_range upload() const { return { in_lo, in_hi - in_lo }; }
  // the outputs first .. last, in the order they were taken
  template <typename A, typename B> static stage_range download(const stage_slot<A> &first, const stage_slot<B> &last)
  {
    return { first.off, last.end() - first.off };
  }

 private:
  template <typename T> bool take(size_t n, stage_slot<T> *s)
  {
    if (off > cap || n > (cap - off) / sizeof(T)) return false;
    s->off = off;
    s->count = n;
    off = stage_align_up(s->end());
    return true;
  }
  size_t cap, off = 0, in_lo = 0, in_hi = 0;
  bool has_in = false, has_out = false;
};

}  // namespace kvzhip
