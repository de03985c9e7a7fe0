"""CPU: the staging layout of the drop-in (kvazaar_amd/csrc/dropin_stage.h) without a device.

strategy.hip stages every strategy call's operands through one buffer and copies, with KVZ_HIP_ZEROCOPY=0, one byte range up and one
down.  The ranges follow from the slots that a function takes; this program holds them to that.  It is a stand-alone C++ program that
includes the header alone, compiled with the address and undefined-behaviour sanitizers (their runtimes linked statically, so that the
program does not depend on what else the process has loaded) and run as a child process.  A "host" and a "device" buffer of exactly
the capacity live on the heap, so a slot or a range one byte too long is an AddressSanitizer report.  Every element of every input
slot is written through the slot's typed host pointer, the upload range is copied, and the typed device pointer must read the same;
a stand-in for the kernel writes every element of every output slot through the device pointer, the download range is copied, and the
host pointer must read that.  The byte behind an upload range must not have been copied.

The walks take the slot sequences of the real functions with sizes from their bodies as literals.  Beside each derived range the
program prints the range that the hand-kept arithmetic of strategy.hip gave before the layout existed (`by hand`: offsets bumped by
sizes rounded up to 16; the lines of each function restated in the walk).  Both begin at the same byte.  Where that code wrote
a byte count (`d2h(oc, 4)`) the lengths are equal; where it took the bump offset (`in_end`, `out_end - first`) its range also
covers the padding behind the last slot, at most 15 bytes, which no kernel reads and no caller gets: there the derived end,
rounded up to 16, is the old one."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <map>
#include <vector>

#include "dropin_stage.h"

using namespace kvzhip;

// the staging as strategy.hip kept it by hand
struct by_hand {
  size_t off = 0;
  size_t take(size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; }
};

// both buffers, of exactly the capacity
struct buffers {
  size_t cap;
  uint8_t *h, *d;
  explicit buffers(size_t c) : cap(c), h((uint8_t *)malloc(c)), d((uint8_t *)malloc(c)) { memset(h, 0xEE, c); memset(d, 0xDD, c); }
  ~buffers() { free(h); free(d); }
};

template <typename T> static T value(unsigned seed, size_t i) { return (T)(seed * 131u + (unsigned)i * 7u + 1u); }

// one call: a layout over the buffers, every slot written and read through its handle
struct walk {
  const char *name;
  buffers &b;
  stage_layout lay;
  unsigned seed = 0;
  bool ok = true;
  std::vector<std::function<bool()>> uploaded;      // per input of the phase: does the device pointer read what the host pointer wrote
  std::vector<std::function<void()>> kernel;        // per output so far: write it through the device pointer
  std::map<size_t, unsigned> seeds;                 // offset of a slot -> the seed of its contents

  walk(const char *n, buffers &bufs) : name(n), b(bufs), lay(bufs.cap) {}

  template <typename T> stage_slot<T> in(size_t n)
  {
    stage_slot<T> s;
    if (lay.in(n, &s) != STAGE_OK) { ok = false; return s; }
    const unsigned sd = seeds[s.off] = ++seed;
    T *p = s.host(b.h);
    for (size_t i = 0; i < s.count; ++i) p[i] = value<T>(sd, i);
    uint8_t *dev = b.d;
    uploaded.push_back([s, sd, dev] { const T *q = s.dev(dev); for (size_t i = 0; i < s.count; ++i) if (q[i] != value<T>(sd, i)) return false; return true; });
    return s;
  }
  template <typename T> stage_slot<T> out(size_t n)
  {
    stage_slot<T> s;
    if (lay.out(n, &s) != STAGE_OK) { ok = false; return s; }
    const unsigned sd = seeds[s.off] = ++seed;
    uint8_t *dev = b.d;
    kernel.push_back([s, sd, dev] { T *q = s.dev(dev); for (size_t i = 0; i < s.count; ++i) q[i] = value<T>(sd, i); });
    return s;
  }
  void report(const char *what, stage_range r, size_t hand_off, size_t hand_bytes)
  {
    printf("%s: %s %zu+%zu", name, what, r.off, r.bytes);
    if (hand_bytes != SIZE_MAX) printf(" by hand %zu+%zu", hand_off, hand_bytes);
    printf("\n");
  }
  void upload(size_t hand_off = 0, size_t hand_bytes = SIZE_MAX)
  {
    const stage_range r = lay.upload();
    memcpy(b.d + r.off, b.h + r.off, r.bytes);
    for (auto &f : uploaded) ok = ok && f();
    uploaded.clear();
    if (r.off + r.bytes < b.cap && b.d[r.off + r.bytes] != 0xDD) ok = false;       // nothing behind the inputs was copied
    report("upload", r, hand_off, hand_bytes);
  }
  void launch() { for (auto &f : kernel) f(); }
  template <typename A, typename B> void download(stage_slot<A> first, stage_slot<B> last, size_t hand_off = 0, size_t hand_bytes = SIZE_MAX)
  {
    const stage_range r = stage_layout::download(first, last);
    memcpy(b.h + r.off, b.d + r.off, r.bytes);
    report("download", r, hand_off, hand_bytes);
  }
  // after a download: the host pointer reads what the kernel wrote
  template <typename T> void got(stage_slot<T> s)
  {
    const unsigned sd = seeds[s.off];
    const T *p = s.host(b.h);
    for (size_t i = 0; i < s.count; ++i) if (p[i] != value<T>(sd, i)) ok = false;
  }
  void next_phase() { lay.next_phase(); }
  void done() { printf("%s: %s\n", name, ok ? "bytes ok" : "BYTES DIFFER"); }
};

// ---- slots of 1, 4, 15, 16, 17 and 4097 bytes, and typed ones ----
static void slot_cases()
{
  buffers b(1u << 20);
  walk w("slots", b);
  const size_t sizes[6] = { 1, 4, 15, 16, 17, 4097 };
  stage_slot<uint8_t> s[6];
  bool apart = true;
  for (int i = 0; i < 6; ++i) {
    s[i] = w.in<uint8_t>(sizes[i]);
    printf("slot of %zu bytes: at %zu\n", sizes[i], s[i].off);
    if (s[i].off % 16 || (i && s[i].off < s[i - 1].end())) apart = false;
  }
  stage_slot<int16_t> a = w.in<int16_t>(17);
  stage_slot<int32_t> c = w.in<int32_t>(5);
  stage_slot<uint64_t> e = w.in<uint64_t>(1);
  stage_slot<uint32_t> o1 = w.out<uint32_t>(1);
  stage_slot<int16_t> o2 = w.out<int16_t>(3);
  printf("int16 x 17: at %zu, %zu bytes; int32 x 5: at %zu, %zu bytes; uint64 x 1: at %zu; outputs at %zu and %zu\n", a.off, a.bytes(), c.off, c.bytes(), e.off,
         o1.off, o2.off);
  if (a.off % 16 || c.off % 16 || e.off % 16 || o1.off % 16 || o2.off % 16 || a.off < s[5].end() || c.off < a.end() || e.off < c.end() || o1.off < e.end() ||
      o2.off < o1.end())
    apart = false;
  printf("slots: %s\n", apart ? "16-byte aligned and apart" : "MISPLACED");
  w.upload();
  w.launch();
  w.download(o1, o2);
  w.got(o1); w.got(o2);
  w.done();
}

// ---- the slot sequences of the real functions ----
// hip_quantize_residual, plain route: [quant and dequant tables of w*w int32,] ref and pred of w*w pixels in; rec, w*w coefficients and `has` out
static void walk_quantize_residual(const char *name, size_t w, bool tables)
{
  buffers b(1u << 20);
  walk k(name, b);
  by_hand s;
  if (tables) { s.take(w * w * 4); s.take(w * w * 4); }
  s.take(w * w); s.take(w * w);
  const size_t in_end = s.off, ore = s.take(w * w);
  s.take(w * w * 2); s.take(4);
  const size_t out_end = s.off;

  if (tables) { k.in<int32_t>(w * w); k.in<int32_t>(w * w); }
  k.in<uint8_t>(w * w); k.in<uint8_t>(w * w);
  auto rec = k.out<uint8_t>(w * w);
  auto coef = k.out<int16_t>(w * w);
  auto has = k.out<int32_t>(1);
  k.upload(0, in_end);
  k.launch();
  k.download(rec, has, ore, out_end - ore);
  k.got(rec); k.got(coef); k.got(has);
  k.done();
}

// hip_quantize_residual, RDOQ route: ref and pred in, residual and coefficients out, the coefficients down; then the levels of the
// host's kvz_rdoq in, dequantised coefficients and rec out, rec down
static void walk_quantize_residual_rdoq(const char *name, size_t w)
{
  buffers b(1u << 20);
  walk k(name, b);
  const size_t n = w * w;
  by_hand s;
  s.take(n); s.take(n);
  const size_t in_end = s.off;
  s.take(n * 2);
  const size_t oco = s.take(n * 2);

  k.in<uint8_t>(n); k.in<uint8_t>(n);
  k.out<int16_t>(n);
  auto coef = k.out<int16_t>(n);
  k.upload(0, in_end);
  k.launch();
  k.download(coef, coef, oco, n * 2);
  k.got(coef);

  const size_t oq = s.take(n * 2), q_end = s.off;
  s.take(n * 2);
  const size_t ore = s.take(n);
  k.next_phase();
  k.in<int16_t>(n);
  k.out<int16_t>(n);
  auto rec = k.out<uint8_t>(n);
  k.upload(oq, q_end - oq);
  k.launch();
  k.download(rec, rec, ore, n);
  k.got(rec);
  k.done();
}

// hip_filter_step: the (w + 9) x (h + 8) window in; four filtered blocks, two rows of horizontal intermediates and their first columns out
static void walk_filter_step(const char *name, size_t w, size_t h)
{
  buffers b(1u << 20);
  walk k(name, b);
  const size_t ph = h + 8, pw = w + 9;
  by_hand s;
  s.take(pw * ph);
  const size_t in_end = s.off, of = s.take(4 * w * h);
  s.take(2 * ph * w * 2); s.take(2 * ph * 2);
  const size_t out_end = s.off;

  k.in<uint8_t>(pw * ph);
  auto filt = k.out<uint8_t>(4 * w * h);
  auto hor = k.out<int16_t>(2 * ph * w);
  auto cols = k.out<int16_t>(2 * ph);
  k.upload(0, in_end);
  k.launch();
  k.download(filt, cols, of, out_end - of);
  k.got(filt); k.got(hor); k.got(cols);
  k.done();
}

// hip_sao_reconstruct_color: the block with its ring (one pixel where the edge class looks), a kvz_hip_sao_block (five int32) and a
// kvz_hip_sao_info (fourteen) in; the filtered window out
static void walk_sao_reconstruct_color(const char *name, size_t bw, size_t bh, size_t rx, size_t ry)
{
  buffers b(1u << 20);
  walk k(name, b);
  const size_t ww = bw + 2 * rx, wh = bh + 2 * ry;
  by_hand s;
  s.take(ww * wh); s.take(20); s.take(56);
  const size_t in_end = s.off, oo = s.take(ww * wh);

  k.in<uint8_t>(ww * wh); k.in<int32_t>(5); k.in<int32_t>(14);
  auto out = k.out<uint8_t>(ww * wh);
  k.upload(0, in_end);
  k.launch();
  k.download(out, out, oo, ww * wh);
  k.got(out);
  k.done();
}

// ---- the order of a phase, and the capacity ----
static const char *word(stage_status st) { return st == STAGE_OK ? "taken" : st == STAGE_OVERFLOW ? "overflow" : "input after output"; }

// prints the verdict of a take, and where the slot lies if it was taken (the slot is read after the take: it is passed by reference)
template <typename T> static void say(const char *lead, stage_status st, const stage_slot<T> &s)
{
  printf("%s %s", lead, word(st));
  if (st == STAGE_OK) printf(" at %zu", s.off);
}
// writes the slot's last byte in both buffers through its handle
static void touch_end(buffers &b, stage_slot<uint8_t> s) { s.host(b.h)[s.count - 1] = 1; s.dev(b.d)[s.count - 1] = 2; }

static void order_and_capacity()
{
  buffers b(256);
  {
    stage_layout lay(256);
    stage_slot<uint8_t> s;
    say("order: input", lay.in(16, &s), s);
    say(", output", lay.out(16, &s), s);
    say(", input", lay.in(16, &s), s);                            // refused, and consumes nothing
    say(", output", lay.out(16, &s), s);
    lay.next_phase();
    say(", after next_phase input", lay.in(16, &s), s);
    printf(", upload %zu+%zu\n", lay.upload().off, lay.upload().bytes);
  }
  {
    stage_layout lay(256);
    stage_slot<uint8_t> s;
    say("capacity 256: 100", lay.in(100, &s), s);
    say(", 100", lay.in(100, &s), s);
    say(", 32", lay.out(32, &s), s);                              // ends with the capacity
    touch_end(b, s);
    say(", 1", lay.out(1, &s), s);
    say(", 0", lay.out(0, &s), s);
    printf("\n");
  }
  {
    stage_layout lay(256);
    stage_slot<uint8_t> s;
    say("capacity 256: 200", lay.in(200, &s), s);
    say(", 57", lay.out(57, &s), s);                              // 208 + 57 crosses; a refused take consumes nothing
    say(", 48", lay.out(48, &s), s);
    touch_end(b, s);
    printf("\n");
  }
  {
    stage_layout a(256), c(256), e(256), f(250);
    stage_slot<int32_t> s;
    stage_slot<uint8_t> u;
    say("capacity 256: int32 x 65", a.in(65, &s), s);
    say(", int32 x 64", a.in(64, &s), s);
    say(", int32 x 2^62", c.in((size_t)1 << 62, &s), s);          // the byte count would wrap
    say(", SIZE_MAX bytes", e.out(SIZE_MAX, &u), u);
    say("; capacity 250: 241", f.in(241, &u), u);                 // the bump offset, 256, is then past the capacity
    say(", 1", f.in(1, &u), u);
    say(", 0", f.in(0, &u), u);
    printf("\n");
  }
}

int main()
{
  slot_cases();
  walk_quantize_residual("quantize_residual 4x4", 4, false);
  walk_quantize_residual("quantize_residual 32x32 with tables", 32, true);
  walk_quantize_residual_rdoq("quantize_residual 4x4 rdoq", 4);
  walk_quantize_residual_rdoq("quantize_residual 8x8 rdoq", 8);
  walk_filter_step("filter_step 8x8", 8, 8);
  walk_filter_step("filter_step 12x16", 12, 16);
  walk_sao_reconstruct_color("sao_reconstruct_color 7x5 diagonal", 7, 5, 1, 1);
  walk_sao_reconstruct_color("sao_reconstruct_color 7x5 band", 7, 5, 0, 0);
  order_and_capacity();
  return 0;
}
"""

EXPECTED = """\
slot of 1 bytes: at 0
slot of 4 bytes: at 16
slot of 15 bytes: at 32
slot of 16 bytes: at 48
slot of 17 bytes: at 64
slot of 4097 bytes: at 96
int16 x 17: at 4208, 34 bytes; int32 x 5: at 4256, 20 bytes; uint64 x 1: at 4288; outputs at 4304 and 4320
slots: 16-byte aligned and apart
slots: upload 0+4296
slots: download 4304+22
slots: bytes ok
quantize_residual 4x4: upload 0+32 by hand 0+32
quantize_residual 4x4: download 32+52 by hand 32+64
quantize_residual 4x4: bytes ok
quantize_residual 32x32 with tables: upload 0+10240 by hand 0+10240
quantize_residual 32x32 with tables: download 10240+3076 by hand 10240+3088
quantize_residual 32x32 with tables: bytes ok
quantize_residual 4x4 rdoq: upload 0+32 by hand 0+32
quantize_residual 4x4 rdoq: download 64+32 by hand 64+32
quantize_residual 4x4 rdoq: upload 96+32 by hand 96+32
quantize_residual 4x4 rdoq: download 160+16 by hand 160+16
quantize_residual 4x4 rdoq: bytes ok
quantize_residual 8x8 rdoq: upload 0+128 by hand 0+128
quantize_residual 8x8 rdoq: download 256+128 by hand 256+128
quantize_residual 8x8 rdoq: upload 384+128 by hand 384+128
quantize_residual 8x8 rdoq: download 640+64 by hand 640+64
quantize_residual 8x8 rdoq: bytes ok
filter_step 8x8: upload 0+272 by hand 0+272
filter_step 8x8: download 272+832 by hand 272+832
filter_step 8x8: bytes ok
filter_step 12x16: upload 0+504 by hand 0+512
filter_step 12x16: download 512+2016 by hand 512+2016
filter_step 12x16: bytes ok
sao_reconstruct_color 7x5 diagonal: upload 0+152 by hand 0+160
sao_reconstruct_color 7x5 diagonal: download 160+63 by hand 160+63
sao_reconstruct_color 7x5 diagonal: bytes ok
sao_reconstruct_color 7x5 band: upload 0+136 by hand 0+144
sao_reconstruct_color 7x5 band: download 144+35 by hand 144+35
sao_reconstruct_color 7x5 band: bytes ok
order: input taken at 0, output taken at 16, input input after output, output taken at 32, after next_phase input taken at 48, upload 48+16
capacity 256: 100 taken at 0, 100 taken at 112, 32 taken at 224, 1 overflow, 0 taken at 256
capacity 256: 200 taken at 0, 57 overflow, 48 taken at 208
capacity 256: int32 x 65 overflow, int32 x 64 taken at 0, int32 x 2^62 overflow, SIZE_MAX bytes overflow; capacity 250: 241 taken at 0, 1 overflow, 0 overflow
""".splitlines()


def up16(v):
    return (v + 15) & ~15


def test_slots_ranges_phases_and_capacity():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dropin_stage_host.cpp"), os.path.join(tmp, "dropin_stage_host")
        with open(src, "w") as f:
            f.write(PROGRAM)
        cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
               "-I", os.path.join(ROOT, "kvazaar_amd", "csrc"), src, "-o", exe]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines() == EXPECTED
    # the literals themselves: a derived range begins where the hand-kept one began and ends with it, but for the padding behind the last slot
    import re
    walks = [re.search(r"(\d+)\+(\d+) by hand (\d+)\+(\d+)", line) for line in EXPECTED if "by hand" in line]
    assert len(walks) == 20
    for m in walks:
        off, n, hand_off, hand_n = map(int, m.groups())
        assert off == hand_off and (n == hand_n or up16(n) == hand_n), m.group(0)
