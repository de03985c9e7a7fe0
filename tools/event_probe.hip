// What does a stop event bound to a dispatch (hipExtLaunchKernelGGL(..., nullptr, stopEvent, 0)) mean on this runtime?  The check that
// came before api.hip let event records ride on launches (output: profiles/headline_alias_probe.txt): times
// between bound events and plain records, ordering of a second stream through a bound event, and what a step of three launches
// costs with no events, with records, and with bound events.  Includes picture.hip for sad_nxn_kernel<8,4,false>, with stubs for
// the context it asks of api.hip.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-function tools/event_probe.hip -o tools/event_probe && tools/event_probe
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/kvz_hip.h"
#include "../kvazaar_amd/csrc/kvz_hip_internal.h"

namespace kvzhip {
int ctx_device() { return 0; }
bool ctx_ready() { return true; }
bool ctx_enter() { return true; }
hipStream_t ctx_stream(kvz_hip_stream s) { return (hipStream_t)s; }
void set_error(const char *, hipError_t) {}
void set_error_msg(const char *) {}
int invalid_arg(const char *) { return -1; }
int num_cus() { return 256; }
int stream_on_current_device(kvz_hip_stream, const char *) { return 0; }
hipEvent_t launch_carrier(hipStream_t) { return nullptr; }      // picture.hip's own entries launch plainly here; the probe binds its events itself
void launch_uncarry(hipStream_t) {}
}
extern "C" int kvz_hip_init(int) { return 0; }

#include "../kvazaar_amd/csrc/picture.hip"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("FAIL %s line %d: %s\n", #x, __LINE__, hipGetErrorString(e_)); return 2; } } while (0)

static unsigned sad_grid(size_t count) { return kvzhip::stream_grid(count * 4, 1024, 256); }

int main()
{
  const size_t count = (size_t)32400 * 128;
  u8 *a, *b; u32 *costs, *slots;
  const int ROUNDS = 8;
  CK(hipMalloc(&a, count * 64)); CK(hipMalloc(&b, count * 64)); CK(hipMalloc(&costs, count * 4));
  CK(hipMalloc(&slots, count * 4 * ROUNDS));
  CK(hipMemset(a, 7, count * 64)); CK(hipMemset(b, 9, count * 64));      // every SAD = 128
  hipStream_t s1, s2;
  CK(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking)); CK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
  hipEvent_t R, A, B, P, D;
  for (hipEvent_t *e : { &R, &A, &B, &P, &D }) CK(hipEventCreateWithFlags(e, hipEventDisableSystemFence));
  const unsigned grid = sad_grid(count);
  auto plain = [&](hipStream_t st) { hipLaunchKernelGGL((sad_nxn_kernel<8, 4, false>), dim3(grid), dim3(256), 0, st, a, b, costs, count, (size_t)0, (size_t)0); };
  auto carried = [&](hipStream_t st, hipEvent_t stop) {
    hipExtLaunchKernelGGL((sad_nxn_kernel<8, 4, false>), dim3(grid), dim3(256), 0, st, nullptr, stop, 0, a, b, costs, count, (size_t)0, (size_t)0); };
  for (int i = 0; i < 10; ++i) plain(s1);
  CK(hipStreamSynchronize(s1));

  // 1. times
  for (int rep = 0; rep < 3; ++rep) {
    CK(hipEventRecord(R, s1));
    carried(s1, A);
    carried(s1, B);
    CK(hipEventRecord(P, s1));
    CK(hipGetLastError());
    CK(hipStreamSynchronize(s1));
    float ra, ab, rb, bp, ap;
    CK(hipEventElapsedTime(&ra, R, A)); CK(hipEventElapsedTime(&ab, A, B)); CK(hipEventElapsedTime(&rb, R, B));
    CK(hipEventElapsedTime(&bp, B, P)); CK(hipEventElapsedTime(&ap, A, P));
    printf("times rep %d: R->A %.5f  A->B %.5f  R->B %.5f  (sum %.5f, diff %.2e)  B->P %.5f  A->P %.5f ms\n", rep, ra, ab, rb, ra + ab, ra + ab - rb, bp, ap);
  }
  // the same with plain records, for comparison
  {
    CK(hipEventRecord(R, s1)); plain(s1); CK(hipEventRecord(A, s1)); plain(s1); CK(hipEventRecord(B, s1));
    CK(hipStreamSynchronize(s1));
    float ra, ab, rb;
    CK(hipEventElapsedTime(&ra, R, A)); CK(hipEventElapsedTime(&ab, A, B)); CK(hipEventElapsedTime(&rb, R, B));
    printf("plain records:  R->A %.5f  A->B %.5f  R->B %.5f ms\n", ra, ab, rb);
  }
  // hipEventQuery / hipEventSynchronize on a bound event
  {
    carried(s1, A);
    hipError_t q = hipEventQuery(A);
    CK(hipEventSynchronize(A));
    hipError_t q2 = hipEventQuery(A);
    printf("query right after launch: %s; after hipEventSynchronize: %s\n", hipGetErrorName(q), hipGetErrorName(q2));
    CK(hipStreamSynchronize(s1));
  }

  // 2. a bound event orders a second stream
  int bad_rounds = 0;
  for (int k = 0; k < ROUNDS; ++k) {
    CK(hipMemsetAsync(costs, 0xFF, count * 4, s1));
    CK(hipEventRecord(R, s1));
    carried(s1, A);
    CK(hipStreamWaitEvent(s2, A, 0));
    CK(hipMemcpyAsync(slots + (size_t)k * count, costs, count * 4, hipMemcpyDeviceToDevice, s2));
    CK(hipEventRecord(D, s2));
    CK(hipStreamWaitEvent(s1, D, 0));
  }
  CK(hipStreamSynchronize(s1)); CK(hipStreamSynchronize(s2));
  {
    std::vector<u32> h(count);
    for (int k = 0; k < ROUNDS; ++k) {
      CK(hipMemcpy(h.data(), slots + (size_t)k * count, count * 4, hipMemcpyDeviceToHost));
      size_t bad = 0;
      for (size_t i = 0; i < count; ++i) bad += h[i] != 128u;
      if (bad) { ++bad_rounds; printf("round %d: %zu of %zu costs wrong (first value %08x)\n", k, bad, count, h[0]); }
    }
    printf("ordering through a bound event: %d of %d rounds wrong\n", bad_rounds, ROUNDS);
  }

  // 3. what a step costs: three launches a step, 40 steps, wall time between stream syncs
  const int STEPS = 40;
  std::vector<hipEvent_t> evs(STEPS * 4);
  for (auto &e : evs) CK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  for (int rep = 0; rep < 3; ++rep) {
    for (int mode = 0; mode < 3; ++mode) {
      for (int i = 0; i < 30; ++i) plain(s1);
      CK(hipStreamSynchronize(s1));
      auto t0 = std::chrono::steady_clock::now();
      for (int k = 0; k < STEPS; ++k) {
        hipEvent_t *ev = &evs[k * 4];
        if (mode == 0) { for (int j = 0; j < 3; ++j) plain(s1); }
        else if (mode == 1) { (void)hipEventRecord(ev[0], s1); for (int j = 0; j < 3; ++j) { plain(s1); (void)hipEventRecord(ev[j + 1], s1); } }
        else { if (k == 0) (void)hipEventRecord(ev[0], s1); for (int j = 0; j < 3; ++j) carried(s1, ev[j + 1]); }
      }
      CK(hipStreamSynchronize(s1));
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      float in = 0;
      if (mode == 1) CK(hipEventElapsedTime(&in, evs[0], evs[STEPS * 4 - 1]));
      if (mode == 2) CK(hipEventElapsedTime(&in, evs[0], evs[STEPS * 4 - 1]));
      printf("rep %d mode %s: %.2f us per step (3 launches) wall; first to last event %.2f us per step\n", rep,
             mode == 0 ? "no events     " : mode == 1 ? "records       " : "bound to launch", us / STEPS, in * 1e3 / STEPS);
    }
  }
  CK(hipGetLastError());
  printf("probe done\n");
  return 0;
}
