// serve_ring.h -- what the two halves of the search service share: the host side (serve.hip, which explains the protocol) and the
// kernels (serve_kernels.hip).
#pragma once
#include "kvz_hip_internal.h"

namespace kvzhip {

// One (PU, reference picture) unit of a batch, as the kernels read it from page-locked host memory.
struct serve_unit {                       // 176 bytes
  int32_t pic_slot, ref_slot;
  void *result;                           // this unit's serve_result (page-locked host memory)
  kvz_hip_me_pu pu;
  kvz_hip_me_params prm;
};
struct serve_result {                     // 80 bytes
  kvz_hip_me_result frac;                 // integer + fractional search: search_pu_inter_ref when info->best_cost < *inter_cost
  kvz_hip_me_result integer;              // otherwise: the integer vector with its SATD cost (search_inter.c:1242-1252)
  uint32_t integer_search_cost;           // info->best_cost after the integer search, what :1239 compares with *inter_cost
  uint32_t done;                          // written last
  uint32_t pad[2];
};
// Resident workers (the service's other way to the device): units travel through a ring of slots in page-locked host memory,
// workgroups that stay on the device take them by ticket.
constexpr int SERVE_MAX_WORKERS = 256;
struct serve_slot {                       // 192 bytes
  serve_unit u;
  uint32_t seq;                           // serve_seq(ticket) once the unit is written (host), 0 once a worker has copied it (device)
  uint32_t pad[3];
};
// serve_slot.seq of the unit with this ticket: never 0 (0 = "free: a worker has copied the unit"), also when the 64-bit ticket count
// passes a multiple of 2^32 -- at a million units a second that is every 71 minutes.
__host__ __device__ inline uint32_t serve_seq(unsigned long long ticket) { return (uint32_t)(ticket % 0xFFFFFFFFull) + 1u; }
struct serve_ring_ctl {                   // page-locked host memory
  unsigned long long tail;                // units published so far (host writes, workers read across PCIe)
  uint32_t quit;                          // host: every worker leaves when it next finds no work
  uint32_t failed;                        // a worker gave up waiting for a slot to be written
  uint32_t pad[12];
  uint32_t alive[SERVE_MAX_WORKERS];      // worker w: 0 = gone (or going and no longer counted), else launched / running
};
struct serve_ring_dev {                   // device memory
  unsigned long long head;                // next ticket to take
  unsigned long long tail;                // the workers' copy of ctl->tail
  unsigned long long reserved0;
  unsigned long long last_claim;          // wall clock of the last ticket taken by anybody: the workers leave together when the service falls idle
  unsigned long long pad[4];
  // what the workers measured (10 ns ticks, summed over units): ticket -> unit copied, ticket -> results written; units served
  unsigned long long fetch_ticks, busy_ticks, units_served, backlog, idle_ticks, pad2[3];   // backlog: units published and not taken, summed at every ticket
};
// "Push" mode (a device whose memory the host can write through a large PCIe BAR): the host writes the units and the published
// ticket count straight into fine-grained DEVICE memory, so a resident worker never reads host memory on the request path (a PCIe read
// is ~2 us, and there were two of them per unit).  The slot's sequence word in HOST memory stays the "slot taken / free" handshake, and
// the ticket count in host memory (serve_ring_ctl.tail) stays what a LEAVING worker looks at last -- that look must be a PCIe read
// behind its "gone" store (serve.hip, "who makes sure somebody is there").
struct serve_push {                       // fine-grained device memory, written by the host through the BAR
  unsigned long long tail;                // = serve_ring_ctl.tail
  uint32_t quit;                          // = serve_ring_ctl.quit
  uint32_t pad[13];
};
struct serve_worker_ids { unsigned char id[SERVE_MAX_WORKERS]; };

// starts `count` workers (512 threads each) named ids.id[0 .. count); they leave after linger_ticks without work, or at the first
// idle moment after life_ticks (wall-clock ticks of 10 ns), or when ctl->quit is set.  `ring` is what the workers READ units from
// (the host ring, or its copy in device memory), `host_ring` the ring whose sequence words they clear, `push` the push block
// (nullptr: they poll serve_ring_ctl in host memory)
int serve_workers_launch(const u8 *planes, size_t plane_bytes, int n_slots, u32 stride, int w, int h, serve_slot *ring, serve_slot *host_ring,
                         const serve_push *push, u32 ring_mask, serve_ring_ctl *ctl, serve_ring_dev *dev, const serve_worker_ids &ids, int count,
                         unsigned long long linger_ticks, unsigned long long life_ticks, unsigned long long poll_period_ticks, hipStream_t st);
// one batch in a launch of its own; `units` is device-visible host memory.  `constrained`: some fracmv_within_tile rule is active in
// the batch (wpp_owf or an mv_constraint)
int serve_launch(bool constrained, const u8 *planes, size_t plane_bytes, int n_slots, u32 stride, int w, int h,
                 const serve_unit *units, int count, hipStream_t st);

}  // namespace kvzhip
