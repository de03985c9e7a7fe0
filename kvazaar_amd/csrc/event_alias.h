// event_alias.h -- bookkeeping that lets an event record which directly follows a kernel launch ride on that launch's own
// dispatch packet instead of a marker packet of its own (api.hip).  Host-only and free of HIP: the event
// handle is a template parameter, so that the rules can be tested without a device (tests/test_event_alias_host.py).
//
// Per stream the table keeps
//   ops         number of ABI operations that touched the stream,
//   record_at   value of ops at the last event record,
//   carried_at  value of ops at which a launch attached a carrier event, and that carrier.
// Rules
//   armed       a launch gets a carrier only if the operation just before its entry was an event record (record_at == ops - 1):
//               a caller that records in front of a launch is taken to record behind it too.  Nobody else's launches change.
//   alias       record() aliases if a carrying launch was the last operation on the stream (carried_at == ops): the event takes a
//               reference to the carrier and nothing is enqueued.  Further records with nothing in between share the carrier.
//   invalidate  every other operation (touch()) ends the carrier's life as an alias target; events that hold it keep it.
//   carriers    come from pools (one per device and event flavour) and return to their pool when no event and no stream refers to
//               them any more.  A pool grows in chunks: when an ABI event is created (provision_event(), one carrier per live
//               event and one to spare, so that the timed launches find theirs made), else inside an armed launch, never in another.
//   threads     a record aliases only a launch of the calling thread.  Threads that share a stream (the library's default stream is
//               one per device) each see their own earlier work covered by their records, as before: between a launch site's arm()
//               and its enqueue another thread's record would otherwise take a carrier that is not bound to anything yet.
// One mutex guards everything; it is held for a table lookup and a few assignments.
#pragma once

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

namespace kvzhip {

// Factory: { bool create(int pool, Handle *out); void destroy(Handle h); } -- create() makes one carrier handle for `pool`.
template <typename Handle, typename Factory>
class event_alias {
 public:
  struct carrier {
    Handle handle;
    int pool;
    int refs;           // events that alias it + the stream it is current on
  };
  // what an ABI event keeps besides its own handle
  struct event_state {
    carrier *held = nullptr;
    int pool = -1;      // the pool provision_event() counted the event in
  };
  static constexpr int CHUNK = 16;

  explicit event_alias(Factory f = Factory()) : factory_(f) {}
  event_alias(const event_alias &) = delete;
  event_alias &operator=(const event_alias &) = delete;
  ~event_alias()
  {
    for (carrier *c : all_) { factory_.destroy(c->handle); delete c; }
  }

  // an ABI event is created: its pool gets a carrier for it (and one for a stream to hold) now, in chunks, so that the armed launches,
  // which are the timed ones, find their carriers made.  take() still grows the pool for events that were never announced.
  void provision_event(event_state &ev, int pool)
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (pool < 0 || ev.pool >= 0) return;
    if ((size_t)pool >= free_.size()) { free_.resize((size_t)pool + 1); made_.resize((size_t)pool + 1, 0); wanted_.resize((size_t)pool + 1, 0); }
    ev.pool = pool;
    ++wanted_[(size_t)pool];
    while (made_[(size_t)pool] < wanted_[(size_t)pool] + 1)
      if (!grow(pool)) break;
  }

  // the launch that arm() gave a carrier to did not take place: nothing is carried
  void disarm(const void *stream)
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = streams_.find(stream);
    if (it == streams_.end()) return;
    drop_current(it->second);
    it->second.record_at = 0;
  }

  // an ABI operation other than a record enters `stream`: whatever was carried can no longer be aliased
  void touch(const void *stream)
  {
    std::lock_guard<std::mutex> lk(mu_);
    stream_state &s = streams_[stream];
    ++s.ops;
    drop_current(s);
  }

  // would a launch on `stream` get a carrier now?  (asked before the costlier questions, such as whether the stream is capturing)
  bool armed(const void *stream)
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = streams_.find(stream);
    return it != streams_.end() && is_armed(it->second);
  }

  // the launch site of an entry that has touch()ed `stream`: the carrier to bind to the dispatch, or false (launch as ever).
  // A second launch of the same entry gets none and ends the first one's: only an entry's last launch may stand for a record.
  bool arm(const void *stream, int pool, Handle *out)
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = streams_.find(stream);
    if (it == streams_.end()) return false;
    stream_state &s = it->second;
    if (s.carried_at == s.ops) {
      drop_current(s);
      s.record_at = 0;
      return false;
    }
    if (!is_armed(s)) return false;
    carrier *c = take(pool);
    if (!c) return false;
    c->refs = 1;
    s.current = c;
    s.carried_at = s.ops;
    s.carried_by = std::this_thread::get_id();
    *out = c->handle;
    return true;
  }

  // record `ev` on `stream`: true = aliased, *out is the carrier's handle and nothing is to be enqueued; false = the caller
  // records the event's own handle (this then counts as an operation on the stream)
  bool record(event_state &ev, const void *stream, Handle *out)
  {
    std::lock_guard<std::mutex> lk(mu_);
    stream_state &s = streams_[stream];
    // only the thread that launched knows that its launch is in the queue: another thread's record is a record of its own
    if (s.current && s.carried_at == s.ops && s.carried_by == std::this_thread::get_id()) {
      carrier *c = s.current;
      ++c->refs;
      release(ev.held);
      ev.held = c;
      s.record_at = s.ops;
      *out = c->handle;
      return true;
    }
    ++s.ops;
    drop_current(s);
    s.record_at = s.ops;
    release(ev.held);
    ev.held = nullptr;
    return false;
  }

  // the handle that stands for the event's last record: the carrier's if it was aliased, else `own`
  Handle current(const event_state &ev, Handle own)
  {
    std::lock_guard<std::mutex> lk(mu_);
    return ev.held ? ev.held->handle : own;
  }

  void destroy_event(event_state &ev)
  {
    std::lock_guard<std::mutex> lk(mu_);
    release(ev.held);
    ev.held = nullptr;
    if (ev.pool >= 0) --wanted_[(size_t)ev.pool];
    ev.pool = -1;
  }

  void forget_stream(const void *stream)
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = streams_.find(stream);
    if (it == streams_.end()) return;
    drop_current(it->second);
    streams_.erase(it);
  }

  // for tests and reports
  size_t carriers_total() { std::lock_guard<std::mutex> lk(mu_); return all_.size(); }
  size_t carriers_free()
  {
    std::lock_guard<std::mutex> lk(mu_);
    size_t n = 0;
    for (auto &p : free_) n += p.size();
    return n;
  }

 private:
  struct stream_state {
    uint64_t ops = 0, record_at = 0, carried_at = 0;      // ops >= 1 once touched: 0 means "never"
    carrier *current = nullptr;                           // carrier of the launch at carried_at, while it can still be aliased
    std::thread::id carried_by;                           // the thread of that launch
  };

  static bool is_armed(const stream_state &s) { return s.record_at != 0 && s.record_at + 1 == s.ops; }

  void release(carrier *c)
  {
    if (c && --c->refs == 0) free_[(size_t)c->pool].push_back(c);
  }
  void drop_current(stream_state &s)
  {
    release(s.current);
    s.current = nullptr;
    s.carried_at = 0;
  }
  carrier *take(int pool)
  {
    if (pool < 0) return nullptr;
    if ((size_t)pool >= free_.size()) { free_.resize((size_t)pool + 1); made_.resize((size_t)pool + 1, 0); wanted_.resize((size_t)pool + 1, 0); }
    std::vector<carrier *> &f = free_[(size_t)pool];
    if (f.empty() && !grow(pool)) return nullptr;
    carrier *c = f.back();
    f.pop_back();
    return c;
  }
  // one more chunk of carriers for `pool` (free_ is large enough); false if none could be made
  bool grow(int pool)
  {
    int n = 0;
    for (; n < CHUNK; ++n) {
      Handle h;
      if (!factory_.create(pool, &h)) break;
      carrier *c = new carrier{ h, pool, 0 };
      all_.push_back(c);
      free_[(size_t)pool].push_back(c);
    }
    made_[(size_t)pool] += (size_t)n;
    return n > 0;
  }

  std::mutex mu_;
  Factory factory_;
  std::unordered_map<const void *, stream_state> streams_;
  std::vector<std::vector<carrier *>> free_;     // [pool]
  std::vector<carrier *> all_;
  std::vector<size_t> made_, wanted_;            // [pool]: carriers made, events provisioned and alive
};

}  // namespace kvzhip
