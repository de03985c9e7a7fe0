"""CPU: the bookkeeping that lets an event record ride on the launch in front of it (kvazaar_amd/csrc/event_alias.h), without a device.

The header has no HIP in it: a stand-alone C++ program instantiates the table with integer handles and a counting factory, plays directed
sequences of ABI operations (touch = an entry resolving its stream, arm = the launch site of a converted entry, record) and prints one
line per case.  It is compiled with the address and undefined-behaviour sanitizers, their runtimes linked statically, and run as a child
process; the table's destructor frees every carrier, so a leak fails the run too."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include <atomic>
#include <thread>
#include <vector>

#include "event_alias.h"

static std::atomic<int> created{0}, destroyed{0};
struct counting_factory {
  bool create(int pool, int *out) { *out = 100000 * (pool + 1) + created.fetch_add(1); return true; }
  void destroy(int) { destroyed.fetch_add(1); }
};
typedef kvzhip::event_alias<int, counting_factory> table;
typedef table::event_state event;

static int streams[4];
static const void *S(int i) { return &streams[i]; }
static const int OWN = -1;

// an entry of one launch on stream s: the handle it carries, or 0
static int launch(table &t, int s, int pool = 0)
{
  t.touch(S(s));
  int h = 0;
  if (!t.armed(S(s))) { if (t.arm(S(s), pool, &h)) return -999; return 0; }      // arm() agrees with armed()
  return t.arm(S(s), pool, &h) ? h : 0;
}
// a record: the carrier's handle if aliased, else OWN
static int record(table &t, event &e, int s)
{
  int h = 0;
  const bool aliased = t.record(e, S(s), &h);
  const int cur = t.current(e, OWN);
  if (aliased ? cur != h : cur != OWN) return -999;                              // current() is what record() said
  return cur;
}
static void verdict(const char *name, bool ok) { printf("%s: %s\n", name, ok ? "ok" : "WRONG"); }

int main()
{
  {
    table t; event a, b;
    const int ra = record(t, a, 0), c = launch(t, 0), rb = record(t, b, 0);
    verdict("record launch record aliases", ra == OWN && c > 0 && rb == c);
    t.destroy_event(a); t.destroy_event(b);
  }
  {
    table t; event b;
    t.touch(S(0));
    const int c = launch(t, 0), rb = record(t, b, 0);
    verdict("launch record without a record before does not", c == 0 && rb == OWN && t.carriers_total() == 0);
    t.destroy_event(b);
  }
  {
    table t; event a, b;
    record(t, a, 0);
    const int c = launch(t, 0);
    t.touch(S(0));                                                               // a copy, a memset, a wait, a graph launch, a plain entry
    const int rb = record(t, b, 0);
    verdict("launch other operation record does not", c > 0 && rb == OWN && t.carriers_free() == t.carriers_total());
    t.destroy_event(a); t.destroy_event(b);
  }
  {
    table t; event a, b, c3, d;
    record(t, a, 0);
    const int c = launch(t, 0);
    const int r1 = record(t, b, 0), r2 = record(t, c3, 0), r3 = record(t, d, 0);
    // the next launch is armed by the aliased records, and gets a carrier of its own
    const int c2 = launch(t, 0);
    verdict("record launch record record shares one carrier", c > 0 && r1 == c && r2 == c && r3 == c && c2 > 0 && c2 != c);
    t.destroy_event(a); t.destroy_event(b); t.destroy_event(c3); t.destroy_event(d);
    t.touch(S(0));
    verdict("shared carrier returns once", t.carriers_free() == t.carriers_total());
  }
  {
    // an entry that launches twice: neither launch may stand for the record behind the entry
    table t; event a, b;
    record(t, a, 0);
    t.touch(S(0));
    int h1 = 0, h2 = 0;
    const bool first = t.arm(S(0), 0, &h1), second = t.arm(S(0), 0, &h2);
    const int rb = record(t, b, 0);
    verdict("two launches in one entry do not", first && !second && rb == OWN);
    t.destroy_event(a); t.destroy_event(b);
  }
  {
    table t; event e;
    bool ok = true;
    record(t, e, 0);
    for (int i = 0; i < 1000; ++i) {
      const int c = launch(t, 0);
      ok = ok && c > 0 && record(t, e, 0) == c;
    }
    ok = ok && t.carriers_total() <= (size_t)table::CHUNK;
    t.destroy_event(e);
    t.touch(S(0));
    verdict("an event re-recorded 1000 times", ok && t.carriers_free() == t.carriers_total());
    printf("pool after 1000 re-records: %zu\n", t.carriers_total());
  }
  {
    // fresh events every step, as a benchmark keeps them: the pool grows with the events held and comes back whole
    table t;
    std::vector<event> ev(4 * 200);
    bool ok = true;
    for (int k = 0; k < 200; ++k) {
      record(t, ev[4 * k], 0);
      for (int j = 1; j < 4; ++j) { const int c = launch(t, 0); ok = ok && c > 0 && record(t, ev[4 * k + j], 0) == c; }
    }
    ok = ok && t.carriers_total() >= 600 && t.carriers_total() <= 600 + (size_t)table::CHUNK;
    for (auto &e : ev) t.destroy_event(e);
    t.touch(S(0));
    verdict("fresh events every step", ok && t.carriers_free() == t.carriers_total());
  }
  {
    table t; event a, b;
    record(t, a, 0);
    const int c = launch(t, 0);
    record(t, b, 0);
    t.destroy_event(b);                                                          // holds the carrier; the stream still does too
    const bool held = t.carriers_free() + 1 == t.carriers_total();
    event d;
    const int rd = record(t, d, 0);                                              // still the last operation's carrier
    t.destroy_event(d); t.destroy_event(a);
    t.forget_stream(S(0));
    verdict("an event destroyed while it holds a carrier", c > 0 && held && rd == c && t.carriers_free() == t.carriers_total());
  }
  {
    table t; event a0, b0, a1, b1;
    record(t, a0, 0);
    record(t, a1, 1);
    const int c0 = launch(t, 0);
    t.touch(S(1));                                                               // stream 1 does something else
    const int c1 = launch(t, 1);                                                 // so its launch is not armed
    const int r1 = record(t, b1, 1), r0 = record(t, b0, 0);
    const int c1b = launch(t, 1);                                                // but the next one is
    const int r1b = record(t, b1, 1);
    verdict("two streams interleaved", c0 > 0 && r0 == c0 && c1 == 0 && r1 == OWN && c1b > 0 && c1b != c0 && r1b == c1b);
    for (event *e : { &a0, &b0, &a1, &b1 }) t.destroy_event(*e);
  }
  {
    table t; event a, b;
    record(t, a, 0);
    const int c = launch(t, 0, 0);
    record(t, b, 0);
    const int c2 = launch(t, 0, 5);
    verdict("pools are separate", c / 100000 == 1 && c2 / 100000 == 6);
    t.destroy_event(a); t.destroy_event(b);
  }
  {
    // events announced when they are created: the carriers are made then, none inside the launches; destroyed events give their share back
    table t;
    std::vector<event> ev(4 * 50);
    for (auto &e : ev) t.provision_event(e, 0);
    const int made = created;
    bool ok = t.carriers_total() >= ev.size() + 1 && t.carriers_total() <= ev.size() + 1 + (size_t)table::CHUNK;
    for (int k = 0; k < 50; ++k) {
      record(t, ev[4 * k], 0);
      for (int j = 1; j < 4; ++j) { const int c = launch(t, 0); ok = ok && c > 0 && record(t, ev[4 * k + j], 0) == c; }
    }
    ok = ok && created == made;
    for (auto &e : ev) t.destroy_event(e);
    t.touch(S(0));
    for (int i = 0; i < 1000; ++i) { event e; t.provision_event(e, 0); t.destroy_event(e); }
    verdict("provisioned events find their carriers made", ok && created == made && t.carriers_free() == t.carriers_total());
  }
  {
    // two threads on ONE stream: a record of the other thread, which cannot know whether the launch is in the queue yet, is a record
    // of its own and ends the alias for the launching thread too
    table t; event a, b, c3;
    record(t, a, 0);
    const int c = launch(t, 0);
    int other = 0;
    std::thread([&] { other = record(t, b, 0); }).join();
    const int mine = record(t, c3, 0);
    verdict("another thread's record does not alias", c > 0 && other == OWN && mine == OWN);
    for (event *e : { &a, &b, &c3 }) t.destroy_event(*e);
  }
  {
    // the carrying launch failed: the record behind it is a real one, and so is the one behind the next launch
    table t; event a, b;
    record(t, a, 0);
    const int c = launch(t, 0);
    t.disarm(S(0));
    const int rb = record(t, b, 0);
    verdict("a failed launch carries nothing", c > 0 && rb == OWN && t.carriers_free() == t.carriers_total());
    t.destroy_event(a); t.destroy_event(b);
  }
  {
    table t;
    std::atomic<int> wrong{0};
    auto worker = [&](int s) {
      event e[4];
      record(t, e[0], s);
      for (int i = 0; i < 20000; ++i) {
        const int c = launch(t, s);
        if (c <= 0 || record(t, e[1 + i % 3], s) != c) ++wrong;
        if (i % 7 == 0) { t.touch(S(s)); if (launch(t, s) != 0) ++wrong; if (record(t, e[0], s) != OWN) ++wrong; }
      }
      for (auto &x : e) t.destroy_event(x);
      t.forget_stream(S(s));
    };
    std::thread t0(worker, 0), t1(worker, 1);
    t0.join(); t1.join();
    verdict("two threads on two streams", wrong == 0 && t.carriers_free() == t.carriers_total() && t.carriers_total() <= 2 * (size_t)table::CHUNK);
  }
  verdict("every carrier destroyed with its table", created == destroyed && created > 0);
  return 0;
}
"""

CASES = (
    "record launch record aliases",
    "launch record without a record before does not",
    "launch other operation record does not",
    "record launch record record shares one carrier",
    "shared carrier returns once",
    "two launches in one entry do not",
    "an event re-recorded 1000 times",
    "fresh events every step",
    "an event destroyed while it holds a carrier",
    "two streams interleaved",
    "pools are separate",
    "provisioned events find their carriers made",
    "another thread's record does not alias",
    "a failed launch carries nothing",
    "two threads on two streams",
    "every carrier destroyed with its table",
)


def test_alias_rules_on_directed_sequences(tmp_path):
    src, exe = tmp_path / "event_alias_host.cpp", tmp_path / "event_alias_host"
    src.write_text(PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-I", os.path.join(ROOT, "kvazaar_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = dict(line.rsplit(": ", 1) for line in r.stdout.splitlines() if line.endswith((": ok", ": WRONG")))
    assert sorted(got) == sorted(CASES), r.stdout
    for name in CASES:
        assert got[name] == "ok", r.stdout
