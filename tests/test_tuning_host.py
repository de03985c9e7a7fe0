"""CPU: the table of tuning knobs and its lookups (kvazaar_amd/csrc/tuning.h), without a device, and the copies that are held to it.

The header has no HIP in it: a stand-alone C++ program includes it, searches every key by name, reads every key through the lookup
its row asks for (tuning<key>() or tuning_or<key>(default)) before and after stores, and runs the KVZ_HIP_TUNE parser on directed
strings; after each of those the values of ALL keys are compared, not only the ones named.  It is compiled with the address and
undefined-behaviour sanitizers, their runtimes linked statically, and run as a child process; the strings it parses live in heap
blocks of their exact size.  It prints one line per case and one line per key of the table.

In plain Python: the comment above kvz_hip_set_tuning in include/kvz_hip.h names every key, quoted, with the table's default on the
key's line; no call site under kvazaar_amd/csrc reads a knob by a string; and a misspelt key, or the lookup that does not fit the
key's row, is refused by the compiler."""
import os
import re
import subprocess

import pytest

from patterns import tuning_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "tuning.h"

using namespace kvzhip;

static void verdict(const char *name, bool ok) { printf("%s: %s\n", name, ok ? "ok" : "WRONG"); }

// tune_find on a heap copy of exactly the string's size: a compare that runs past the end is an error of the run
static int find(const std::string &s)
{
  std::vector<char> heap(s.c_str(), s.c_str() + s.size() + 1);
  return tune_find(heap.data());
}
static bool is_key(const std::string &s)
{
  for (int i = 0; i < TUNE_COUNT; ++i) if (s == tune_key[i]) return true;
  return false;
}

static void reset() { for (auto &v : tune_value) v.store(-1); }
static bool all_unset_but(tune k) { for (int i = 0; i < TUNE_COUNT; ++i) if (i != (int)k && tune_value[i].load() != -1) return false; return true; }

// the lookup the key's row asks for; the other one would not compile
template <tune K> static int read_knob(int site_default)
{
  if constexpr (tune_default[(int)K] == TUNE_PER_SITE) return tuning_or<K>(site_default);
  else return tuning<K>();
}
template <tune K> static bool lookup_follows_the_store()
{
  bool ok = true;
  for (int site : { 11, 77 }) {                      // two call sites with different defaults
    const int dflt = tune_default[(int)K] == TUNE_PER_SITE ? site : tune_default[(int)K];
    reset();
    ok = ok && read_knob<K>(site) == dflt && !tuning_is_set(K);
    for (int v : { 0, 1, 7 }) {
      tune_value[(int)K].store(v);
      ok = ok && read_knob<K>(site) == v && tuning_is_set(K) && all_unset_but(K);
    }
    for (int v : { -1, -5 }) {
      tune_value[(int)K].store(v);
      ok = ok && read_knob<K>(site) == dflt && !tuning_is_set(K);
    }
  }
  reset();
  return ok;
}

// KVZ_HIP_TUNE = text on a fresh store: exactly the keys of `want` hold a value, all others are untouched
static bool env_gives(const char *text, std::initializer_list<std::pair<tune, int>> want)
{
  std::atomic<int> store[TUNE_COUNT];
  int expect[TUNE_COUNT];
  for (int i = 0; i < TUNE_COUNT; ++i) { store[i].store(-1); expect[i] = -1; }
  for (auto &w : want) expect[(int)w.first] = w.second;
  std::vector<char> heap(text, text + strlen(text) + 1);
  tune_apply_env(heap.data(), store);
  for (int i = 0; i < TUNE_COUNT; ++i) if (store[i].load() != expect[i]) return false;
  return true;
}

int main()
{
  for (int i = 0; i < TUNE_COUNT; ++i) {
    if (tune_default[i] == TUNE_PER_SITE) printf("key %s per-site\n", tune_key[i]);
    else printf("key %s %d\n", tune_key[i], tune_default[i]);
  }
  {
    bool own = true, dup = false, tail = true, prefix = true;
    for (int i = 0; i < TUNE_COUNT; ++i) {
      const std::string k = tune_key[i];
      own = own && find(k) == i;
      for (int j = 0; j < i; ++j) dup = dup || k == tune_key[j];
      tail = tail && find(k + "x") == -1 && find(k + " ") == -1 && find(k + "=") == -1;
      for (size_t n = 0; n < k.size(); ++n) {
        if (!is_key(k.substr(0, n))) prefix = prefix && find(k.substr(0, n)) == -1;
        if (n && !is_key(k.substr(n))) prefix = prefix && find(k.substr(n)) == -1;
      }
    }
    verdict("tune_find gives every key its own index", own && TUNE_COUNT == (int)tune::count_ && find(tune_key[TUNE_COUNT - 1]) == TUNE_COUNT - 1);
    verdict("no two rows share a key", !dup);
    verdict("a key with a trailing character is no key", tail);
    verdict("a proper prefix or suffix of a key is no key", prefix);
    verdict("keys that end alike are told apart", find("pipe") == (int)tune::pipe && find("dct_pipe") == (int)tune::dct_pipe &&
            find("qr_tile_pipe") == (int)tune::qr_tile_pipe && find("qr_wgs_per_cu") == (int)tune::qr_wgs_per_cu &&
            find("qr8_wgs_per_cu") == (int)tune::qr8_wgs_per_cu && find("_pipe") == -1 && find("r_wgs_per_cu") == -1);
    verdict("the empty string, an unknown key and NULL are no keys", find("") == -1 && find("no_such_key") == -1 && tune_find(nullptr) == -1);
  }
  {
    bool ok = true;
#define CHECK(name, dflt, doc) ok = lookup_follows_the_store<tune::name>() && ok;
    KVZ_TUNE_KEYS(CHECK)
#undef CHECK
    verdict("every lookup follows the stored value", ok);
    // the two sites of one per-site key, spelled out
    reset();
    bool sites = tuning_or<tune::qr8_wgs_per_cu>(8) == 8 && tuning_or<tune::qr8_wgs_per_cu>(32) == 32;
    tune_value[(int)tune::qr8_wgs_per_cu].store(0);
    sites = sites && tuning_or<tune::qr8_wgs_per_cu>(8) == 0 && tuning_or<tune::qr8_wgs_per_cu>(32) == 0;
    reset();
    verdict("two sites of a per-site key keep their defaults", sites && tuning<tune::sad_wgs_per_cu>() == 256 && tuning<tune::pipe>() == 0);
  }
  {
    const tune a = tune::sad_wgs_per_cu, b = tune::dct_pipe;
    verdict("env one pair", env_gives("sad_wgs_per_cu=1", { { a, 1 } }));
    verdict("env two pairs", env_gives("sad_wgs_per_cu=1,dct_pipe=2", { { a, 1 }, { b, 2 } }));
    verdict("env empty pair between two", env_gives("sad_wgs_per_cu=1,,dct_pipe=2", { { a, 1 }, { b, 2 } }));
    verdict("env pair without =", env_gives("sad_wgs_per_cu", {}) && env_gives("sad_wgs_per_cu,dct_pipe=2", { { b, 2 } }));
    verdict("env pair without key", env_gives("=3", {}));
    verdict("env unknown key skipped", env_gives("nokey=3,sad_wgs_per_cu=4", { { a, 4 } }) && env_gives("sad_wgs_per_cu =4,pipe2=1,dct_pip=1", {}));
    verdict("env later pair wins", env_gives("sad_wgs_per_cu=1,sad_wgs_per_cu=2", { { a, 2 } }));
    verdict("env negative value stored", env_gives("sad_wgs_per_cu=-1", {}) && env_gives("sad_wgs_per_cu=-7", { { a, -7 } }));
    verdict("env value through atoi", env_gives("sad_wgs_per_cu=x", { { a, 0 } }) && env_gives("sad_wgs_per_cu=", { { a, 0 } }) &&
            env_gives("sad_wgs_per_cu=12x", { { a, 12 } }) && env_gives("sad_wgs_per_cu= 5", { { a, 5 } }));
    verdict("env split at the first =", env_gives("sad_wgs_per_cu=1=2", { { a, 1 } }));
    verdict("env trailing comma", env_gives("sad_wgs_per_cu=1,", { { a, 1 } }) && env_gives(",", {}) && env_gives(",dct_pipe=0", { { b, 0 } }));
    verdict("env empty string", env_gives("", {}));
    // on the library's own store: a negative value from the environment reads as the default
    reset();
    tune_apply_env("sad_wgs_per_cu=5,dct_pipe=1", tune_value);
    bool ok = tuning<tune::sad_wgs_per_cu>() == 5 && tuning<tune::dct_pipe>() == 1;
    tune_apply_env("sad_wgs_per_cu=-1,dct_pipe=-7", tune_value);
    ok = ok && tuning<tune::sad_wgs_per_cu>() == 256 && tuning<tune::dct_pipe>() == 0 && !tuning_is_set(a) && !tuning_is_set(b);
    reset();
    verdict("env negative value reads as the default", ok);
  }
  return 0;
}
"""

CASES = (
    "tune_find gives every key its own index",
    "no two rows share a key",
    "a key with a trailing character is no key",
    "a proper prefix or suffix of a key is no key",
    "keys that end alike are told apart",
    "the empty string, an unknown key and NULL are no keys",
    "every lookup follows the stored value",
    "two sites of a per-site key keep their defaults",
    "env one pair",
    "env two pairs",
    "env empty pair between two",
    "env pair without =",
    "env pair without key",
    "env unknown key skipped",
    "env later pair wins",
    "env negative value stored",
    "env value through atoi",
    "env split at the first =",
    "env trailing comma",
    "env empty string",
    "env negative value reads as the default",
)
PER_SITE = ("dct_wgs_per_cu", "qr_wgs_per_cu", "intra_rough_waves", "qr8_wgs_per_cu", "service_spin_us")


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("tuning_host")
    src, exe = d / "tuning_host.cpp", d / "tuning_host"
    src.write_text(PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-I", os.path.join(ROOT, "kvazaar_amd", "csrc"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return r.stdout


def test_lookups_and_parser_on_directed_cases(program_output):
    got = dict(line.rsplit(": ", 1) for line in program_output.splitlines() if line.endswith((": ok", ": WRONG")))
    assert sorted(got) == sorted(CASES), program_output
    for name in CASES:
        assert got[name] == "ok", program_output


def test_table_as_compiled_is_the_table_as_parsed(program_output):
    """what the tests read out of tuning.h with a regular expression is what the compiler made of it: 43 keys, five of them per site"""
    compiled = [tuple(line.split()[1:]) for line in program_output.splitlines() if line.startswith("key ")]
    table = tuning_table()
    assert compiled == [(k, "per-site" if d is None else str(d)) for k, d in table]
    assert len(table) == 43
    assert tuple(k for k, d in table if d is None) == PER_SITE


def tuning_comment():
    """the lines of the comment above kvz_hip_set_tuning in include/kvz_hip.h"""
    text = open(os.path.join(ROOT, "include", "kvz_hip.h")).read()
    end = text.index("KVZ_HIP_API int kvz_hip_set_tuning(")
    return text[text.rindex("/*", 0, end):end].splitlines()


def test_header_comment_names_every_key_with_its_default():
    lines = tuning_comment()
    for key, dflt in tuning_table():
        own = [ln for ln in lines if re.match(r'\s*\*\s+"%s"\s\s' % key, ln)]          # a row of the list: the key, then a column's gap
        assert len(own) == 1, "%s: %d rows of the comment's list begin with the quoted key" % (key, len(own))
        m = re.match(r'\s*\*\s+"%s"\s+(per site|-?\d+)\s' % key, own[0])
        assert m and m.group(1) == ("per site" if dflt is None else str(dflt)), "%s: %r" % (key, own[0])
    listed = [m.group(1) for ln in lines for m in [re.match(r'\s*\*\s+"(\w+)"\s+(per site|-?\d+)\s', ln)] if m]
    assert listed == [k for k, _ in tuning_table()]          # and no line for a key that does not exist
    assert not any("{" in ln for ln in lines)                # no brace-expanded group of keys


def test_no_call_site_reads_a_knob_by_string():
    d = os.path.join(ROOT, "kvazaar_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            hits = re.findall(r'\btuning(?:_or|_is_set)?\s*(?:<[^>]*>)?\s*\(\s*"', open(os.path.join(d, name)).read())
            assert not hits, "%s: %s" % (name, hits)


@pytest.mark.parametrize("call, says", [("tuning<tune::dct_wgs_per_cu>()", "per call site"), ("tuning_or<tune::sad_wgs_per_cu>(1)", "in the table"),
                                        ("tuning<tune::no_such_key>()", "no_such_key")])
def test_the_wrong_lookup_for_a_key_does_not_compile(tmp_path, call, says):
    src = tmp_path / "wrong_lookup.cpp"
    src.write_text('#include "tuning.h"\nusing namespace kvzhip;\nint main() { return %s; }\n' % call)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "kvazaar_amd", "csrc"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 0 and says in r.stdout, r.stdout
