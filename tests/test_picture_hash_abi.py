"""CPU: the declarations of the hash stage -- kvz_hip_picture_hash_frame, kvz_hip_picture_hash_frames, kvz_hip_array_checksum_batch with
its host-only helper, and kvz_strategy_register_nal_hip: declared, documented, exported and bound; kvz_hip_lcu_hash,
kvz_hip_picture_hash, kvz_hip_hash_picture and kvz_hip_hash_plane in C99, in ctypes and in the header's comments; the ABI version
unchanged; the record checks of kvazaar_amd/csrc/chain_host.h as a host program; without a device the entries refuse before they look
at anything."""
import ctypes
import inspect
import os
import re
import subprocess

import test_abi as A

ENTRIES = ("kvz_hip_picture_hash_frame", "kvz_hip_picture_hash_frames", "kvz_hip_array_checksum_blocks", "kvz_hip_array_checksum_batch",
           "kvz_strategy_register_nal_hip")
FIELDS = ("width", "height", "chroma", "reserved", "src", "rec_y", "rec_u", "rec_v", "stride_y", "stride_c", "lcu_out", "out")
OFFSETS = [0, 4, 8, 12, 16, 56, 64, 72, 80, 84, 88, 96]
SIZE = 104
PLANE_FIELDS, PLANE_OFFSETS, PLANE_SIZE = ("data", "width", "height", "stride", "reserved"), [0, 8, 12, 16, 20], 24

RECORD = "planes and strides must be 4-byte aligned, strides >= the width, width / height multiples of 8"
OUTPUTS = "lcu_out or out is null or misaligned"
CHROMA = "a chroma plane is null or misaligned, or its stride is"
SRC_SIZE = "src.width / src.height differ from width / height"
SRC_PLANE = "a src plane is null or misaligned, or its stride is"
SHARED = "an output shared with another picture"


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def test_header_declares_and_library_exports_the_entries():
    L = _lib()
    from kvazaar_amd import _lib as B
    exported = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB], text=True)
    for name in ENTRIES:
        assert name.startswith("kvz_") and name in A.declared_symbols() and hasattr(L, name) and hasattr(B.load(), name)
        assert re.search(r"\bT %s\b" % name, exported), name
    P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    assert B.SIGNATURES["kvz_hip_picture_hash_frame"] == (I, [P, P, U, P, P, U, I, I, I, P, P, P])
    assert B.SIGNATURES["kvz_hip_picture_hash_frames"] == (I, [ctypes.POINTER(B.HashPicture), I, P])
    assert B.SIGNATURES["kvz_hip_array_checksum_blocks"] == (ctypes.c_size_t, [I, I])
    assert B.SIGNATURES["kvz_hip_array_checksum_batch"] == (I, [ctypes.POINTER(B.HashPlane), I, P, P, P])
    assert B.SIGNATURES["kvz_strategy_register_nal_hip"] == (I, [P, ctypes.c_uint8])
    # no array_md5 anywhere in the library's interface: the selector keeps generic for it
    assert "array_md5" not in re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    strategy = open(os.path.join(A.ROOT, "kvazaar_amd", "csrc", "strategy.hip")).read()
    assert 'reg(opaque, "array_checksum"' in strategy and 'reg(opaque, "array_md5"' not in strategy


def test_structs_in_c99_and_ctypes_and_in_the_header_comments(tmp_path):
    from kvazaar_amd import _lib as B
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %zu %d %d %d", sizeof(kvz_hip_lcu_hash), sizeof(kvz_hip_picture_hash), sizeof(kvz_hip_hash_picture),',
             '         sizeof(kvz_hip_hash_plane), KVZ_HIP_MAX_HASH_PLANES, KVZ_HIP_MAX_CHAIN_PICTURES, KVZ_HIP_ABI_VERSION);']
    lines += ['  printf(" %%zu", offsetof(kvz_hip_hash_picture, %s));' % f for f in FIELDS]
    lines += ['  printf(" %%zu", offsetof(kvz_hip_hash_plane, %s));' % f for f in PLANE_FIELDS]
    lines += ['  printf(" %%zu", offsetof(kvz_hip_lcu_hash, %s));' % f for f in ("checksum", "sse")]
    lines += ['  printf(" %%zu", offsetof(kvz_hip_picture_hash, %s));' % f for f in ("checksum", "n_lcu", "sse")]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [24, 40, SIZE, PLANE_SIZE, B.MAX_HASH_PLANES, B.MAX_CHAIN_PICTURES, 4] + OFFSETS + PLANE_OFFSETS + [0, 12] + [0, 12, 16]
    assert B.MAX_HASH_PLANES == 48
    assert ctypes.sizeof(B.LcuHash) == 24 and ctypes.sizeof(B.PictureHash) == 40
    assert [getattr(B.LcuHash, f).offset for f in ("checksum", "sse")] == [0, 12]
    assert [getattr(B.PictureHash, f).offset for f in ("checksum", "n_lcu", "sse")] == [0, 12, 16]
    for struct, fields, offsets, size in ((B.HashPicture, FIELDS, OFFSETS, SIZE), (B.HashPlane, PLANE_FIELDS, PLANE_OFFSETS, PLANE_SIZE)):
        assert ctypes.sizeof(struct) == size and [getattr(struct, f).offset for f in fields] == offsets
        assert [f for f, _ in struct._fields_] == list(fields)
        # no implicit padding: the fields fill the record
        assert [o + getattr(struct, f).size for o, f in zip(offsets, fields)] == offsets[1:] + [size]
    from kvazaar_amd import api
    assert api.LCU_HASH.itemsize == 24 and api.PICTURE_HASH.itemsize == 40
    assert [api.PICTURE_HASH.fields[f][1] for f in ("checksum", "n_lcu", "sse")] == [0, 12, 16]
    # the header states what the compiler says
    text = open(A.HEADER).read()
    for end, fields, offsets in (("} kvz_hip_hash_picture;", FIELDS, OFFSETS), ("} kvz_hip_hash_plane;", PLANE_FIELDS, PLANE_OFFSETS)):
        decl = text[:text.index(end)]
        decl = decl[decl.rindex("typedef struct {"):]
        stated = {}
        for line in decl.splitlines():
            m = re.match(r"\s*(?:const )?[\w ]+?[ *]([\w, *]+);\s*/\*\s*([\d, ]+)[: ]", line)
            if m:
                names = [n.strip(" *") for n in m.group(1).split(",")]
                offs = [int(v) for v in m.group(2).split(",")]
                assert len(offs) == len(names), line
                stated.update(zip(names, offs))
        assert stated == dict(zip(fields, offsets)), end
    for name, size in (("kvz_hip_lcu_hash", 24), ("kvz_hip_picture_hash", 40), ("kvz_hip_hash_picture", SIZE), ("kvz_hip_hash_plane", PLANE_SIZE)):
        assert re.search(r"\} %s;\s+/\* %d bytes\b" % (name, size), text), name


def test_header_and_design_say_why_md5_stays_out():
    text = open(A.HEADER).read()
    doc = text[text.index("nal group and the last stage of the picture chain"):text.index("KVZ_HIP_API int kvz_hip_array_checksum_batch")]
    for what in ("mod 2^32", "(x >> 8) ^ (y >> 8)) & 255", "big-endian", "MD5 IS LEFT OUT ON PURPOSE", "serial dependency chain", "ignores stride",
                 "No array_md5 is registered", "THE RULE", "byte for byte", "picture 2", "No atomics on memory", "kvz_hip_graph_begin",
                 "KVZ_HIP_ERR_INVALID", "KVZ_HIP_ERR_NO_DEVICE", "checksum only", "never read"):
        assert what in doc, what
    design = open(os.path.join(A.ROOT, "DESIGN.md")).read()
    assert "array_md5" in design and "serial" in design and "ignores" in design


def test_numpy_conveniences_exist():
    from kvazaar_amd import api
    assert list(inspect.signature(api.picture_hash_frame).parameters) == ["rec", "src", "chroma"]
    assert list(inspect.signature(api.picture_hash_frames).parameters) == ["pictures"]
    assert list(inspect.signature(api.array_checksum_batch).parameters) == ["planes"]


def test_abi_version_is_still_4():
    L = _lib()
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4


def test_block_count_helper_needs_no_device():
    L = _lib()
    f = L.kvz_hip_array_checksum_blocks
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]
    assert [f(1, 1), f(64, 64), f(65, 64), f(13, 7), f(4352, 4096), f(65536, 65536)] == [1, 1, 2, 1, 68 * 64, 1024 * 1024]
    assert [f(0, 8), f(8, 0), f(-1, 8), f(65537, 8), f(8, 65537)] == [0] * 5


def test_argument_checks_return_invalid_or_no_device():
    """with a device NULL records and a count out of range are refused as invalid; without one the entries say so before they look at
    anything"""
    import torch
    from kvazaar_amd import _lib as B
    L = B.load()
    text = open(A.HEADER).read()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", text).group(1))
    invalid = int(re.search(r"KVZ_HIP_ERR_INVALID\s*=?\s*(-?\d+)", text).group(1))
    have = torch.cuda.is_available()
    want = invalid if have else no_device
    records, planes = (B.HashPicture * 17)(), (B.HashPlane * 49)()
    f = L.kvz_hip_picture_hash_frames
    assert f(None, 1, None) == want and f(records, 17, None) == want and f(records, -1, None) == want and f(records, 1, None) == want
    assert f(None, 0, None) == (0 if have else no_device)
    assert L.kvz_hip_picture_hash_frame(None, None, 0, None, None, 0, 8, 8, 1, None, None, None) == want
    g = L.kvz_hip_array_checksum_batch
    assert g(None, 1, None, None, None) == want and g(planes, 49, None, None, None) == want and g(planes, 1, None, None, None) == want
    assert g(None, 0, None, None, None) == (0 if have else no_device)


PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <functional>
#include <string>

#include "kvz_hip.h"
#include "chain_host.h"

static std::string last_message;
void kvzhip::set_error_msg(const char *what) { last_message = what; }

// a pointer value that nothing is ever read through: slot k of record i, 4 KB apart
template <typename T> static T *fake(int i, int k) { return (T *)(uintptr_t)(0x10000000u + 0x100000u * (unsigned)i + 0x1000u * (unsigned)k); }
enum { MAX = KVZ_HIP_MAX_CHAIN_PICTURES };

// record i of a clean call: 72x40 and 8x8 in turn, 4:2:0 and 4:0:0 in turn of two, every third without a source
static kvz_hip_hash_picture clean(int i)
{
  const int w = i % 2 ? 8 : 72, h = i % 2 ? 8 : 40;
  kvz_hip_hash_picture p;
  memset(&p, 0, sizeof p);
  p.width = w; p.height = h; p.chroma = (i / 2) % 2 ? 0 : 1;
  if (i % 3 != 2) {
    p.src.y = fake<kvz_hip_pixel>(i, 0);
    if (p.chroma) { p.src.u = fake<kvz_hip_pixel>(i, 1); p.src.v = fake<kvz_hip_pixel>(i, 2); }
    p.src.stride_y = (uint32_t)w + 8; p.src.stride_c = (uint32_t)w / 2 + 20; p.src.width = w; p.src.height = h;
  }
  p.rec_y = fake<kvz_hip_pixel>(i, 3);
  if (p.chroma) { p.rec_u = fake<kvz_hip_pixel>(i, 4); p.rec_v = fake<kvz_hip_pixel>(i, 5); }
  p.stride_y = (uint32_t)w + 24; p.stride_c = (uint32_t)w / 2 + 12;
  p.lcu_out = fake<kvz_hip_lcu_hash>(i, 6); p.out = fake<kvz_hip_picture_hash>(i, 7);
  return p;
}

static void picture_case(const char *name, int n, const std::function<void(kvz_hip_hash_picture *)> &plant)
{
  kvz_hip_hash_picture p[MAX];
  for (int i = 0; i < n; ++i) p[i] = clean(i);
  plant(p);
  for (int i = 0; i < n; ++i)
    if (const char *w = hash_record_why(p, i)) {
      refuse_picture("entry", i, w);
      char head[64];
      snprintf(head, sizeof head, "entry: invalid argument in picture %d (", i);
      if (last_message != std::string(head) + w + ")") { printf("%s: MESSAGE %s\n", name, last_message.c_str()); return; }
      printf("%s: %d %s\n", name, i, w);
      return;
    }
  printf("%s: ok\n", name);
}

static void plane_case(const char *name, const kvz_hip_hash_plane &p)
{
  const char *w = hash_plane_why(p);
  printf("%s: %s\n", name, w ? w : "ok");
}

int main()
{
  typedef kvz_hip_hash_picture P;
  picture_case("clean", MAX, [](P *) {});
  picture_case("lcu_out null", 3, [](P *p) { p[2].lcu_out = nullptr; });
  picture_case("out null", 3, [](P *p) { p[1].out = nullptr; });
  picture_case("lcu_out misaligned", 3, [](P *p) { p[1].lcu_out = (kvz_hip_lcu_hash *)((uintptr_t)p[1].lcu_out + 2); });
  picture_case("out misaligned", 3, [](P *p) { p[0].out = (kvz_hip_picture_hash *)((uintptr_t)p[0].out + 4); });
  picture_case("rec_y null", 3, [](P *p) { p[2].rec_y = nullptr; });
  picture_case("rec_y misaligned", 3, [](P *p) { p[0].rec_y += 2; });
  picture_case("stride_y misaligned", 3, [](P *p) { p[0].stride_y += 2; });
  picture_case("stride_y short", 3, [](P *p) { p[0].stride_y = 64; });
  picture_case("width 76", 3, [](P *p) { p[0].width = p[0].src.width = 76; });
  picture_case("height 0", 3, [](P *p) { p[1].height = p[1].src.height = 0; });
  picture_case("height 16392", 3, [](P *p) { p[0].height = p[0].src.height = 16392; });
  picture_case("rec_v null", 3, [](P *p) { p[0].rec_v = nullptr; });
  picture_case("rec_v null in 4:0:0", 3, [](P *p) { p[2].rec_v = nullptr; p[2].rec_u = nullptr; p[2].stride_c = 0; });
  picture_case("stride_c short", 3, [](P *p) { p[0].stride_c = 32; });
  picture_case("src of another size", 3, [](P *p) { p[1].src.width = 16; });
  picture_case("src.u null", 3, [](P *p) { p[0].src.u = nullptr; });
  picture_case("src.stride_y misaligned", 3, [](P *p) { p[0].src.stride_y += 1; });
  picture_case("no source, leftovers in src", 3, [](P *p) { p[0].src.y = nullptr; p[0].src.width = 3; p[0].src.stride_c = 1; });
  picture_case("lcu_out of record 0", 3, [](P *p) { p[2].lcu_out = p[0].lcu_out; });
  picture_case("out of record 1", 4, [](P *p) { p[3].out = p[1].out; });
  picture_case("shared inputs", 3, [](P *p) { p[2].rec_y = p[0].rec_y; p[1].src.y = p[0].src.y; });
  picture_case("outputs before planes", 3, [](P *p) { p[1].out = nullptr; p[1].rec_y = nullptr; });
  picture_case("record 1 before record 2", 3, [](P *p) { p[1].rec_y = nullptr; p[2].out = p[0].out; });

  const kvz_hip_hash_plane ok = { fake<kvz_hip_pixel>(0, 0) + 3, 13, 7, 29, 0 };
  plane_case("plane clean", ok);
  kvz_hip_hash_plane q = ok; q.data = nullptr; plane_case("plane data null", q);
  q = ok; q.width = 0; plane_case("plane width 0", q);
  q = ok; q.height = 65537; plane_case("plane height 65537", q);
  q = ok; q.stride = 12; plane_case("plane stride short", q);
  q = ok; q.width = 65536; q.stride = 65536; q.height = 1; plane_case("plane 65536 wide", q);
  printf("blocks: %zu %zu %zu\n", hash_plane_blocks(13, 7), hash_plane_blocks(4352, 4096), hash_plane_blocks(0, 5));
  return 0;
}
"""

EXPECTED = {
    "clean": None,
    "lcu_out null": (2, OUTPUTS),
    "out null": (1, OUTPUTS),
    "lcu_out misaligned": (1, OUTPUTS),
    "out misaligned": (0, OUTPUTS),
    "rec_y null": (2, RECORD),
    "rec_y misaligned": (0, RECORD),
    "stride_y misaligned": (0, RECORD),
    "stride_y short": (0, RECORD),
    "width 76": (0, RECORD),
    "height 0": (1, RECORD),
    "height 16392": (0, RECORD),
    "rec_v null": (0, CHROMA),
    "rec_v null in 4:0:0": None,
    "stride_c short": (0, CHROMA),
    "src of another size": (1, SRC_SIZE),
    "src.u null": (0, SRC_PLANE),
    "src.stride_y misaligned": (0, SRC_PLANE),
    "no source, leftovers in src": None,
    "lcu_out of record 0": (2, SHARED),
    "out of record 1": (3, SHARED),
    "shared inputs": None,
    "outputs before planes": (1, OUTPUTS),
    "record 1 before record 2": (1, RECORD),
}
EXPECTED_PLANES = {"plane clean": "ok", "plane data null": "data is null", "plane width 0": "width or height outside 1..65536",
                   "plane height 65537": "width or height outside 1..65536", "plane stride short": "stride below the width", "plane 65536 wide": "ok",
                   "blocks": "1 4352 0"}


def test_record_checks_as_a_host_program(tmp_path):
    """chain_host.h takes a plain C++17 compiler with kvz_hip.h alone: the checks compare pointers and never follow them"""
    src, exe = tmp_path / "hash_checks.cpp", tmp_path / "hash_checks"
    src.write_text(PROGRAM)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(A.ROOT, "include"), "-I", os.path.join(A.ROOT, "kvazaar_amd", "csrc"), str(src), "-o",
           str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got, planes = {}, {}
    for line in r.stdout.splitlines():
        name, _, verdict = line.partition(": ")
        if name.startswith("plane") or name == "blocks":
            planes[name] = verdict
            continue
        index, _, reason = verdict.partition(" ")
        got[name] = None if verdict == "ok" else (int(index), reason)
    assert got == EXPECTED
    assert planes == EXPECTED_PLANES
