"""GPU: the rectangle-copy kernel (kvz_hip_copy_rects_batch) and the tile halo exchange built on it (kvz_hip_tile_halo_exchange,
kvazaar_amd/shard.py exchange_tile_halo_into) against numpy, against the row exchange kvz_hip_halo_exchange, and the search of a
tile's PU groups against the unsharded search under the same frame-coordinate rectangles."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from kvazaar_amd import _lib
    lib = _lib.init(0)
    yield lib
    assert lib.kvz_hip_set_device(0) == 0


def _random_rects(g, src_bytes, n):
    """n rects with widths 1..300, any alignment; destinations laid out one after the other (no overlap), some rects empty"""
    rects, dst_off = [], 0
    for i in range(n):
        kind = i % 4
        w = int(g.integers(1, 301))
        h = int(g.integers(1, 41))
        if kind == 0:                                            # 16-byte pointers and strides
            ss, ds = (w + 15) // 16 * 16 + 16 * int(g.integers(0, 3)), (w + 15) // 16 * 16 + 16 * int(g.integers(0, 3))
            so, pad = 16 * int(g.integers(0, 64)), 16 * int(g.integers(0, 4))
        elif kind == 1:                                          # 8-byte
            ss, ds = (w + 7) // 8 * 8 + 8, (w + 7) // 8 * 8
            so, pad = 8 * int(g.integers(0, 64)) + 8, 8
        else:                                                    # arbitrary
            ss, ds = w + int(g.integers(0, 37)), w + int(g.integers(0, 37))
            so, pad = int(g.integers(0, 1000)), int(g.integers(0, 16))
        if i % 7 == 6:
            w, h = (0, h) if i % 2 else (w, 0)
        dst_off += pad
        assert so + (max(h, 1) - 1) * ss + w <= src_bytes
        rects.append((so, dst_off, ss, ds, w, h))
        dst_off += max(h, 1) * ds + 16
    return rects, dst_off


def _emulate(src, dst, rects):
    for (so, do, ss, ds, w, h) in rects:
        for r in range(h):
            dst[do + r * ds:do + r * ds + w] = src[so + r * ss:so + r * ss + w]


def test_copy_rects_matches_numpy(L):
    from kvazaar_amd import api, _lib
    g = np.random.default_rng(31)
    src = g.integers(0, 256, 2 << 20, dtype=np.uint8)
    d_src = api.DeviceBuffer.from_numpy(src)
    for trial, n in enumerate([1, 2, 5, 8, 13, _lib.MAX_RECTS, _lib.MAX_RECTS]):
        rects, dst_bytes = _random_rects(g, src.size, n)
        init = np.full(dst_bytes, 0xA5, np.uint8)
        d_dst = api.DeviceBuffer.from_numpy(init)
        api.copy_rects([(d_src.ptr + so, d_dst.ptr + do, ss, ds, w, h) for (so, do, ss, ds, w, h) in rects])
        want = init.copy()
        _emulate(src, want, rects)
        np.testing.assert_array_equal(d_dst.to_numpy(np.uint8, (dst_bytes,)), want, err_msg="trial %d" % trial)
    # a single tall 80-byte strip (a luma column halo) and a wide one with a ragged end
    for (w, h, ss, ds) in ((80, 1000, 1120, 80), (1000, 3, 1008, 1024)):
        init = np.zeros(h * ds, np.uint8)
        d_dst = api.DeviceBuffer.from_numpy(init)
        api.copy_rects([(d_src.ptr + 32, d_dst.ptr, ss, ds, w, h)])
        _emulate(src, init, [(32, 0, ss, ds, w, h)])
        np.testing.assert_array_equal(d_dst.to_numpy(np.uint8, (h * ds,)), init)


def test_copy_rects_refusals(L):
    from kvazaar_amd import api, _lib
    b = api.DeviceBuffer(4096)
    R = _lib.RectCopy

    def call(rects, n=None):
        arr = (R * max(1, len(rects)))(*rects)
        return L.kvz_hip_copy_rects_batch(arr if rects else None, len(rects) if n is None else n, None)
    ok = R(b.ptr, b.ptr + 2048, 64, 64, 64, 4)
    assert call([]) == 0 and call([R(b.ptr, b.ptr + 2048, 64, 64, 0, 5), R(None, None, 0, 0, 7, 0)]) == 0     # no-ops
    assert call([ok] * 17) == -2 and call([ok], n=-1) == -2
    assert L.kvz_hip_copy_rects_batch(None, 1, None) == -2
    assert call([R(b.ptr, b.ptr + 2048, 64, 64, -1, 4)]) == -2
    assert call([R(None, b.ptr + 2048, 64, 64, 8, 4)]) == -2
    assert call([R(b.ptr, b.ptr + 2048, 32, 64, 64, 4)]) == -2          # stride < w
    assert call([ok]) == 0
    assert L.kvz_hip_stream_sync(None) == 0


def _tile_planes(api, L, shards, plane, ndev, extra_stride=0, halo_fill=0):
    from kvazaar_amd import _lib
    bufs, recs = [], []
    for i, t in enumerate(shards):
        dev = i % ndev
        assert L.kvz_hip_set_device(dev) == 0
        stride = t.ext_w + extra_stride
        ext = np.full((t.ext_h, stride), halo_fill, np.uint8)
        ext[t.top:t.top + t.own_h, t.left:t.left + t.own_w] = plane[t.y_lo:t.y_hi, t.x_lo:t.x_hi]
        b = api.DeviceBuffer.from_numpy(ext)
        bufs.append(b)
        recs.append(_lib.TilePlane(b.ptr, dev, stride, *(t.ext + t.own)))
    return bufs, recs


@pytest.mark.parametrize("grid", [(2, 2), (4, 2)])
@pytest.mark.parametrize("plane_kind", ["luma", "chroma"])
def test_tile_halo_exchange_4k(L, grid, plane_kind):
    """every tile pushes into its up to 8 neighbours (device i % count); afterwards every extended buffer equals its crop"""
    from kvazaar_amd import api, shard as S
    ndev = L.kvz_hip_device_count()
    W, H, margin, ctu, extra = (3840, 2160, 80, 64, 0) if plane_kind == "luma" else (1920, 1080, 40, 32, 24)
    world = grid[0] * grid[1]
    plane = np.random.default_rng(41 + world).integers(0, 256, (H, W), dtype=np.uint8)
    shards = [S.TileShard(W, H, world, r, margin, margin, grid=grid, ctu=ctu) for r in range(world)]
    bufs, recs = _tile_planes(api, L, shards, plane, ndev, extra_stride=extra, halo_fill=0xEE)
    for r, t in enumerate(shards):
        assert L.kvz_hip_set_device(recs[r].device) == 0
        api.tile_halo_exchange(recs[r], [recs[nb] for nb in t.neighbours()])
        assert L.kvz_hip_stream_sync(None) == 0
    for r, t in enumerate(shards):
        assert L.kvz_hip_set_device(recs[r].device) == 0
        got = bufs[r].to_numpy(np.uint8, (t.ext_h, t.ext_w + extra))[:, :t.ext_w]
        np.testing.assert_array_equal(got, plane[t.ext_y0:t.ext_y0 + t.ext_h, t.ext_x0:t.ext_x0 + t.ext_w], err_msg="tile %d" % r)
    assert L.kvz_hip_set_device(0) == 0


def test_tile_halo_exchange_refusals(L):
    from kvazaar_amd import api, _lib, shard as S
    ndev = L.kvz_hip_device_count()
    W, H = 640, 512
    plane = np.zeros((H, W), np.uint8)
    shards = [S.TileShard(W, H, 4, r, grid=(2, 2)) for r in range(4)]
    bufs, recs = _tile_planes(api, L, shards, plane, 1)
    assert L.kvz_hip_set_device(0) == 0
    T = _lib.TilePlane

    def call(me, nbs, n=None):
        arr = (T * max(1, len(nbs)))(*nbs)
        return L.kvz_hip_tile_halo_exchange(C.byref(me), arr if nbs else None, len(nbs) if n is None else n, None)
    assert call(recs[0], [recs[1], recs[2], recs[3]]) == 0
    assert call(recs[0], []) == 0
    assert call(recs[0], [recs[0]]) == -2                                     # own rectangles overlap
    assert call(recs[0], [recs[1], recs[1]]) == -2
    bad = T(*[getattr(recs[1], f) for f, _ in T._fields_])
    bad.own_x = bad.ext_x - 1                                                 # own not inside ext
    assert call(recs[0], [bad]) == -2
    bad = T(*[getattr(recs[0], f) for f, _ in T._fields_])
    bad.stride = bad.ext_w - 1
    assert call(bad, [recs[1]]) == -2
    assert call(recs[0], [recs[1]] * 9, n=9) == -2
    assert L.kvz_hip_tile_halo_exchange(C.byref(recs[0]), None, 1, None) == -2
    bad = T(*[getattr(recs[0], f) for f, _ in T._fields_])
    bad.device = 63                                                           # a device that was never initialised
    assert call(recs[1], [bad]) == -2
    if ndev >= 2:
        assert L.kvz_hip_set_device(1) == 0
        assert call(recs[0], [recs[1]]) == -2                                  # the calling thread does not work on self->device
        assert L.kvz_hip_set_device(0) == 0
    assert L.kvz_hip_stream_sync(None) == 0


def test_row_layout_equals_halo_exchange(L):
    """a full-width row shard is a tile: kvz_hip_tile_halo_exchange gives byte for byte what kvz_hip_halo_exchange gives"""
    from kvazaar_amd import api, _lib, shard as S
    W, H, margin, world = 256, 64 * 7 + 24, 40, 3
    plane = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)

    class ShardPlane(C.Structure):
        _fields_ = [("ext", C.c_void_p), ("device", C.c_int32), ("top", C.c_int32), ("rows", C.c_int32)]
    shards = [S.RowShard(W, H, world, r, margin) for r in range(world)]
    a, b, ra, rb = [], [], [], []
    for sh in shards:
        ext = np.full((sh.ext_rows, W), 0x5A, np.uint8)
        ext[sh.top:sh.top + sh.rows] = plane[sh.y_lo:sh.y_hi]
        a.append(api.DeviceBuffer.from_numpy(ext))
        b.append(api.DeviceBuffer.from_numpy(ext))
        ra.append(ShardPlane(a[-1].ptr, 0, sh.top, sh.rows))
        rb.append(_lib.TilePlane(b[-1].ptr, 0, W, 0, sh.ext_lo, W, sh.ext_rows, 0, sh.y_lo, W, sh.rows))
    for r in range(world):
        up = C.byref(ra[r - 1]) if r > 0 else None
        down = C.byref(ra[r + 1]) if r < world - 1 else None
        _lib.check(L.kvz_hip_halo_exchange(C.byref(ra[r]), up, down, W, margin, None), "halo_exchange")
        api.tile_halo_exchange(rb[r], [rb[q] for q in (r - 1, r + 1) if 0 <= q < world])
    assert L.kvz_hip_stream_sync(None) == 0
    for r, sh in enumerate(shards):
        got_a = a[r].to_numpy(np.uint8, (sh.ext_rows, W))
        np.testing.assert_array_equal(b[r].to_numpy(np.uint8, (sh.ext_rows, W)), got_a)
        np.testing.assert_array_equal(got_a, plane[sh.ext_lo:sh.ext_hi])


def test_tile_search_groups_equal_unsharded_search(L):
    """kvz_hip_search_pu_batch per tile group (interior under the own rectangle with the halo poisoned, boundary under the extended
    one) == the unsharded search of the same PUs under the same rectangles in frame coordinates"""
    import torch
    from kvazaar_amd import api, shard as S
    from patterns import ME_PU, me_params
    W, H, seed = 64 * 8 + 20, 64 * 6 + 40, 17
    pic = S.full_plane(torch, "cpu", W, H, seed, 1, 0).numpy()
    ref = S.full_plane(torch, "cpu", W, H, seed, 0, 1).numpy()
    n_groups = []
    for r in range(4):
        t = S.TileShard(W, H, 4, r, grid=(2, 2))
        ext_pic = pic[t.ext_y0:t.ext_y0 + t.ext_h, t.ext_x0:t.ext_x0 + t.ext_w]
        ext_ref = ref[t.ext_y0:t.ext_y0 + t.ext_h, t.ext_x0:t.ext_x0 + t.ext_w].copy()
        poisoned = 255 - ext_ref
        poisoned[t.top:t.top + t.own_h, t.left:t.left + t.own_w] = ext_ref[t.top:t.top + t.own_h, t.left:t.left + t.own_w]
        pus, _ = S.tile_pus(np, t, S.PU_SIZES, ME_PU)
        groups = S.tile_search_groups(np, t, pus)
        n_groups.append(len(groups))
        pf = pus.copy()
        pf["x"] += t.ext_x0
        pf["y"] += t.ext_y0
        for name, idx, tile in groups:
            prm = me_params(lambda_cost=20, mv_constraint=4, wpp_owf=0, tile=tile)
            got = api.search_pu_batch(ext_pic, poisoned if name == "interior" else ext_ref, pus[idx], prm)
            frame_tile = (tile[0] + t.ext_x0, tile[1] + t.ext_y0, tile[2], tile[3])
            want = api.search_pu_batch(pic, ref, pf[idx], me_params(lambda_cost=20, mv_constraint=4, wpp_owf=0, tile=frame_tile))
            np.testing.assert_array_equal(got, want, err_msg="tile %d, %s" % (r, name))
            assert (got[:, 2].view(np.uint32) != 0xFFFFFFFF).all() if got.size else True
    assert n_groups == [2, 2, 2, 2]


def _gloo_gpu_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    from kvazaar_amd import shard as S
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    W, H = 64 * 9 + 20, 64 * 6 + 40
    plane = torch.from_numpy(np.random.default_rng(23).integers(0, 256, (H, W), dtype=np.uint8))
    t = S.TileShard(W, H, world, rank, 80, 80, grid=(2, 2))
    ext = torch.zeros((t.ext_h, t.ext_w), dtype=torch.uint8, device=dev)
    ext[t.top:t.top + t.own_h, t.left:t.left + t.own_w] = plane[t.y_lo:t.y_hi, t.x_lo:t.x_hi].to(dev)
    staging = {}
    oks = []
    for _ in range(2):                                           # the second call reuses the staging buffers
        S.exchange_tile_halo_into(ext, t, dist, staging)
        torch.cuda.synchronize()
        oks.append(bool(torch.equal(ext.cpu(), plane[t.ext_y0:t.ext_y0 + t.ext_h, t.ext_x0:t.ext_x0 + t.ext_w])))
    res = [None] * world
    dist.all_gather_object(res, all(oks))
    if rank == 0:
        q.put(res)
    dist.barrier()
    dist.destroy_process_group()


def test_exchange_tile_halo_into_gpu_tensors_gloo():
    """exchange_tile_halo_into with GPU tensors at world 4 on a 2 x 2 grid over gloo: packing / unpacking by the copy kernel on the
    current torch stream, pinned host staging in between; every extended buffer equals its crop"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 34300 + (os.getpid() % 300)
    procs = [ctx.Process(target=_gloo_gpu_worker, args=(r, 4, port, q)) for r in range(4)]
    for p_ in procs:
        p_.start()
    res = q.get(timeout=300)
    for p_ in procs:
        p_.join(120)
        assert p_.exitcode == 0
    assert res == [True] * 4
