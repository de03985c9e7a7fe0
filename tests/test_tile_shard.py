"""CPU: the 2-D tile partition of kvazaar_amd/shard.py (TileShard, tile_grid, exchange_regions, exchange_tile_halo_into and the
tile forms of the search workload) -- geometry for worlds 1-8, and the exchange and the sharded search at world 2 and 4 over gloo
with the oracle standing in for the GPU kernels (this is a test; the product never uses the oracle).  Asserted: every CTU in
exactly one tile, tiles never worse than rows, every extended buffer equal to the crop of the whole plane after the exchange
(corners included), sharded search == unsharded search under the same rectangles."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from kvazaar_amd import shard  # noqa: E402
from kvazaar_amd.shard import TileShard  # noqa: E402

SIZES = ((3840, 2160), (1920, 1080), (520, 300), (1000, 710))      # the last two ragged in both directions


@pytest.mark.parametrize("size", SIZES)
def test_tiles_partition_every_ctu_exactly_once(size):
    w, h = size
    ncx, ncy = (w + 63) // 64, (h + 63) // 64
    for world in range(1, 9):
        tiles = [TileShard(w, h, world, r, margin_x=0, margin_y=0) for r in range(world)]
        owner = np.full((ncy, ncx), -1)
        for t in tiles:
            assert (t.cols, t.rows) == (tiles[0].cols, tiles[0].rows) and t.cols * t.rows == world
            assert (owner[t.cy_lo:t.cy_hi, t.cx_lo:t.cx_hi] == -1).all()
            owner[t.cy_lo:t.cy_hi, t.cx_lo:t.cx_hi] = t.rank
            assert t.own == (t.cx_lo * 64, t.cy_lo * 64, min(t.cx_hi * 64, w) - t.cx_lo * 64, min(t.cy_hi * 64, h) - t.cy_lo * 64)
            ex, ey, ew, eh = t.ext
            assert 0 <= ex <= t.x_lo and t.x_hi <= ex + ew <= w and 0 <= ey <= t.y_lo and t.y_hi <= ey + eh <= h
            assert t.col == t.rank % t.cols and t.row == t.rank // t.cols           # raster order
        assert (owner >= 0).all()
        widths = [t.cx_hi - t.cx_lo for t in tiles]
        heights = [t.cy_hi - t.cy_lo for t in tiles]
        assert max(widths) - min(widths) <= 1 and max(heights) - min(heights) <= 1
        assert sum(t.pus() for t in tiles) == shard.pus_in_rect(0, 0, w, h)


def test_tile_grid_4k_and_the_rule():
    assert shard.tile_grid(3840, 2160, 2) == (2, 1)
    assert shard.tile_grid(3840, 2160, 8) == (4, 2)
    assert shard.tile_grid(3840, 2160, 4) == (4, 1)         # the ragged last CTU row tips 4 x 1 over 2 x 2
    assert shard.tile_grid(3840, 2160, 7) == (1, 7)         # 300 CTUs against 7 x 1's 306: the row partition
    assert shard.tile_grid(1920, 1080, 8) == (8, 1)
    tiles = [TileShard(3840, 2160, 8, r) for r in range(8)]
    for t in tiles:
        assert (t.cx_hi - t.cx_lo, t.cy_hi - t.cy_lo) == (15, 17)
        interior = [(cx, cy) for cx in range(t.cx_lo, t.cx_hi) for cy in range(t.cy_lo, t.cy_hi) if t.ctu_is_interior(cx, cy)]
        assert len(interior) in (11 * 15, 13 * 15)              # 65 % (three shared edges) or 76 % (two) of 255
    assert max(t.pus() for t in tiles) == 21675
    assert max(shard.tile_halo_bytes(3840, 2160, 4, 2)) == 263680 < 2 * 80 * 3840
    assert abs(shard.ideal_speedup([t.pus() for t in tiles]) - 172020 / 21675) < 1e-12


@pytest.mark.parametrize("size", [(3840, 2160), (1920, 1080)])
def test_tiles_never_do_worse_than_rows(size):
    w, h = size
    for world in range(1, 9):
        tiles = [TileShard(w, h, world, r).pus() for r in range(world)]
        rows = shard.row_shard_pus(w, h, world)
        assert sum(tiles) == sum(rows)
        assert shard.ideal_speedup(tiles) >= shard.ideal_speedup(rows) - 1e-12, world


@pytest.mark.parametrize("grid,world", [(None, 2), ((2, 2), 4), ((4, 2), 8), ((3, 3), 9), ((1, 3), 3)])
def test_exchange_regions_are_symmetric_and_fill_the_halo(grid, world):
    w, h, mx, my = 64 * 9 + 20, 64 * 7 + 40, 48, 40
    tiles = [TileShard(w, h, world, r, mx, my, grid=grid) for r in range(world)]
    regions = {t.rank: {nb: (s, r) for (nb, s, r) in shard.exchange_regions(t)} for t in tiles}
    for a in regions:
        for b, (send, recv) in regions[a].items():
            assert regions[b][a] == (recv, send)
            assert shard.rect_intersect(send, tiles[a].own) == send and shard.rect_intersect(recv, tiles[b].own) == recv
    for t in tiles:
        cover = np.zeros((t.ext_h, t.ext_w), np.int32)
        cover[t.top:t.top + t.own_h, t.left:t.left + t.own_w] += 1
        for (_, _, (x, y, rw, rh)) in shard.exchange_regions(t):
            cover[y - t.ext_y0:y - t.ext_y0 + rh, x - t.ext_x0:x - t.ext_x0 + rw] += 1
        assert (cover == 1).all(), "own + received != extended rectangle for rank %d" % t.rank
        assert len(shard.exchange_regions(t)) == len(t.neighbours())


def test_too_thin_tiles_raise_on_every_rank():
    for r in range(8):                                          # 10 CTU columns over 8: 2,2,1,1,... -> 64 < 80 columns
        with pytest.raises(ValueError):
            TileShard(640, 1080, 8, r, grid=(8, 1))
    for r in range(4):                                          # 4 CTU rows over 4: 64 < 80 rows
        with pytest.raises(ValueError):
            TileShard(1920, 256, 4, r, grid=(1, 4))
    TileShard(640, 1080, 8, 0, margin_x=64, grid=(8, 1))        # a margin that fits
    with pytest.raises(ValueError):
        TileShard(640, 1080, 4, 0, grid=(3, 1))                 # 3 x 1 does not hold 4 ranks


# ---- gloo: the exchange itself ----
def _exchange_worker(rank, world, port, grid, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = np.random.default_rng(13)
    W, H, mx, my = 64 * 5 + 24, 64 * 4 + 40, 48, 40
    plane = torch.from_numpy(g.integers(0, 256, (H, W), dtype=np.uint8))
    t = TileShard(W, H, world, rank, mx, my, grid=grid)
    ext = torch.zeros((t.ext_h, t.ext_w), dtype=torch.uint8)
    ext[t.top:t.top + t.own_h, t.left:t.left + t.own_w] = plane[t.y_lo:t.y_hi, t.x_lo:t.x_hi]
    shard.exchange_tile_halo_into(ext, t, dist)
    ok = bool(torch.equal(ext, plane[t.ext_y0:t.ext_y0 + t.ext_h, t.ext_x0:t.ext_x0 + t.ext_w]))
    res = [None] * world
    dist.all_gather_object(res, (ok, len(t.neighbours())))
    if rank == 0:
        q.put(res)
    dist.destroy_process_group()


@pytest.mark.parametrize("world,grid", [(2, None), (4, (2, 2))])
def test_tile_halo_exchange_gloo(world, grid):
    """after the exchange every extended buffer equals the crop of the whole plane; at 2 x 2 every rank has a corner neighbour"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33100 + world + (os.getpid() % 400) * 4
    procs = [ctx.Process(target=_exchange_worker, args=(r, world, port, grid, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    res = q.get(timeout=180)
    for p_ in procs:
        p_.join(60)
        assert p_.exitcode == 0
    assert all(ok for ok, _ in res), res
    if grid == (2, 2):
        assert [n for _, n in res] == [3, 3, 3, 3]


# ---- gloo: the sharded search of a tile, rehearsed with the oracle as the kernels ----
def _search_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import oracle_lib as O
    from patterns import ME_PU, me_params
    dev = torch.device("cpu")
    W, H, margin, frames, seed = 64 * 6 + 20, 64 * 5 + 40, 48, 2, 91      # 7 x 6 CTUs, ragged in both directions
    t = TileShard(W, H, world, rank, margin, margin, grid=(2, 2))
    pus, _ = shard.tile_pus(np, t, shard.PU_SIZES, ME_PU)
    pus = pus[::7]                                                  # the oracle takes ~1 ms per PU
    groups = shard.tile_search_groups(np, t, pus, boundary_ctus=1)  # margin 48 < 64: one CTU next to a shared edge reads halo
    assert groups[0][0] == "interior" and len(groups) == 2
    ext_ref = torch.zeros((t.ext_h, t.ext_w), dtype=torch.uint8)
    own_mask = torch.zeros_like(ext_ref, dtype=torch.bool)
    own_mask[t.top:t.top + t.own_h, t.left:t.left + t.own_w] = True
    results = []
    for f in range(1, frames + 1):
        ext_ref[t.top:t.top + t.own_h, t.left:t.left + t.own_w] = shard.tile_plane(torch, dev, t, seed, f - 1, 1, extended=False)
        pic = shard.tile_plane(torch, dev, t, seed, f, 0)
        res_f = {}
        name, idx, tile = groups[0]
        poisoned = ext_ref.clone()
        poisoned[~own_mask] = 255 - poisoned[~own_mask]              # the interior group runs while the halo is in flight
        res_f[name] = O.search_pu_batch(pic.numpy(), poisoned.numpy(), pus[idx], me_params(lambda_cost=20, mv_constraint=4, tile=tile))
        shard.exchange_tile_halo_into(ext_ref, t, dist)
        whole = shard.full_plane(torch, dev, W, H, seed, f - 1, 1)
        assert torch.equal(ext_ref, whole[t.ext_y0:t.ext_y0 + t.ext_h, t.ext_x0:t.ext_x0 + t.ext_w])
        for name, idx, tile in groups[1:]:
            res_f[name] = O.search_pu_batch(pic.numpy(), ext_ref.numpy(), pus[idx], me_params(lambda_cost=20, mv_constraint=4, tile=tile))
        results.append(res_f)
    gathered = [None] * world
    dist.all_gather_object(gathered, ((t.ext_x0, t.ext_y0), [(n, i, tl) for (n, i, tl) in groups], pus, results))
    if rank == 0:
        ok, total, found = True, 0, 0
        for ((ex, ey), grp, p, res_sh) in gathered:
            pf = p.copy()
            pf["x"] += ex
            pf["y"] += ey
            for (name, idx, tl) in grp:
                prm = me_params(lambda_cost=20, mv_constraint=4, tile=(tl[0] + ex, tl[1] + ey, tl[2], tl[3]))
                for f in range(1, frames + 1):
                    pic = shard.full_plane(torch, dev, W, H, seed, f, 0).numpy()
                    ref = shard.full_plane(torch, dev, W, H, seed, f - 1, 1).numpy()
                    want = O.search_pu_batch(pic, ref, pf[idx], prm)
                    got = res_sh[f - 1][name]
                    ok = ok and bool((want.view(np.int32) == got.view(np.int32)).all())
                    total += len(got)
                    found += int((got["cost"] != 0xFFFFFFFF).sum())
        q.put((ok, total, found, [len(g_[1]) for g_ in gathered]))
    dist.barrier()
    dist.destroy_process_group()


def test_tile_sharded_search_equals_unsharded_gloo():
    world = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33700 + (os.getpid() % 250)
    procs = [ctx.Process(target=_search_worker, args=(r, world, port, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    ok, total, found, n_groups = q.get(timeout=600)
    for p_ in procs:
        p_.join(60)
        assert p_.exitcode == 0
    assert ok, "a tile's search differs from the unsharded search under the same rectangles"
    assert found == total > 0
    assert n_groups == [2, 2, 2, 2]
