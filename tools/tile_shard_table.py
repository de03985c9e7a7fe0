"""CPU: rows against tiles for N = 1..8 at 3840x2160 and 1920x1080 -- the grid tile_grid picks, ideal_speedup by PU counts (full
8/16/32/64 PUs: total / largest rank), the interior / boundary PU split of the search (CTUs >= BOUNDARY_CTU_ROWS from every shared
edge / the rest) and the largest per-rank halo in bytes per plane per frame (margin 80; a rank receives as much as it sends).
Arithmetic on the geometry of kvazaar_amd/shard.py, no measurement."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvazaar_amd import shard as S  # noqa: E402


def row_split(w, h, n):
    inner = bound = 0
    for r in range(n):
        sh = S.RowShard(w, h, n, r, margin=0)
        for cy in range(sh.ctu_lo, sh.ctu_hi):
            near = (r > 0 and cy < sh.ctu_lo + S.BOUNDARY_CTU_ROWS) or (r < n - 1 and cy >= sh.ctu_hi - S.BOUNDARY_CTU_ROWS)
            p = S.pus_in_rect(0, cy * 64, w, min(64, h - cy * 64))
            bound, inner = (bound + p, inner) if near else (bound, inner + p)
    return inner, bound


def tile_split(w, h, n):
    inner = bound = 0
    for r in range(n):
        t = S.TileShard(w, h, n, r)
        for cy in range(t.cy_lo, t.cy_hi):
            for cx in range(t.cx_lo, t.cx_hi):
                p = S.pus_in_rect(cx * 64, cy * 64, min(64, w - cx * 64), min(64, h - cy * 64))
                inner, bound = (inner + p, bound) if t.ctu_is_interior(cx, cy) else (inner, bound + p)
    return inner, bound


def main():
    hdr = "%-9s %2s | %-5s %6s %9s %9s %9s | %-5s %6s %9s %9s %9s" % (
        "frame", "N", "rows", "ideal", "interior", "boundary", "halo B", "tiles", "ideal", "interior", "boundary", "halo B")
    print(hdr)
    print("-" * len(hdr))
    for (w, h) in ((3840, 2160), (1920, 1080)):
        for n in range(1, 9):
            rows = S.row_shard_pus(w, h, n)
            r_in, r_bd = row_split(w, h, n)
            r_halo = max(S.tile_halo_bytes(w, h, 1, n))
            cols, trows = S.tile_grid(w, h, n)
            tiles = [S.TileShard(w, h, n, r).pus() for r in range(n)]
            t_in, t_bd = tile_split(w, h, n)
            t_halo = max(S.tile_halo_bytes(w, h, cols, trows))
            print("%-9s %2d | %-5s %6.3f %9d %9d %9d | %-5s %6.3f %9d %9d %9d" % (
                "%dx%d" % (w, h), n, "1x%d" % n, S.ideal_speedup(rows), r_in, r_bd, r_halo,
                "%dx%d" % (cols, trows), S.ideal_speedup(tiles), t_in, t_bd, t_halo))


if __name__ == "__main__":
    main()
