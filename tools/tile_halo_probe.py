"""GPU: times the tile halo exchange of one 4K 4:2:0 frame on ONE device -- 8 tiles in a 4 x 2 grid, luma (margin 80, 64-pixel
CTUs) and both chroma planes (margin 40, 32-pixel CTUs): every tile's kvz_hip_tile_halo_exchange (one launch of the rectangle-copy
kernel each, up to 8 regions), 24 calls per frame.  Device-event timing of many frames after a warm-up; the kernel time itself
comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.  On one device the pushes are device-local copies:
this measures the kernel and the launches, not xGMI.
    python tools/tile_halo_probe.py [--frames 200] [--out probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kvazaar_amd import _lib, api, shard as S  # noqa: E402


def planes(L, W, H, margin, ctu, seed):
    plane = np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    shards = [S.TileShard(W, H, 8, r, margin, margin, grid=(4, 2), ctu=ctu) for r in range(8)]
    bufs, recs = [], []
    for t in shards:
        ext = np.zeros((t.ext_h, t.ext_w), np.uint8)
        ext[t.top:t.top + t.own_h, t.left:t.left + t.own_w] = plane[t.y_lo:t.y_hi, t.x_lo:t.x_hi]
        b = api.DeviceBuffer.from_numpy(ext)
        bufs.append(b)
        recs.append(_lib.TilePlane(b.ptr, 0, t.ext_w, *(t.ext + t.own)))
    calls = []
    for r, t in enumerate(shards):
        nbs = [recs[q] for q in t.neighbours()]
        calls.append((recs[r], (_lib.TilePlane * len(nbs))(*nbs), len(nbs)))
    moved = sum(s[2] * s[3] for t in shards for (_, s, _) in S.exchange_regions(t))
    return plane, shards, bufs, calls, moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.init(0)
    sets = {"luma": planes(L, 3840, 2160, 80, 64, 1), "cb": planes(L, 1920, 1080, 40, 32, 2), "cr": planes(L, 1920, 1080, 40, 32, 3)}

    def run(names):
        for nm in names:
            for (me, nbs, n) in sets[nm][3]:
                rc = L.kvz_hip_tile_halo_exchange(C.byref(me), nbs, n, None)
                if rc:
                    _lib.check(rc, "tile_halo_exchange")
    e0, e1 = L.kvz_hip_event_create(), L.kvz_hip_event_create()

    def timed(names):
        for _ in range(a.warmup):
            run(names)
        _lib.check(L.kvz_hip_stream_sync(None), "sync")
        _lib.check(L.kvz_hip_event_record(e0, None), "event")
        for _ in range(a.frames):
            run(names)
        _lib.check(L.kvz_hip_event_record(e1, None), "event")
        ms = C.c_float()
        _lib.check(L.kvz_hip_event_elapsed_ms(e0, e1, C.byref(ms)), "elapsed")
        return ms.value / a.frames
    out = {"device": L.kvz_hip_device_name().decode(), "frames": a.frames, "grid": [4, 2]}
    out["frame_ms"] = timed(["luma", "cb", "cr"])
    out["luma_ms"] = timed(["luma"])
    out["calls_per_frame"] = 24
    out["us_per_call"] = out["frame_ms"] * 1000.0 / 24
    out["bytes_per_frame"] = sum(s[4] for s in sets.values())
    out["luma_bytes"] = sets["luma"][4]
    out["GB_per_s"] = out["bytes_per_frame"] / (out["frame_ms"] * 1e-3) / 1e9
    for nm, (plane, shards, bufs, _, _) in sets.items():        # the buffers hold their crops after the exchange
        for t, b in zip(shards, bufs):
            got = b.to_numpy(np.uint8, (t.ext_h, t.ext_w))
            assert (got == plane[t.ext_y0:t.ext_y0 + t.ext_h, t.ext_x0:t.ext_x0 + t.ext_w]).all(), (nm, t.rank)
    out["verified"] = True
    L.kvz_hip_event_destroy(e0)
    L.kvz_hip_event_destroy(e1)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
