#!/usr/bin/env python3
"""One 1080p frame's worth of the batched entries, launched the three ways a host can launch them:

  eager    every entry enqueued on one stream, frame after frame
  graph    the frame's launch sequence captured once (kvz_hip_graph_begin/_end), replayed per frame
  graph4   the same, with the four independent stages (motion search, intra rough search, prediction + TU
           reconstruction + cost, SAO statistics) on forked streams = parallel branches of the graph
  graph7   the four motion-search launches (one per PU size class) on a branch each as well
  eager4/7 the forked streams without the graph

The per-frame batch sizes are the real ones (every PU / TU / LCU of one 1920x1080 frame, each size
once), so launch overhead, partial waves and tails count the way they do in an encoder -- unlike
tools/bench_all.py, whose batches are sized to hide them.  It is a measurement of the kernels on a
frame-sized workload, not of an encoder: the mode decision around them is not here.

  python tools/frame_pipeline.py [--frames 200] [--lcu-qp] [--tiles CxR] [--scaling-list [default|none]] [--transform-skip]
  python tools/frame_pipeline.py --lossless [--tiles CxR]
  python tools/frame_pipeline.py --pictures N [--tiles CxR] [--scaling-list [default|none]] [--transform-skip]

--lcu-qp: the picture chain of a frame whose QP changes per LCU (rate control, --roi): intra reconstruction through
kvz_hip_intra_recon_frame_qp with a QP array, then kvz_hip_cu_qp_frame (the QP map and the per-LCU predictor), and deblocking
with per_cu_qp = 1.
--tiles CxR: the picture is cut into C x R uniform tiles (the reference's spacing): the stages of the picture chain that depend on
tiles go through their *_tiles entries -- intra reconstruction, the QP map (with --lcu-qp), deblocking and the SAO reconstruction.
--scaling-list: the two stages that quantise go through their *_sl entries with the reference's default lists (the packed tables of
tests/golden/scaling_list.npz): the residual coding of the inter CUs (kvz_hip_inter_residual_frame_sl, after the motion compensation,
on its planes and its map) and the intra reconstruction (kvz_hip_intra_recon_frame_sl).  `none` passes tables == NULL: the same
entries, which then launch the kernels of the entries without lists -- the baseline of what the table reads cost.  Combines with
--lcu-qp and --tiles.
--transform-skip: both residual calls go through their *_ts entries with one bit cost, (int)(lambda + 0.5) at the frame's QP: every 4x4
luma TU is coded transformed and transform-skipped and the cheaper trial is kept.  Combines with --lcu-qp, --tiles and --scaling-list
(without --scaling-list the tables are NULL, as with `none`).
--cabac-cost (with --transform-skip): the two residual calls go through their *_ts_cabac entries: every trial is priced as the reference
does by default, with the CABAC counting coder on the context set of the TU's LCU (a set per LCU, fast_limit 0) instead of the estimate.
Run with and without it for the cost of the pricing.
--lossless: the picture chain of a frame coded with --lossless: prediction, then kvz_hip_inter_residual_frame_lossless and
kvz_hip_intra_recon_frame_lossless (implicit_rdpcm on), one kernel launch each.  The quantising batches, the QP map, deblocking and SAO
are left out: encoder.c:623-628 switches sign hiding, transform skip, deblocking and SAO off under --lossless.  Combines with --tiles
(the grid goes to the intra entry); --lcu-qp, --scaling-list and --transform-skip have no meaning without quantisation and are refused.
--pictures N (1..16): N independent pictures in flight.  All N are predicted by ONE kvz_hip_inter_recon_frames call over the pool of their
distinct reference pictures; then the two residual stages of all N go through ONE kvz_hip_inter_residual_frames and ONE
kvz_hip_intra_recon_frames call (one QP per picture).
Combines with --tiles, --scaling-list and --transform-skip: the two calls are then kvz_hip_inter_residual_frames_ts and
kvz_hip_intra_recon_frames_ts, every picture with the same grid, the same tables and the same bit cost.  The stages behind them take
all N pictures in one call each as well: kvz_hip_deblock_frames, kvz_hip_sao_stats_frames and kvz_hip_sao_frames, and with --lcu-qp
kvz_hip_cu_qp_frames after the intra stage.  --lossless (one launch per picture already) stays single-picture and is refused with
--pictures.
The last stage of a picture in every sequence is its hash, kvz_hip_picture_hash_frame on what kvz_hip_sao_frame wrote (with --lossless on
what the intra stage wrote; with --pictures kvz_hip_picture_hash_frames for all N): the SEI checksum and the squared error stay on the device.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from kvazaar_amd import _lib  # noqa: E402
from kvazaar_amd._lib import QuantParams  # noqa: E402

W, H = 1920, 1080


def build_stages(L, dev, lcu_qp=False, tiles=None, lists=None, trskip=False, lossless=False, pictures=0, cabac_cost=False):
    """-> {stage: [(name, units, launch(stream))]}, plus the tensors kept alive"""
    g = torch.Generator(device=dev); g.manual_seed(7)
    keep = []
    cur = torch.randint(0, 256, (H, W), dtype=torch.uint8, device=dev, generator=g)
    ref = torch.roll(cur, shifts=(1, 2), dims=(0, 1)).contiguous()
    noise = torch.randint(-6, 7, (H, W), dtype=torch.int16, device=dev, generator=g)
    pred = (cur.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
    keep += [cur, ref, pred]
    stages = {"me": [], "intra": [], "tu": [], "sao": []}      # "sao": the in-loop filter stage, deblocking + SAO statistics

    # the CU arrays the candidate derivation reads: this frame's (as if every neighbour were decided) and the collocated one's
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from patterns import inter_cu_map, inter_params
    ip = np.ascontiguousarray(inter_params(W, H, poc=8, ref_pocs=(7,), l0=(0,), col_ref_pocs=(6,), col_l0=(0,)))
    cu_now = torch.from_numpy(inter_cu_map(W, H, 1)[0].view(np.uint8).copy()).to(dev)
    cu_col = torch.from_numpy(inter_cu_map(W, H, 2)[0].view(np.uint8).copy()).to(dev)
    keep += [ip, cu_now, cu_col]
    me_prm = np.zeros(24, dtype=np.int32); me_prm[:8] = (20, 1, -1, 4, 0, 0, 1, 1)
    for n in (8, 16, 32, 64):
        xy = [(x, y) for y in range(0, H - n + 1, n) for x in range(0, W - n + 1, n)]
        pus = np.zeros((len(xy), 16), dtype=np.int32)
        pus[:, 0] = [p[0] for p in xy]; pus[:, 1] = [p[1] for p in xy]; pus[:, 2] = n; pus[:, 3] = n
        pus_d = torch.from_numpy(pus).to(dev)
        res_d = torch.empty((len(xy), 8), dtype=torch.int32, device=dev)
        prm = me_prm.copy(); prm[10] = 1 if n <= 16 else (2 if n <= 32 else 4)
        keep += [pus_d, res_d, prm]
        stages["me"].append(("inter_candidates_%dx%d" % (n, n), len(xy),
                             lambda s, pus_d=pus_d, k=len(xy): L.kvz_hip_inter_candidates_batch(
                                 cu_now.data_ptr(), cu_col.data_ptr(), cu_col.data_ptr(), ip.ctypes.data, pus_d.data_ptr(), k, None, s)))
        stages["me"].append(("search_pu_%dx%d" % (n, n), len(xy),
                             lambda s, pus_d=pus_d, res_d=res_d, k=len(xy), prm=prm: L.kvz_hip_search_pu_batch(
                                 cur.data_ptr(), W, W, H, ref.data_ptr(), W, W, H, pus_d.data_ptr(), k, prm.ctypes.data, res_d.data_ptr(), s)))

    flat_cur, flat_pred = cur.reshape(-1), pred.reshape(-1)
    for lg in (2, 3, 4, 5):
        n = 1 << lg
        cnt = (W // n) * (H // n)
        refs_d = torch.empty(cnt * 130, dtype=torch.uint8, device=dev)
        costs_d = torch.empty(cnt * 35, dtype=torch.int32, device=dev)
        pos_d = torch.tensor([(x, y) for y in range(0, H - n + 1, n) for x in range(0, W - n + 1, n)], dtype=torch.int32, device=dev)
        keep += [refs_d, costs_d, pos_d]
        stages["intra"].append(("intra_build_reference_%dx%d" % (n, n), cnt,
                                lambda s, lg=lg, cnt=cnt, refs_d=refs_d, pos_d=pos_d: L.kvz_hip_intra_build_reference_batch(
                                    lg, 0, pred.data_ptr(), W, W, H, pos_d.data_ptr(), cnt, refs_d.data_ptr(), s)))
        stages["intra"].append(("intra_rough_%dx%d" % (n, n), cnt,
                                lambda s, lg=lg, cnt=cnt, refs_d=refs_d, costs_d=costs_d: L.kvz_hip_intra_rough_batch(
                                    lg, 3, refs_d.data_ptr(), flat_cur.data_ptr(), cnt, costs_d.data_ptr(), None, s)))

    # prediction: the motion compensation of the whole picture from its CU array, the producer of the TU stage's pred_in (it
    # leads that stage's branch in the forked forms)
    import inter_recon_cases as IC
    from kvazaar_amd import api
    rc_cus, rc_LX = IC.random_cu_map(W, H, 31, 1, False, intra_share=0.1, blank_share=0.0, bad_share=0.0, far=0.0)
    rc_cus_d = torch.from_numpy(rc_cus.view(np.uint8).copy()).to(dev)
    rc_ref = [ref] + [torch.randint(0, 256, (H // 2, W // 2), dtype=torch.uint8, device=dev, generator=g) for _ in range(2)]
    rc_dst = [torch.empty((H >> c, W >> c), dtype=torch.uint8, device=dev) for c in (0, 1, 1)]
    rc_tab = api.ref_picture_table([(rc_ref[0].data_ptr(), rc_ref[1].data_ptr(), rc_ref[2].data_ptr(), W, W // 2)], W, H)
    rc_prm = np.zeros(1, dtype=api.INTER_RECON_PARAMS)
    rc_prm["chroma"], rc_prm["n_refs"], rc_prm["ref_LX"] = 1, 1, rc_LX
    keep += [rc_cus_d, rc_ref, rc_dst, rc_tab, rc_prm]
    if not pictures:                                                    # with --pictures all of them are predicted by one call, below
        stages["tu"].append(("inter_recon_frame", 1, lambda s: L.kvz_hip_inter_recon_frame(
            rc_dst[0].data_ptr(), W, rc_dst[1].data_ptr(), rc_dst[2].data_ptr(), W // 2, W, H, rc_cus_d.data_ptr(), rc_tab.ctypes.data,
            rc_prm.ctypes.data, s)))
    # the intra CUs of a picture (a tenth of it; tr_depth and modes as tests/intra_recon_cases.py sets them), in coding order on a map
    # and planes of its own: an init launch and one launch per wavefront of LCUs, 63 kernel launches at 1080p for the one call
    import intra_recon_cases as XC
    ir_cus, _, ir_modes = XC.make_map(W, H, 33, intra_share=0.1, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
    ir_src_h, ir_rec_h = XC.make_planes(ir_cus, 34)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
    ir_src, ir_rec, ir_cus_d, ir_modes_d = [up(p) for p in ir_src_h], [up(p) for p in ir_rec_h], up(ir_cus), up(ir_modes)
    ir_shapes = api.coeff_shapes(W, H)
    ir_co = [torch.zeros(ir_shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)]
    ir_tab = api.ref_picture_table([(ir_src[0].data_ptr(), ir_src[1].data_ptr(), ir_src[2].data_ptr(), W, W // 2)], W, H)
    ir_prm = api.inter_residual_params(27, 0, 0, 1)
    keep += [ir_src, ir_rec, ir_cus_d, ir_modes_d, ir_co, ir_tab, ir_prm]
    grid = api.uniform_tile_grid(W, H, tiles[0], tiles[1]) if tiles else None      # 1080 and the 1088 coded rows are the same 17 LCU rows
    keep.append(grid)
    if lcu_qp:
        # a QP per LCU: the flags go to an array (cleared once), the QP map is written from it after the intra stage
        ir_qp = up(np.random.default_rng(35).integers(22, 43, api.lcu_count(W, H)).astype(np.int8))
        ir_cbf = torch.zeros(ir_cus.shape, dtype=torch.uint8, device=dev)
        ir_last = torch.empty(api.lcu_count(W, H), dtype=torch.int8, device=dev)
        ir_qprm = np.zeros(1, dtype=api.CU_QP_PARAMS)
        ir_qprm["start_qp"] = 27
        keep += [ir_qp, ir_cbf, ir_last, ir_qprm]
    if lossless:
        # nothing is quantised: the two lossless entries on the maps and planes of the lossy ones, and the chain ends there
        ll = _lib.Lossless(1, 1, (0, 0))
        rc_co = [torch.zeros(ir_shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)]
        rc_src = [cur] + [torch.randint(0, 256, (H // 2, W // 2), dtype=torch.uint8, device=dev, generator=g) for _ in range(2)]
        rc_src_tab = api.ref_picture_table([(rc_src[0].data_ptr(), rc_src[1].data_ptr(), rc_src[2].data_ptr(), W, W // 2)], W, H)
        keep += [ll, rc_co, rc_src, rc_src_tab]
        stages["tu"].append(("inter_residual_frame_lossless", 1, lambda s: L.kvz_hip_inter_residual_frame_lossless(
            rc_src_tab.ctypes.data, rc_dst[0].data_ptr(), W, rc_dst[1].data_ptr(), rc_dst[2].data_ptr(), W // 2, rc_cus_d.data_ptr(),
            rc_co[0].data_ptr(), rc_co[1].data_ptr(), rc_co[2].data_ptr(), None, None, C.byref(ll), s)))
        stages["tu"].append(("intra_recon_frame_lossless", 1, lambda s: L.kvz_hip_intra_recon_frame_lossless(
            ir_tab.ctypes.data, ir_rec[0].data_ptr(), W, ir_rec[1].data_ptr(), ir_rec[2].data_ptr(), W // 2, ir_cus_d.data_ptr(), ir_modes_d.data_ptr(),
            ir_co[0].data_ptr(), ir_co[1].data_ptr(), ir_co[2].data_ptr(), None, None, grid.ctypes.data if tiles else None, C.byref(ll), s)))
        # the last stage of a picture: the SEI checksum and the squared error of the finished reconstruction
        ll_lcu = torch.empty(api.lcu_count(W, H) * 6, dtype=torch.int32, device=dev)
        ll_hash = torch.empty(5, dtype=torch.int64, device=dev)
        keep += [ll_lcu, ll_hash]
        stages["tu"].append(("picture_hash_frame", api.lcu_count(W, H), lambda s: L.kvz_hip_picture_hash_frame(
            ir_tab.ctypes.data, ir_rec[0].data_ptr(), W, ir_rec[1].data_ptr(), ir_rec[2].data_ptr(), W // 2, W, H, 1, ll_lcu.data_ptr(),
            ll_hash.data_ptr(), s)))
        del stages["sao"]                                            # no deblocking, no SAO (encoder.c:623-628)
        return stages, keep
    if pictures:
        # N independent pictures in flight: ONE kvz_hip_inter_recon_frames predicts all of them -- the pool is their distinct references,
        # here the one picture they share -- then ONE kvz_hip_inter_residual_frames and ONE kvz_hip_intra_recon_frames take all of them.  Picture 0 is the frame's own;
        # the others have planes, coefficients and intra maps of their own (the inter map and the references are shared inputs).
        # With --tiles, --scaling-list or --transform-skip the two calls are kvz_hip_inter_residual_frames_ts / kvz_hip_intra_recon_frames_ts:
        # every picture carries the grid, the tables (one set, shared) and a bit cost with an array of choices of its own per stage
        options = bool(tiles or lists == "default" or trskip)
        Record = _lib.ChainPictureTs if options else _lib.ChainPicture
        sl = None
        if lists == "default":
            z = np.load(os.path.join(ROOT, "tests", "golden", "scaling_list.npz"), allow_pickle=False)
            sl_q, sl_d = up(z["default_quant"]), up(z["default_dequant"])
            sl = _lib.ScalingTables(sl_q.data_ptr(), sl_d.data_ptr())
            keep += [sl_q, sl_d, sl]
        ts = _lib.TrSkip(18, 0, None) if trskip else None                # (int)(lambda + 0.5) at QP 27
        grid_p = C.cast(grid.ctypes.data, C.POINTER(_lib.TileGrid)) if tiles else None
        qp_recs = (_lib.FilterPicture * pictures)()                      # --lcu-qp: the QP map of all pictures in one kvz_hip_cu_qp_frames
        keep += [ts, grid_p, qp_recs]
        rc_src = [cur] + [torch.randint(0, 256, (H // 2, W // 2), dtype=torch.uint8, device=dev, generator=g) for _ in range(2)]
        inter, intra = (Record * pictures)(), (Record * pictures)()
        recon, rc_pool = (_lib.ReconPicture * pictures)(), (_lib.RefPicture * 1).from_buffer_copy(rc_tab.tobytes())
        keep += [rc_src, inter, intra, recon, rc_pool]
        for i in range(pictures):
            dst, co = rc_dst, [torch.zeros(ir_shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)]
            x_src, x_rec, x_cus, x_modes, x_co = ir_src, ir_rec, ir_cus_d, ir_modes_d, ir_co
            if i:
                dst = [torch.empty_like(p) for p in rc_dst]
                cus_h, _, modes_h = XC.make_map(W, H, 33 + 10 * i, intra_share=0.1, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
                src_h, rec_h = XC.make_planes(cus_h, 34 + 10 * i)
                x_src, x_rec, x_cus, x_modes = [up(p) for p in src_h], [up(p) for p in rec_h], up(cus_h), up(modes_h)
                x_co = [torch.zeros(ir_shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)]
            cus_copy = rc_cus_d.clone()                                  # cbf_y is written back: a map per picture
            p = recon[i]
            p.pred_y, p.pred_u, p.pred_v, p.stride_y, p.stride_c = dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), W, W // 2
            p.width, p.height, p.cus = W, H, rc_cus_d.data_ptr()
            p.refs[0], p.params = 0, _lib.InterReconParams.from_buffer_copy(rc_prm.tobytes())
            keep += [dst, co, x_src, x_rec, x_cus, x_modes, x_co, cus_copy]
            for full, src, rec, cus_d, modes_d, c in ((inter[i], rc_src, dst, cus_copy, None, co), (intra[i], x_src, x_rec, x_cus, x_modes, x_co)):
                r = full.pic if options else full
                r.src = _lib.RefPicture(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), W, W // 2, W, H)
                r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c = rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), W, W // 2
                r.cus, r.intra_modes = cus_d.data_ptr(), modes_d.data_ptr() if modes_d is not None else None
                r.coeff_y, r.coeff_u, r.coeff_v = c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr()
                r.params = _lib.InterResidualParams(27, 0, 0, 1 if sl is not None else 0, 1, 0)
                if lcu_qp:
                    r.lcu_qp = ir_qp.data_ptr()
                if options:
                    full.grid = grid_p
                    if sl is not None:
                        full.tables = sl
                    if trskip:
                        skip = torch.zeros(ir_cus.shape, dtype=torch.uint8, device=dev)
                        keep.append(skip)
                        full.ts, full.tr_skip_out = C.pointer(ts), skip.data_ptr()
            if lcu_qp:
                # the flags of the intra stage go to an array per picture (cleared once); the QP array is a shared input
                cbf_i, last_i = (ir_cbf, ir_last) if i == 0 else (torch.zeros_like(ir_cbf), torch.empty_like(ir_last))
                keep += [cbf_i, last_i]
                (intra[i].pic if options else intra[i]).cbf_out = cbf_i.data_ptr()
                q = qp_recs[i]
                q.width, q.height, q.chroma, q.deblock.chroma = W, H, 1, 1
                q.cus, q.cbf, q.lcu_qp, q.lcu_last_qp = x_cus.data_ptr(), cbf_i.data_ptr(), ir_qp.data_ptr(), last_i.data_ptr()
                q.grid, q.cu_qp = grid_p, _lib.CuQpTilesParams(27, 0)
        stages["tu"].append(("inter_recon_frames", pictures, lambda s: L.kvz_hip_inter_recon_frames(recon, pictures, rc_pool, 1, s)))
        if options:
            stages["tu"].append(("inter_residual_frames_ts", pictures, lambda s: L.kvz_hip_inter_residual_frames_ts(inter, pictures, s)))
            stages["tu"].append(("intra_recon_frames_ts", pictures, lambda s: L.kvz_hip_intra_recon_frames_ts(intra, pictures, s)))
        else:
            stages["tu"].append(("inter_residual_frames", pictures, lambda s: L.kvz_hip_inter_residual_frames(inter, pictures, s)))
            stages["tu"].append(("intra_recon_frames", pictures, lambda s: L.kvz_hip_intra_recon_frames(intra, pictures, s)))
        if lcu_qp:
            stages["tu"].append(("cu_qp_frames", pictures, lambda s: L.kvz_hip_cu_qp_frames(qp_recs, pictures, s)))
    elif lists or trskip:
        # the packed tables on the device; `none`: no tables, and params->scaling_list stays 0
        sl = None
        if lists == "default":
            z = np.load(os.path.join(ROOT, "tests", "golden", "scaling_list.npz"), allow_pickle=False)
            sl_q, sl_d = up(z["default_quant"]), up(z["default_dequant"])
            sl = _lib.ScalingTables(sl_q.data_ptr(), sl_d.data_ptr())
            ir_prm = api.inter_residual_params(27, 0, 0, 1, scaling_list=1)
            keep += [sl_q, sl_d, sl, ir_prm]
        sl_ref = C.byref(sl) if sl is not None else None
        # residual coding of the inter CUs, on the planes the motion compensation has just written (tr_depth 0 in this map: the
        # TUs are as large as their CUs, 32 at the most)
        rc_co = [torch.zeros(ir_shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)]
        rc_src = [cur] + [torch.randint(0, 256, (H // 2, W // 2), dtype=torch.uint8, device=dev, generator=g) for _ in range(2)]
        rc_src_tab = api.ref_picture_table([(rc_src[0].data_ptr(), rc_src[1].data_ptr(), rc_src[2].data_ptr(), W, W // 2)], W, H)
        keep += [rc_co, rc_src, rc_src_tab]
        if trskip:
            # one bit cost, (int)(lambda + 0.5) at QP 27; the choices of the two stages go to an array each (cleared once)
            ts = _lib.TrSkip(18, 0, None)
            rc_skip, ir_skip = (torch.zeros(ir_cus.shape, dtype=torch.uint8, device=dev) for _ in range(2))
            keep += [ts, rc_skip, ir_skip]
            if cabac_cost:
                # the reference's default pricing inside the decision: a context set per LCU, fast_limit 0 (cfg.c:82), so every
                # trial of every 4x4 luma TU is priced with the counting coder
                n_lcu = api.lcu_count(W, H)
                host = np.random.default_rng(36)
                cc_sets = np.zeros(n_lcu, dtype=api.COEFF_CTX)
                cc_sets["range"] = host.integers(256, 511, n_lcu)
                cc_sets["ctx"][:, :138] = host.integers(0, 126, (n_lcu, 138))
                cc_sets_d, cc_idx_d = up(cc_sets.view(np.uint8).reshape(-1)), up(np.arange(n_lcu, dtype=np.uint16))
                pricing = _lib.CoeffPricing(cc_sets_d.data_ptr(), n_lcu, 0, cc_idx_d.data_ptr())
                keep += [cc_sets_d, cc_idx_d, pricing]
                stages["tu"].append(("inter_residual_frame_ts_cabac", 1, lambda s: L.kvz_hip_inter_residual_frame_ts_cabac(
                    rc_src_tab.ctypes.data, rc_dst[0].data_ptr(), W, rc_dst[1].data_ptr(), rc_dst[2].data_ptr(), W // 2, rc_cus_d.data_ptr(),
                    rc_co[0].data_ptr(), rc_co[1].data_ptr(), rc_co[2].data_ptr(), None, None, ir_qp.data_ptr() if lcu_qp else None, sl_ref,
                    C.byref(ts), rc_skip.data_ptr(), C.byref(pricing), ir_prm.ctypes.data, s)))
                stages["tu"].append(("intra_recon_frame_ts_cabac", 1, lambda s: L.kvz_hip_intra_recon_frame_ts_cabac(
                    ir_tab.ctypes.data, ir_rec[0].data_ptr(), W, ir_rec[1].data_ptr(), ir_rec[2].data_ptr(), W // 2, ir_cus_d.data_ptr(), ir_modes_d.data_ptr(),
                    ir_co[0].data_ptr(), ir_co[1].data_ptr(), ir_co[2].data_ptr(), ir_cbf.data_ptr() if lcu_qp else None, None,
                    ir_qp.data_ptr() if lcu_qp else None, grid.ctypes.data if tiles else None, sl_ref, C.byref(ts), ir_skip.data_ptr(),
                    C.byref(pricing), ir_prm.ctypes.data, s)))
        if trskip and not cabac_cost:
            stages["tu"].append(("inter_residual_frame_ts", 1, lambda s: L.kvz_hip_inter_residual_frame_ts(
                rc_src_tab.ctypes.data, rc_dst[0].data_ptr(), W, rc_dst[1].data_ptr(), rc_dst[2].data_ptr(), W // 2, rc_cus_d.data_ptr(),
                rc_co[0].data_ptr(), rc_co[1].data_ptr(), rc_co[2].data_ptr(), None, None, ir_qp.data_ptr() if lcu_qp else None, sl_ref,
                C.byref(ts), rc_skip.data_ptr(), ir_prm.ctypes.data, s)))
            stages["tu"].append(("intra_recon_frame_ts", 1, lambda s: L.kvz_hip_intra_recon_frame_ts(
                ir_tab.ctypes.data, ir_rec[0].data_ptr(), W, ir_rec[1].data_ptr(), ir_rec[2].data_ptr(), W // 2, ir_cus_d.data_ptr(), ir_modes_d.data_ptr(),
                ir_co[0].data_ptr(), ir_co[1].data_ptr(), ir_co[2].data_ptr(), ir_cbf.data_ptr() if lcu_qp else None, None,
                ir_qp.data_ptr() if lcu_qp else None, grid.ctypes.data if tiles else None, sl_ref, C.byref(ts), ir_skip.data_ptr(),
                ir_prm.ctypes.data, s)))
        elif not trskip:
            stages["tu"].append(("inter_residual_frame_sl", 1, lambda s: L.kvz_hip_inter_residual_frame_sl(
                rc_src_tab.ctypes.data, rc_dst[0].data_ptr(), W, rc_dst[1].data_ptr(), rc_dst[2].data_ptr(), W // 2, rc_cus_d.data_ptr(),
                rc_co[0].data_ptr(), rc_co[1].data_ptr(), rc_co[2].data_ptr(), None, None, ir_qp.data_ptr() if lcu_qp else None, sl_ref,
                ir_prm.ctypes.data, s)))
            stages["tu"].append(("intra_recon_frame_sl", 1, lambda s: L.kvz_hip_intra_recon_frame_sl(
                ir_tab.ctypes.data, ir_rec[0].data_ptr(), W, ir_rec[1].data_ptr(), ir_rec[2].data_ptr(), W // 2, ir_cus_d.data_ptr(), ir_modes_d.data_ptr(),
                ir_co[0].data_ptr(), ir_co[1].data_ptr(), ir_co[2].data_ptr(), ir_cbf.data_ptr() if lcu_qp else None, None,
                ir_qp.data_ptr() if lcu_qp else None, grid.ctypes.data if tiles else None, sl_ref, ir_prm.ctypes.data, s)))
        if lcu_qp and tiles:
            ir_tprm = np.zeros(1, dtype=api.CU_QP_TILES_PARAMS)
            ir_tprm["start_qp"] = 27
            keep.append(ir_tprm)
            stages["tu"].append(("cu_qp_frame_tiles", 1, lambda s: L.kvz_hip_cu_qp_frame_tiles(
                ir_cus_d.data_ptr(), ir_cbf.data_ptr(), W, H, ir_qp.data_ptr(), ir_last.data_ptr(), grid.ctypes.data, ir_tprm.ctypes.data, s)))
        elif lcu_qp:
            stages["tu"].append(("cu_qp_frame", 1, lambda s: L.kvz_hip_cu_qp_frame(
                ir_cus_d.data_ptr(), ir_cbf.data_ptr(), W, H, ir_qp.data_ptr(), ir_last.data_ptr(), ir_qprm.ctypes.data, s)))
    elif tiles:
        stages["tu"].append(("intra_recon_frame_tiles", 1, lambda s: L.kvz_hip_intra_recon_frame_tiles(
            ir_tab.ctypes.data, ir_rec[0].data_ptr(), W, ir_rec[1].data_ptr(), ir_rec[2].data_ptr(), W // 2, ir_cus_d.data_ptr(), ir_modes_d.data_ptr(),
            ir_co[0].data_ptr(), ir_co[1].data_ptr(), ir_co[2].data_ptr(), ir_cbf.data_ptr() if lcu_qp else None, None,
            ir_qp.data_ptr() if lcu_qp else None, grid.ctypes.data, ir_prm.ctypes.data, s)))
        if lcu_qp:
            ir_tprm = np.zeros(1, dtype=api.CU_QP_TILES_PARAMS)
            ir_tprm["start_qp"] = 27
            keep.append(ir_tprm)
            stages["tu"].append(("cu_qp_frame_tiles", 1, lambda s: L.kvz_hip_cu_qp_frame_tiles(
                ir_cus_d.data_ptr(), ir_cbf.data_ptr(), W, H, ir_qp.data_ptr(), ir_last.data_ptr(), grid.ctypes.data, ir_tprm.ctypes.data, s)))
    elif lcu_qp:
        stages["tu"].append(("intra_recon_frame_qp", 1, lambda s: L.kvz_hip_intra_recon_frame_qp(
            ir_tab.ctypes.data, ir_rec[0].data_ptr(), W, ir_rec[1].data_ptr(), ir_rec[2].data_ptr(), W // 2, ir_cus_d.data_ptr(), ir_modes_d.data_ptr(),
            ir_co[0].data_ptr(), ir_co[1].data_ptr(), ir_co[2].data_ptr(), ir_cbf.data_ptr(), None, ir_qp.data_ptr(), ir_prm.ctypes.data, s)))
        stages["tu"].append(("cu_qp_frame", 1, lambda s: L.kvz_hip_cu_qp_frame(
            ir_cus_d.data_ptr(), ir_cbf.data_ptr(), W, H, ir_qp.data_ptr(), ir_last.data_ptr(), ir_qprm.ctypes.data, s)))
    else:
        stages["tu"].append(("intra_recon_frame", 1, lambda s: L.kvz_hip_intra_recon_frame(
            ir_tab.ctypes.data, ir_rec[0].data_ptr(), W, ir_rec[1].data_ptr(), ir_rec[2].data_ptr(), W // 2, ir_cus_d.data_ptr(), ir_modes_d.data_ptr(),
            ir_co[0].data_ptr(), ir_co[1].data_ptr(), ir_co[2].data_ptr(), None, None, ir_prm.ctypes.data, s)))

    qp = QuantParams(); qp.qp = 27
    keep.append(qp)
    for n in (4, 8, 16, 32):
        cnt = (W // n) * (H // n)
        rec = torch.empty(cnt * n * n, dtype=torch.uint8, device=dev)
        coef = torch.empty(cnt * n * n, dtype=torch.int16, device=dev)
        has = torch.empty(cnt, dtype=torch.int32, device=dev)
        ssd = torch.empty(cnt, dtype=torch.int32, device=dev)
        cas = torch.empty(cnt, dtype=torch.int32, device=dev)
        keep += [rec, coef, has, ssd, cas]
        stages["tu"].append(("quantize_residual_cost_%dx%d" % (n, n), cnt,
                             lambda s, n=n, cnt=cnt, rec=rec, coef=coef, has=has, ssd=ssd, cas=cas: L.kvz_hip_quantize_residual_cost_batch(
                                 C.byref(qp), 0, n, 0, 0, 0, flat_cur.data_ptr(), flat_pred.data_ptr(), rec.data_ptr(), coef.data_ptr(),
                                 has.data_ptr(), ssd.data_ptr(), cas.data_ptr(), cnt, s)))

    # SAO: every luma LCU (64x64) and both chroma planes (32x32 per LCU) of the frame
    for label, n, cnt in (("luma", 64, (W // 64) * (H // 64)), ("chroma", 32, 2 * (W // 64) * (H // 64))):
        edge = torch.empty(cnt * 40, dtype=torch.int32, device=dev)
        band = torch.empty(cnt * 64, dtype=torch.int32, device=dev)
        keep += [edge, band]
        stages["sao"].append(("sao_edge_stats_%s" % label, cnt,
                              lambda s, n=n, cnt=cnt, edge=edge: L.kvz_hip_sao_edge_stats_batch(
                                  flat_cur.data_ptr(), flat_pred.data_ptr(), n, n, cnt, edge.data_ptr(), s)))
        stages["sao"].append(("sao_band_stats_%s" % label, cnt,
                              lambda s, n=n, cnt=cnt, band=band: L.kvz_hip_sao_band_stats_batch(
                                  flat_cur.data_ptr(), flat_pred.data_ptr(), n, n, cnt, band.data_ptr(), s)))
    # deblocking of the reconstructed frame (1088 coded rows), both passes
    from patterns import deblock_case, deblock_params
    DH = 1088
    ty, tu, tv, tcus = deblock_case(256, 128, 11, qp=36)
    reps = (DH // 128 + 1, W // 256 + 1)
    dby = torch.from_numpy(np.tile(ty, reps)[:DH, :W].copy()).to(dev)
    dbu = torch.from_numpy(np.tile(tu, reps)[:DH // 2, :W // 2].copy()).to(dev)
    dbv = torch.from_numpy(np.tile(tv, reps)[:DH // 2, :W // 2].copy()).to(dev)
    dbc = torch.from_numpy(np.tile(tcus, reps)[:DH // 4, :W // 4].copy().view(np.uint8)).to(dev)
    dbp = deblock_params(qp=36, per_cu_qp=1 if lcu_qp else 0)          # per_cu_qp: the filter reads the qp field of the records
    keep += [dby, dbu, dbv, dbc, dbp]
    if pictures:
        pass                                                             # deblocking of all pictures in one call: below, with the SAO stages
    elif tiles:
        stages["sao"].insert(0, ("deblock_frame_tiles", 1, lambda s: L.kvz_hip_deblock_frame_tiles(
            dby.data_ptr(), W, dbu.data_ptr(), dbv.data_ptr(), W // 2, W, DH, dbc.data_ptr(), grid.ctypes.data, dbp.ctypes.data, s)))
    else:
        stages["sao"].insert(0, ("deblock_frame", 1, lambda s: L.kvz_hip_deblock_frame(
            dby.data_ptr(), W, dbu.data_ptr(), dbv.data_ptr(), W // 2, W, DH, dbc.data_ptr(), dbp.ctypes.data, s)))
    # SAO of the deblocked picture, the two whole-picture calls: statistics + candidates of every LCU and plane, then the
    # reconstruction into the next frame's reference (records: every LCU an edge or band record, as after a decision)
    from patterns import sao_records
    n_lcu = api.lcu_count(W, DH)
    so_src = [(p.to(torch.int16) + torch.randint(-6, 7, p.shape, dtype=torch.int16, device=dev, generator=g)).clamp_(0, 255).to(torch.uint8)
              for p in (dby, dbu, dbv)]
    so_tab = api.ref_picture_table([(so_src[0].data_ptr(), so_src[1].data_ptr(), so_src[2].data_ptr(), W, W // 2)], W, DH)
    so_stats = torch.empty(3 * n_lcu * 104, dtype=torch.int32, device=dev)
    so_cands = torch.empty(3 * n_lcu * 30, dtype=torch.int32, device=dev)
    so_luma = torch.from_numpy(sao_records(n_lcu, 3)).to(dev)
    so_chroma = torch.from_numpy(sao_records(n_lcu, 4)).to(dev)
    so_dst = [torch.empty_like(p) for p in (dby, dbu, dbv)]
    keep += [so_src, so_tab, so_stats, so_cands, so_luma, so_chroma, so_dst]
    if pictures:
        # the stages behind the residual stages, all pictures in one call each: deblocking in place, the statistics and the SAO
        # reconstruction.  Picture 0 is the frame's own; the others have planes, statistics and destinations of their own (the map,
        # the source and the SAO records are shared inputs)
        f_recs = (_lib.FilterPicture * pictures)()
        keep.append(f_recs)
        for i in range(pictures):
            rec = [dby, dbu, dbv] if i == 0 else [p.clone() for p in (dby, dbu, dbv)]
            dst = so_dst if i == 0 else [torch.empty_like(p) for p in so_dst]
            st, cd = (so_stats, so_cands) if i == 0 else (torch.empty_like(so_stats), torch.empty_like(so_cands))
            keep += [rec, dst, st, cd]
            r = f_recs[i]
            r.width, r.height, r.chroma = W, DH, 1
            r.src = _lib.RefPicture(so_src[0].data_ptr(), so_src[1].data_ptr(), so_src[2].data_ptr(), W, W // 2, W, DH)
            r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c = rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), W, W // 2
            r.dst_y, r.dst_u, r.dst_v, r.dst_stride_y, r.dst_stride_c = dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), W, W // 2
            r.cus, r.stats, r.cands = dbc.data_ptr(), st.data_ptr(), cd.data_ptr()
            r.sao_luma, r.sao_chroma = so_luma.data_ptr(), so_chroma.data_ptr()
            r.grid = C.cast(grid.ctypes.data, C.POINTER(_lib.TileGrid)) if tiles else None
            r.deblock = _lib.DeblockParams.from_buffer_copy(dbp.tobytes())
        stages["sao"].insert(0, ("deblock_frames", pictures, lambda s: L.kvz_hip_deblock_frames(f_recs, pictures, s)))
        stages["sao"].insert(1, ("sao_stats_frames", pictures * 3 * n_lcu, lambda s: L.kvz_hip_sao_stats_frames(f_recs, pictures, s)))
        stages["sao"].insert(2, ("sao_frames", pictures, lambda s: L.kvz_hip_sao_frames(f_recs, pictures, s)))
        # the last stage: the SEI checksum and the squared error of every finished picture, in one call
        h_recs = (_lib.HashPicture * pictures)()
        keep.append(h_recs)
        for i in range(pictures):
            lcu, tot = torch.empty(n_lcu * 6, dtype=torch.int32, device=dev), torch.empty(5, dtype=torch.int64, device=dev)
            keep += [lcu, tot]
            f, r = f_recs[i], h_recs[i]
            r.width, r.height, r.chroma, r.src = W, DH, 1, f.src
            r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c = f.dst_y, f.dst_u, f.dst_v, f.dst_stride_y, f.dst_stride_c
            r.lcu_out, r.out = lcu.data_ptr(), tot.data_ptr()
        stages["sao"].insert(3, ("picture_hash_frames", pictures * n_lcu, lambda s: L.kvz_hip_picture_hash_frames(h_recs, pictures, s)))
        return stages, keep
    stages["sao"].insert(1, ("sao_stats_frame", 3 * n_lcu, lambda s: L.kvz_hip_sao_stats_frame(
        so_tab.ctypes.data, dby.data_ptr(), W, dbu.data_ptr(), dbv.data_ptr(), W // 2, 1, so_stats.data_ptr(), so_cands.data_ptr(), s)))
    if tiles:
        stages["sao"].insert(2, ("sao_frame_tiles", 1, lambda s: L.kvz_hip_sao_frame_tiles(
            dby.data_ptr(), W, dbu.data_ptr(), dbv.data_ptr(), W // 2, so_dst[0].data_ptr(), W, so_dst[1].data_ptr(), so_dst[2].data_ptr(), W // 2,
            W, DH, so_luma.data_ptr(), so_chroma.data_ptr(), 1, grid.ctypes.data, s)))
    else:
        stages["sao"].insert(2, ("sao_frame", 1, lambda s: L.kvz_hip_sao_frame(
            dby.data_ptr(), W, dbu.data_ptr(), dbv.data_ptr(), W // 2, so_dst[0].data_ptr(), W, so_dst[1].data_ptr(), so_dst[2].data_ptr(), W // 2,
            W, DH, so_luma.data_ptr(), so_chroma.data_ptr(), 1, s)))
    # the last stage of a picture: the SEI checksum and the squared error of the finished reconstruction
    so_lcu = torch.empty(n_lcu * 6, dtype=torch.int32, device=dev)
    so_hash = torch.empty(5, dtype=torch.int64, device=dev)
    keep += [so_lcu, so_hash]
    stages["sao"].insert(3, ("picture_hash_frame", n_lcu, lambda s: L.kvz_hip_picture_hash_frame(
        so_tab.ctypes.data, so_dst[0].data_ptr(), W, so_dst[1].data_ptr(), so_dst[2].data_ptr(), W // 2, W, DH, 1, so_lcu.data_ptr(),
        so_hash.data_ptr(), s)))
    return stages, keep


def chk(rc, what):
    _lib.check(rc, what)


def enqueue_serial(stages, s):
    for st in stages.values():
        for name, _, fn in st:
            chk(fn(s), name)


def by_launch(stages):
    """finer branches: every motion-search launch on its own (they are latency bound and, at 480..8040 PUs, none of the
    larger sizes fills the chip), the other three stages as before"""
    out = {}
    for name, units, fn in stages["me"]:                 # a size's candidate derivation and its search stay on one branch, in order
        out.setdefault(name.rsplit("_", 1)[1], []).append((name, units, fn))
    out.update({k: v for k, v in stages.items() if k != "me"})
    return out


def enqueue_forked(L, stages, s, side, events):
    """stage k on side[k]; fork from s, join back into s"""
    fork = events[0]
    chk(L.kvz_hip_event_record(fork, s), "fork")
    for k, st in enumerate(stages.values()):
        chk(L.kvz_hip_stream_wait_event(side[k], fork), "fork wait")
        for name, _, fn in st:
            chk(fn(side[k]), name)
        chk(L.kvz_hip_event_record(events[1 + k], side[k]), "join record")
        chk(L.kvz_hip_stream_wait_event(s, events[1 + k]), "join wait")


def run(L, s, frames, per_frame):
    """wall-clock ms per frame, frames enqueued back to back, one sync at the end"""
    for _ in range(5):
        per_frame()
    chk(L.kvz_hip_stream_sync(s), "sync")
    t0 = time.perf_counter()
    for _ in range(frames):
        per_frame()
    t_enq = time.perf_counter() - t0
    chk(L.kvz_hip_stream_sync(s), "sync")
    return (time.perf_counter() - t0) * 1e3 / frames, t_enq * 1e3 / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--tune", default="", help="key=value[,key=value...] passed to kvz_hip_set_tuning")
    ap.add_argument("--lcu-qp", action="store_true", help="a QP per LCU: intra_recon_frame_qp, cu_qp_frame, deblocking with per_cu_qp = 1")
    ap.add_argument("--tiles", default="", metavar="CxR", help="C x R uniform tiles: the *_tiles entries of intra, QP map, deblocking and SAO")
    ap.add_argument("--scaling-list", nargs="?", const="default", default=None, choices=("default", "none"),
                    help="the *_sl entries of the inter residual coding and the intra reconstruction; `none`: with tables == NULL (the baseline)")
    ap.add_argument("--transform-skip", action="store_true",
                    help="the *_ts entries of the inter residual coding and the intra reconstruction, with one bit cost")
    ap.add_argument("--cabac-cost", action="store_true",
                    help="with --transform-skip: the *_ts_cabac entries, every trial priced with CABAC on its LCU's context set (fast_limit 0)")
    ap.add_argument("--lossless", action="store_true",
                    help="a frame coded with --lossless: prediction, then the two *_lossless entries; no QP map, deblocking or SAO, which "
                         "encoder.c:623-628 switches off with sign hiding and transform skip")
    ap.add_argument("--pictures", type=int, default=0, metavar="N",
                    help="N independent pictures (1..16): their prediction through kvz_hip_inter_recon_frames, their two residual stages through kvz_hip_inter_residual_frames / kvz_hip_intra_recon_frames, or "
                         "through the *_frames_ts entries with --tiles, --scaling-list or --transform-skip; the QP map (--lcu-qp), deblocking and SAO "
                         "through kvz_hip_cu_qp_frames, kvz_hip_deblock_frames, kvz_hip_sao_stats_frames and kvz_hip_sao_frames")
    args = ap.parse_args()
    if args.pictures and (args.lossless or not 1 <= args.pictures <= 16):
        ap.error("--pictures N: 1..16, and without --lossless (one launch per picture already), which stays with the single-picture entries; "
                 "--lcu-qp, --tiles, --scaling-list and --transform-skip combine with it")
    if args.lossless and (args.lcu_qp or args.scaling_list or args.transform_skip):
        ap.error("--lossless: nothing is quantised, so --lcu-qp, --scaling-list and --transform-skip do not combine with it")
    tiles = tuple(int(v) for v in args.tiles.lower().split("x")) if args.tiles else None
    assert tiles is None or len(tiles) == 2
    dev = torch.device("cuda", 0)
    L = _lib.init(0)
    for kv in filter(None, args.tune.split(",")):
        k, v = kv.split("=")
        chk(L.kvz_hip_set_tuning(k.encode(), int(v)), "set_tuning " + k)
    s = L.kvz_hip_stream_create()
    side = [L.kvz_hip_stream_create() for _ in range(7)]
    events = [L.kvz_hip_event_create() for _ in range(8)]
    if args.cabac_cost and (not args.transform_skip or args.pictures):
        ap.error("--cabac-cost belongs to --transform-skip, one picture at a time")
    stages, keep = build_stages(L, dev, args.lcu_qp, tiles, args.scaling_list, args.transform_skip, args.lossless, args.pictures, args.cabac_cost)
    torch.cuda.synchronize()
    n_launch = sum(len(v) for v in stages.values())

    # per-entry device time at frame-sized batches (HIP events around 20 back-to-back launches)
    print("%-34s %9s %10s" % ("entry (one 1080p frame)", "units", "us/launch"))
    total = 0.0
    for st in stages.values():
        for name, units, fn in st:
            e0, e1 = L.kvz_hip_event_create(), L.kvz_hip_event_create()
            for _ in range(3):
                chk(fn(s), name)
            L.kvz_hip_event_record(e0, s)
            for _ in range(20):
                chk(fn(s), name)
            L.kvz_hip_event_record(e1, s)
            ms = C.c_float()
            chk(L.kvz_hip_event_elapsed_ms(e0, e1, C.byref(ms)), "elapsed")
            L.kvz_hip_event_destroy(e0); L.kvz_hip_event_destroy(e1)
            total += ms.value / 20
            print("%-34s %9d %10.1f" % (name, units, ms.value / 20 * 1e3))
    waves = (W + 63) // 64 + 2 * ((H + 63) // 64 - 1)
    if tiles:
        from kvazaar_amd import api
        g = api.uniform_tile_grid(W, H, tiles[0], tiles[1])
        waves = int(max(np.diff(g["col_bd"][0, :tiles[0] + 1])) + 2 * (max(np.diff(g["row_bd"][0, :tiles[1] + 1])) - 1))
    print("%-34s %9s %10.1f   (%d calls; the intra reconstruction is %d kernel launch%s of its own)" % ("sum of the entries", "", total * 1e3, n_launch,
                                                                                                  1 if args.lossless else 1 + waves,
                                                                                                  "" if args.lossless else "es"))

    results = {}
    results["eager"] = run(L, s, args.frames, lambda: enqueue_serial(stages, s))
    results["eager4"] = run(L, s, args.frames, lambda: enqueue_forked(L, stages, s, side, events))

    graph = C.c_void_p()
    chk(L.kvz_hip_graph_begin(s), "graph_begin")
    enqueue_serial(stages, s)
    chk(L.kvz_hip_graph_end(s, C.byref(graph)), "graph_end")
    results["graph"] = run(L, s, args.frames, lambda: chk(L.kvz_hip_graph_launch(graph, s), "graph_launch"))
    L.kvz_hip_graph_destroy(graph)

    graph4 = C.c_void_p()
    chk(L.kvz_hip_graph_begin(s), "graph_begin")
    enqueue_forked(L, stages, s, side, events)
    chk(L.kvz_hip_graph_end(s, C.byref(graph4)), "graph_end")
    results["graph4"] = run(L, s, args.frames, lambda: chk(L.kvz_hip_graph_launch(graph4, s), "graph_launch"))
    L.kvz_hip_graph_destroy(graph4)

    fine = by_launch(stages)
    results["eager7"] = run(L, s, args.frames, lambda: enqueue_forked(L, fine, s, side, events))
    graph7 = C.c_void_p()
    chk(L.kvz_hip_graph_begin(s), "graph_begin")
    enqueue_forked(L, fine, s, side, events)
    chk(L.kvz_hip_graph_end(s, C.byref(graph7)), "graph_end")
    results["graph7"] = run(L, s, args.frames, lambda: chk(L.kvz_hip_graph_launch(graph7, s), "graph_launch"))
    L.kvz_hip_graph_destroy(graph7)

    print()
    print("%-8s %14s %18s %10s" % ("mode", "ms per frame", "host enqueue ms", "frames/s"))
    for k, (ms, enq) in results.items():
        print("%-8s %14.3f %18.3f %10.0f" % (k, ms, enq, 1e3 / ms))


if __name__ == "__main__":
    main()
