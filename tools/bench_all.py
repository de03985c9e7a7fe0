#!/usr/bin/env python3
"""Per-kernel throughput of every batched entry of the C ABI (HIP-event timed, inputs
resident in HBM, working sets larger than the 256 MiB Infinity Cache where the kernel
streams).  Development tool; bench.py is the contract benchmark.

  python tools/bench_all.py                       # table of all kernels
  python tools/bench_all.py --only dct --tune dct32_wgs_per_cu=3,4,5,6,8   # interleaved A/B in one process (--only a,b: several substrings)
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from kvazaar_amd import _lib, api  # noqa: E402
from kvazaar_amd._lib import QuantParams  # noqa: E402


def timed(L, stream, fn, iters=20, warm=3):
    e0, e1 = L.kvz_hip_event_create(), L.kvz_hip_event_create()
    for _ in range(warm):
        fn()
    L.kvz_hip_event_record(e0, stream)
    for _ in range(iters):
        fn()
    L.kvz_hip_event_record(e1, stream)
    ms = C.c_float()
    _lib.check(L.kvz_hip_event_elapsed_ms(e0, e1, C.byref(ms)), "elapsed")
    L.kvz_hip_event_destroy(e0); L.kvz_hip_event_destroy(e1)
    return ms.value / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--tune", default="", help="key=v1,v2,... (interleaved rounds)")
    ap.add_argument("--mb", type=int, default=512, help="bytes per operand array (MiB)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rdoq-cpu", action="store_true", help="no device: the compiled reference's kvz_rdoq on the inputs of the rdoq_batch rows, us per TU")
    args = ap.parse_args()
    if args.rdoq_cpu:
        return rdoq_cpu_rows()
    dev = torch.device("cuda", 0)
    L = _lib.init(0)
    st = L.kvz_hip_stream_create()
    nbytes = args.mb << 20
    g = torch.Generator(device=dev); g.manual_seed(1)
    a8 = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev, generator=g)
    b8 = (a8.to(torch.int16) + torch.randint(-8, 9, (nbytes,), dtype=torch.int16, device=dev, generator=g)).clamp_(0, 255).to(torch.uint8)
    r16 = torch.randint(-255, 256, (nbytes // 2,), dtype=torch.int16, device=dev, generator=g)
    o16 = torch.empty_like(r16)
    o8 = torch.empty_like(a8)
    o32 = torch.empty(nbytes // 16, dtype=torch.int32, device=dev)
    has = torch.empty(nbytes // 16, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    cases = []   # (name, blocks, algorithmic bytes per block, fn)
    for n in (4, 8, 16, 32, 64):
        cnt = nbytes // (n * n)
        cases.append(("sad_%dx%d" % (n, n), cnt, 2 * n * n + 4,
                      lambda n=n, cnt=cnt: L.kvz_hip_sad_nxn_batch(n, a8.data_ptr(), b8.data_ptr(), cnt, o32.data_ptr(), st)))
        cases.append(("satd_%dx%d" % (n, n), cnt, 2 * n * n + 4,
                      lambda n=n, cnt=cnt: L.kvz_hip_satd_nxn_batch(n, a8.data_ptr(), b8.data_ptr(), cnt, o32.data_ptr(), st)))
    for n in (4, 8, 16, 32):
        cnt = (nbytes // 2) // (n * n)
        for kind, kid in (("dct", 0), ("idct", 1)):
            cases.append(("%s_%dx%d" % (kind, n, n), cnt, 4 * n * n,
                          lambda n=n, cnt=cnt, kid=kid: L.kvz_hip_transform_batch(kid, n, r16.data_ptr(), o16.data_ptr(), cnt, st)))
    qp = QuantParams(); qp.qp = 27
    for n in (4, 8, 16, 32):
        cnt = (nbytes // 2) // (n * n)
        cases.append(("quant_%dx%d" % (n, n), cnt, 4 * n * n,
                      lambda n=n, cnt=cnt: L.kvz_hip_quant_batch(C.byref(qp), r16.data_ptr(), o16.data_ptr(), n, 0, 0, cnt, st)))
        cases.append(("dequant_%dx%d" % (n, n), cnt, 4 * n * n,
                      lambda n=n, cnt=cnt: L.kvz_hip_dequant_batch(C.byref(qp), r16.data_ptr(), o16.data_ptr(), n, 0, cnt, st)))
        cnt2 = (nbytes // 4) // (n * n)
        cases.append(("quantize_residual_%dx%d" % (n, n), cnt2, 5 * n * n,
                      lambda n=n, cnt2=cnt2: L.kvz_hip_quantize_residual_batch(C.byref(qp), 0, n, 0, 0, 0, a8.data_ptr(), b8.data_ptr(),
                                                                              o8.data_ptr(), o16.data_ptr(), has.data_ptr(), cnt2, st)))

    # batched ME: 1080p CTU grid x frames, the speed_tests.c +-6 grid (25 candidates) -> 85 PU costs each
    import numpy as np
    W, H, F = 1920, 1080, 16
    picf = torch.randint(0, 256, (F * H, W), dtype=torch.uint8, device=dev, generator=g)
    reff = torch.roll(picf, shifts=(1, 2), dims=(0, 1)).contiguous()
    ctu_list = np.array([(x, f * H + y, 0, 0) for f in range(F) for y in range(0, H - 63, 64) for x in range(0, W, 64)], dtype=np.int32)
    ctus_d = torch.from_numpy(ctu_list).to(dev)
    for label, offs in (("grid25", [(dx, dy) for dy in (-6, -3, 0, 3, 6) for dx in (-6, -3, 0, 3, 6)]),
                        ("full8", [(dx, dy) for dy in range(-8, 9) for dx in range(-8, 9)])):
        mv_d = torch.tensor(offs, dtype=torch.int16, device=dev)
        out_d = torch.empty((len(ctu_list), len(offs), 85), dtype=torch.int32, device=dev)
        n_sad8 = len(ctu_list) * len(offs) * 64
        # bytes per 8x8-candidate: the HBM traffic of this kernel divided by the 8x8 SADs it produces
        bpb = (len(ctu_list) * (4096 + (64 + 16) ** 2) + out_d.numel() * 4) / n_sad8
        cases.append(("ctu_sad_%s(8x8 cands)" % label, n_sad8, bpb,
                      lambda mv_d=mv_d, out_d=out_d, offs=offs: L.kvz_hip_ctu_sad_grid_batch(
                          picf.data_ptr(), W, W, F * H, reff.data_ptr(), W, W, F * H, ctus_d.data_ptr(), len(ctu_list),
                          mv_d.data_ptr(), len(offs), out_d.data_ptr(), st)))

    # frame-level kernels on one 1080p frame pair x F frames: every 8x8 / 16x16 / 64x64 block with a small MV
    rs = np.random.default_rng(3)
    for n in (8, 16, 64):
        prs = np.array([(x, f * H + y, min(max(x + int(dx), 0), W - n), f * H + min(max(y + int(dy), 0), H - n), n, n)
                        for f in range(4) for y in range(0, H - n + 1, n) for x in range(0, W - n + 1, n)
                        for (dx, dy) in [rs.integers(-6, 7, 2)]], dtype=np.int32)
        prs_d = torch.from_numpy(prs).to(dev)
        outp = torch.empty(len(prs), dtype=torch.int32, device=dev)
        cases.append(("reg_sad_frame_%dx%d" % (n, n), len(prs), 2 * n * n + 4 + 24,
                      lambda prs_d=prs_d, outp=outp, k=len(prs): L.kvz_hip_reg_sad_batch(picf.data_ptr(), W, reff.data_ptr(), W, prs_d.data_ptr(), k, outp.data_ptr(), st)))
        cases.append(("image_satd_frame_%dx%d" % (n, n), len(prs), 2 * n * n + 4 + 24,
                      lambda prs_d=prs_d, outp=outp, k=len(prs): L.kvz_hip_image_calc_satd_batch(picf.data_ptr(), W, reff.data_ptr(), W, W, F * H, prs_d.data_ptr(), k, outp.data_ptr(), st)))
    # ipol: quarter-pel luma samples and the fused fractional search, all blocks of 4 frames
    for n in (8, 16, 32, 64):
        blks = np.array([(x, f * H + y, int(fx), int(fy), n, n) for f in range(4) for y in range(0, H - n + 1, n) for x in range(0, W - n + 1, n)
                         for (fx, fy) in [rs.integers(0, 4, 2)]], dtype=np.int32)
        blks_d = torch.from_numpy(blks).to(dev)
        offs_d = torch.arange(len(blks), dtype=torch.int64, device=dev) * (n * n)
        dst = torch.empty(len(blks) * n * n, dtype=torch.uint8, device=dev)
        cases.append(("sample_luma_%dx%d" % (n, n), len(blks), (n + 7) * (n + 7) + n * n,
                      lambda blks_d=blks_d, offs_d=offs_d, dst=dst, k=len(blks): L.kvz_hip_sample_luma_batch(
                          reff.data_ptr(), W, W, F * H, blks_d.data_ptr(), offs_d.data_ptr(), k, 0, dst.data_ptr(), st)))
        prs = np.array([(x, f * H + y, x + 1, f * H + y + 1, n, n) for f in range(4) for y in range(0, H - n + 1, n) for x in range(0, W - n + 1, n)], dtype=np.int32)
        prs_d = torch.from_numpy(prs).to(dev)
        co = torch.empty(len(prs) * 17, dtype=torch.int32, device=dev)
        be = torch.empty(len(prs) * 2, dtype=torch.int32, device=dev)
        cases.append(("search_frac_%dx%d" % (n, n), len(prs), (n + 8) * (n + 8) + n * n + 76,
                      lambda prs_d=prs_d, co=co, be=be, k=len(prs): L.kvz_hip_search_frac_batch(
                          picf.data_ptr(), W, reff.data_ptr(), W, W, F * H, prs_d.data_ptr(), k, co.data_ptr(), be.data_ptr(), st)))

    # whole-PU motion search (hexagon + fractional, with MV costs): every n x n PU of 4 frames
    me_prm = np.zeros(24, dtype=np.int32); me_prm[:8] = (20, 1, -1, 4, 0, 0, 1, 1)
    for n in (8, 16, 32, 64):
        rows = [(x, f * H + y) for f in range(4) for y in range(0, H - n + 1, n) for x in range(0, W - n + 1, n)]
        pus = np.zeros((len(rows), 16), dtype=np.int32)
        pus[:, 0] = [r[0] for r in rows]; pus[:, 1] = [r[1] for r in rows]; pus[:, 2] = n; pus[:, 3] = n
        pus_d = torch.from_numpy(pus).to(dev)
        res_d = torch.empty((len(rows), 8), dtype=torch.int32, device=dev)
        cls_prm = me_prm.copy(); cls_prm[10] = 1 if n <= 16 else (2 if n <= 32 else 4)     # size_classes hint: one launch instead of three
        cases.append(("search_pu_%dx%d" % (n, n), len(rows), 2 * n * n + 96,
                      lambda pus_d=pus_d, res_d=res_d, k=len(rows), cls_prm=cls_prm: L.kvz_hip_search_pu_batch(
                          picf.data_ptr(), W, W, F * H, reff.data_ptr(), W, W, F * H, pus_d.data_ptr(), k,
                          cls_prm.ctypes.data, res_d.data_ptr(), st)))
        if n == 16:
            for alg_name, alg in (("dia", 1), ("tz", 2)):                      # --me dia / --me tz
                alg_prm = cls_prm.copy(); alg_prm[8] = alg
                cases.append(("search_pu_16x16_%s" % alg_name, len(rows), 2 * n * n + 96,
                              lambda pus_d=pus_d, res_d=res_d, k=len(rows), alg_prm=alg_prm: L.kvz_hip_search_pu_batch(
                                  picf.data_ptr(), W, W, F * H, reff.data_ptr(), W, W, F * H, pus_d.data_ptr(), k,
                                  alg_prm.ctypes.data, res_d.data_ptr(), st)))
            full_prm = me_prm.copy(); full_prm[8] = 3; full_prm[9] = 16        # --me full16: 1089 positions per PU
            kk = len(rows) // 8
            cases.append(("search_pu_16x16_full16", kk, 2 * n * n + 96,
                          lambda pus_d=pus_d, res_d=res_d, kk=kk, full_prm=full_prm: L.kvz_hip_search_pu_batch(
                              picf.data_ptr(), W, W, F * H, reff.data_ptr(), W, W, F * H, pus_d.data_ptr(), kk,
                              full_prm.ctypes.data, res_d.data_ptr(), st)))

    # SAO statistics: every 64x64 luma LCU of 16 frames (blocks contiguous, as sao.c blits them)
    sao_cnt = min(nbytes // 4096, 510 * 16)
    sao_stats = torch.empty(sao_cnt * 64, dtype=torch.int32, device=dev)
    cases.append(("sao_edge_stats_64x64(4 classes)", sao_cnt, 2 * 4096 + 160,
                  lambda: L.kvz_hip_sao_edge_stats_batch(a8.data_ptr(), b8.data_ptr(), 64, 64, sao_cnt, sao_stats.data_ptr(), st)))
    cases.append(("sao_band_stats_64x64", sao_cnt, 2 * 4096 + 256,
                  lambda: L.kvz_hip_sao_band_stats_batch(a8.data_ptr(), b8.data_ptr(), 64, 64, sao_cnt, sao_stats.data_ptr(), st)))

    # deblocking of a whole 1080p (1920x1080 -> 1080 is not a multiple of 8 in the reference either: 1088 coded rows) frame
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from patterns import deblock_case, deblock_params
    DW, DH = 1920, 1088
    ty, tu, tv, tcus = deblock_case(256, 128, 11, qp=36)
    reps = (DH // 128 + 1, DW // 256 + 1)
    dby = torch.from_numpy(np.tile(ty, reps)[:DH, :DW].copy()).to(dev)
    dbu = torch.from_numpy(np.tile(tu, reps)[:DH // 2, :DW // 2].copy()).to(dev)
    dbv = torch.from_numpy(np.tile(tv, reps)[:DH // 2, :DW // 2].copy()).to(dev)
    dbc = torch.from_numpy(np.tile(tcus, reps)[:DH // 4, :DW // 4].copy().view(np.uint8)).to(dev)
    dbp = deblock_params(qp=36)
    # bytes per frame: luma + chroma read and written once per pass at most + the SCU map
    cases.append(("deblock_frame_1080p(frames)", 1, 2 * 2 * (DW * DH * 3 // 2) + DW * DH // 16 * 20 * 2,
                  lambda: L.kvz_hip_deblock_frame(dby.data_ptr(), DW, dbu.data_ptr(), dbv.data_ptr(), DW // 2, DW, DH, dbc.data_ptr(),
                                                  dbp.ctypes.data, st)))

    # intra rough search: all 35 modes per PU; bytes per PU = refs 130 + orig N^2 + 35 costs
    for lg in (2, 3, 4, 5):
        n = 1 << lg
        cnt = min((nbytes // 4) // (n * n), 1 << 20)
        refs_d = torch.randint(0, 256, (cnt * 130,), dtype=torch.uint8, device=dev, generator=g)
        costs_d = torch.empty(cnt * 35, dtype=torch.int32, device=dev)
        cases.append(("intra_rough_%dx%d(PUs)" % (n, n), cnt, 130 + n * n + 140,
                      lambda lg=lg, cnt=cnt, refs_d=refs_d, costs_d=costs_d: L.kvz_hip_intra_rough_batch(
                          lg, 3, refs_d.data_ptr(), a8.data_ptr(), cnt, costs_d.data_ptr(), None, st)))

    # candidate derivation + intra reference building of one 1080p frame's 8x8 PUs (the glue kernels between dependency fronts)
    from patterns import ME_PU, inter_cu_map, inter_params
    ip = inter_params(1920, 1080, poc=8, ref_pocs=(7,), l0=(0,), col_ref_pocs=(6,), col_l0=(0,))
    cu_now, _ = inter_cu_map(1920, 1080, 1)
    cu_col, _ = inter_cu_map(1920, 1080, 2)
    grid = np.zeros(32400, dtype=ME_PU)
    grid["x"], grid["y"] = (np.arange(32400) % 240) * 8, (np.arange(32400) // 240) * 8
    grid["width"] = grid["height"] = 8
    cu_now_d = torch.from_numpy(cu_now.view(np.uint8).copy()).to(dev)
    cu_col_d = torch.from_numpy(cu_col.view(np.uint8).copy()).to(dev)
    grid_d = torch.from_numpy(grid.view(np.uint8).copy()).to(dev)
    merge_d = torch.empty(32400 * 60, dtype=torch.uint8, device=dev)
    ip_host = np.ascontiguousarray(ip)
    cases.append(("inter_candidates_8x8(PUs)", 32400, 64 + 60 + 7 * 20,
                  lambda: L.kvz_hip_inter_candidates_batch(cu_now_d.data_ptr(), cu_col_d.data_ptr(), cu_col_d.data_ptr(), ip_host.ctypes.data,
                                                           grid_d.data_ptr(), 32400, merge_d.data_ptr(), st)))
    pos = np.stack([grid["x"], grid["y"]], axis=1).astype(np.int32)
    pos_d = torch.from_numpy(pos.copy()).to(dev)
    rec_d = torch.randint(0, 256, (1080 * 1920,), dtype=torch.uint8, device=dev, generator=g)
    refs8_d = torch.empty(32400 * 130, dtype=torch.uint8, device=dev)
    cases.append(("intra_build_reference_8x8(PUs)", 32400, 130 + 33,
                  lambda: L.kvz_hip_intra_build_reference_batch(3, 0, rec_d.data_ptr(), 1920, 1920, 1080, pos_d.data_ptr(), 32400, refs8_d.data_ptr(), st)))

    tune_key, tune_vals = "", [None]
    if args.tune:
        tune_key, vals = args.tune.split("=")
        tune_vals = [int(v) for v in vals.split(",")]
    torch.cuda.synchronize()         # the operands above were written on torch's stream; the library's stream does not wait for it
    print("%-26s %10s %12s %10s %8s" % ("kernel", "tune", "Mblocks/s", "GB/s", "ms"))
    for name, blocks, bpb, fn in cases:
        if args.only and not any(o in name for o in args.only.split(",")):
            continue
        best = {}
        for _ in range(args.rounds):
            for v in tune_vals:
                with api.tuned(**({tune_key: v} if tune_key else {})):
                    ms = timed(L, st, lambda: _lib.check(fn(), name))
                best[v] = min(best.get(v, 1e9), ms)
        for v in tune_vals:
            ms = best[v]
            print("%-26s %10s %12.1f %10.1f %8.4f" % (name, "-" if v is None else v, blocks / ms / 1e3, blocks * bpb / ms / 1e6, ms))
    if not args.only or any(o in "inter_recon_frame_p inter_recon_frame_b" for o in args.only.split(",")):
        inter_recon_rows(L, st, dev, max(args.rounds, 5))
    if not args.only or any(o in "inter_residual_frame_1080p inter_residual_frame_4k inter_residual_frame_1080p_lcu_qp inter_residual_frame_1080p_ts inter_residual_frame_1080p_lossless" for o in args.only.split(",")):
        inter_residual_rows(L, st, dev, max(args.rounds, 5))
    if not args.only or any(o in "sao_stats_frame_1080p sao_frame_1080p sao_frame_1080p_tiles4x2" for o in args.only.split(",")):
        sao_frame_rows(L, st, dev, max(args.rounds, 5))
    if not args.only or any(o in "intra_recon_frame_1080p_mixed intra_recon_frame_1080p_all intra_recon_frame_1080p_mixed_lcu_qp cu_qp_frame_1080p "
                            "intra_recon_frame_1080p_mixed_tiles4x2 intra_recon_frame_1080p_all_tiles4x2 cu_qp_frame_1080p_tiles4x2 "
                            "intra_recon_frame_1080p_mixed_ts intra_recon_frame_1080p_all_ts intra_recon_frame_1080p_mixed_ts_null intra_recon_frame_1080p_all_ts_null "
                            "intra_recon_frame_1080p_mixed_lossless intra_recon_frame_1080p_all_lossless" for o in args.only.split(",")):
        intra_recon_rows(L, st, dev, max(args.rounds, 5))
    if not args.only or any(o in "deblock_frame_1080p_tiles4x2" for o in args.only.split(",")):
        deblock_tiles_rows(L, st, max(args.rounds, 5), (dby, dbu, dbv, dbc, dbp, DW, DH))
    if not args.only or any(o in "intra_recon_frames_1080p_all_x4 intra_recon_frames_1080p_mixed_x4 inter_residual_frames_1080p_x4" for o in args.only.split(",")):
        chain_multi_rows(L, st, dev, max(args.rounds, 5), args.only.split(",") if args.only else [""])
    if not args.only or any(o in "intra_recon_frames_ts_1080p_all_tiles4x2_x4 intra_recon_frames_ts_1080p_mixed_tiles4x2_x4 intra_recon_frames_ts_1080p_all_trskip_x4 "
                            "inter_residual_frames_ts_1080p_x4" for o in args.only.split(",")):
        chain_multi_ts_rows(L, st, dev, max(args.rounds, 5), args.only.split(",") if args.only else [""])
    if not args.only or any(o in "cu_qp_frames_1080p_x4 deblock_frames_1080p_x4 sao_stats_frames_1080p_x4 sao_frames_1080p_x4 deblock_frames_1080p_tiles4x2_x4 "
                            "sao_frames_1080p_tiles4x2_x4" for o in args.only.split(",")):
        chain_filter_multi_rows(L, st, dev, max(args.rounds, 5), args.only.split(",") if args.only else [""])
    if not args.only or any(o in "inter_recon_frames_1080p_p_x4 inter_recon_frames_1080p_b_x4" for o in args.only.split(",")):
        inter_recon_multi_rows(L, st, dev, max(args.rounds, 5), args.only.split(",") if args.only else [""])
    if not args.only or any(o in "picture_hash_frame_1080p picture_hash_frame_4k picture_hash_frames_1080p_x16 array_checksum_batch_1080p" for o in args.only.split(",")):
        picture_hash_rows(L, st, dev, max(args.rounds, 5))
    if not args.only or any(o in "coeff_cost_batch_1080p_4x4 coeff_cost_batch_1080p_8x8 coeff_cost_batch_1080p_16x16 coeff_cost_batch_1080p_32x32" for o in args.only.split(",")):
        coeff_cost_rows(L, st, dev, max(args.rounds, 5), args.only.split(",") if args.only else [""])
    if not args.only or any(o in "rdoq_batch_1080p_4x4 rdoq_batch_1080p_8x8 rdoq_batch_1080p_16x16 rdoq_batch_1080p_32x32" for o in args.only.split(",")):
        rdoq_rows(L, st, dev, max(args.rounds, 5), args.only.split(",") if args.only else [""])
    if not args.only or any(o in "inter_residual_rdoq_1080p intra_recon_rdoq_1080p_mixed intra_recon_rdoq_1080p_all" for o in args.only.split(",")):
        rdoq_chain_rows(L, st, dev, max(args.rounds, 5), args.only.split(",") if args.only else [""])
    if not args.only or any(o in "inter_residual_frames_rdoq_1080p_x4 intra_recon_frames_rdoq_1080p_all_x4" for o in args.only.split(",")):
        rdoq_chain_multi_rows(L, st, dev, max(args.rounds, 5), args.only.split(",") if args.only else [""])


RDOQ_QP = 27


def rdoq_inputs(n, count):
    """What the rdoq_batch rows and --rdoq-cpu both run on: `count` luma TUs n wide from the recipe of tests/rdoq_cases.py (about 3 quantiser
    steps at DC, decaying along x + y) at QP 27, intra and inter alternating, a context set per 4096 coefficients drawn from the fixture's
    sets, the fixture's tables of flat lists.  numpy only, so that a machine without a device builds the same TUs."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rdoq_cases as K
    from kvazaar_amd import api
    z = np.load(os.path.join(ROOT, "tests", "golden", "rdoq.npz"))
    g = np.random.default_rng(47 + n)
    yy, xx = np.divmod(np.arange(n * n), n)
    amp = 3.0 * K.step_of(n, 0, RDOQ_QP) * np.exp(-(xx + yy) / (n / 2.0))
    coef = np.clip(np.rint(g.normal(0.0, 1.0, (count, n * n)) * amp * np.where(g.random((count, n * n)) < 0.04, 2.5, 1.0)), -32768, 32767).astype(np.int16)
    n_sets = (count * n * n + 4095) // 4096
    pick = g.integers(0, len(z["dumps"]), n_sets)
    dumps = z["dumps"][pick]
    descs = np.zeros(count, dtype=api.RDOQ_DESC)
    descs["src_offset"] = descs["dst_offset"] = np.arange(count, dtype=np.int64) * n * n
    descs["width"], descs["block_type"], descs["tr_depth"] = n, 1 + (np.arange(count) & 1), 1 if n < 32 else 0
    descs["ctx_index"] = (descs["src_offset"] // 4096) % 65536
    return coef, descs, dumps, K.lambda_of(RDOQ_QP), (z["quant"][0], z["err_scale"][0])


def rdoq_rows(L, st, dev, rounds, only, iters=5):
    """RDOQ: kvz_hip_rdoq_batch over one 1080p picture's worth (1920 x 1088) of luma TUs of one size (rdoq_inputs).  Device time by events,
    ms per call: median and min..max over the rounds, TUs per second and ns per TU.  `--rdoq-cpu` prints the compiled reference's kvz_rdoq
    on the same TUs where the reference is built."""
    import numpy as np
    from kvazaar_amd import api
    W, H = 1920, 1088
    prm = _lib.RdoqParams(1)
    print("%-32s %9s %10s %18s %10s %12s %10s" % ("kernel", "launches", "ms", "min..max ms", "TUs", "MTU / s", "ns / TU"))
    for n in (4, 8, 16, 32):
        name = "rdoq_batch_1080p_%dx%d" % (n, n)
        if not any(o in name for o in only):
            continue
        count = W * H // (n * n)
        coef, descs, dumps, lam, (quant, err) = rdoq_inputs(n, count)
        sets = np.array([api.coeff_ctx_from_dump(d, 256) for d in dumps], dtype=api.COEFF_CTX)
        states = np.array([api.rdoq_state_from_dump(d, lam, RDOQ_QP) for d in dumps], dtype=api.RDOQ_STATE)
        dev_arrays = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in (coef, descs, sets, states, quant, err)]
        d_c, d_d, d_s, d_t, d_q, d_e = dev_arrays
        dest = torch.zeros(coef.size, dtype=torch.int16, device=dev)
        tab = _lib.RdoqTables(d_q.data_ptr(), d_e.data_ptr())
        torch.cuda.synchronize()

        def fn():
            _lib.check(L.kvz_hip_rdoq_batch(d_c.data_ptr(), dest.data_ptr(), d_d.data_ptr(), count, d_s.data_ptr(), d_t.data_ptr(), len(sets), C.byref(tab),
                                            C.byref(prm), st), name)
        t = [timed(L, st, fn, iters=iters, warm=1) for _ in range(rounds)]
        ms = float(np.median(t))
        print("%-32s %9d %10.4f %18s %10d %12.3f %10.1f   %.2f levels / TU" % (name, 2, ms, "%.4f..%.4f" % (min(t), max(t)), count, count / ms / 1e3,
                                                                                ms * 1e6 / count, float((dest != 0).float().sum()) / count))


def rdoq_chain_rows(L, st, dev, rounds, only, iters=3):
    """RDOQ inside the two residual stages: kvz_hip_inter_residual_frame_rdoq on the picture of the inter_residual_frame_1080p row and
    kvz_hip_intra_recon_frame_rdoq on the two pictures of the intra_recon_frame_1080p_* rows, at QP 27 with flat lists, one context set per
    LCU row (drawn from the fixture's sets, lambda of QP 27), sign hiding as in those rows.  Per picture, interleaved round by round in one
    process: the entry with rdoq == NULL (the _sl entry on the same arguments: the stage without RDOQ), rdoq_skip 0 and rdoq_skip 1.  Device
    time by events, ms per call: median and min..max over the rounds; TUs of the stage, and ns per TU for the inter stage."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inter_residual_cases as RC
    import intra_recon_cases as XC
    import rdoq_cases as K
    W, H = 1920, 1080
    lx, ly = (W + 63) // 64, (H + 63) // 64
    z = np.load(os.path.join(ROOT, "tests", "golden", "rdoq.npz"))
    dumps = z["dumps"][np.random.default_rng(61).integers(0, len(z["dumps"]), ly)]
    sets = np.array([api.coeff_ctx_from_dump(d, 256) for d in dumps], dtype=api.COEFF_CTX)
    states = np.array([api.rdoq_state_from_dump(d, K.lambda_of(RDOQ_QP), RDOQ_QP) for d in dumps], dtype=api.RDOQ_STATE)
    lcu_ctx = np.repeat(np.arange(ly, dtype=np.uint16), lx)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_s, d_t, d_l, d_q, d_e = (up(a) for a in (sets, states, lcu_ctx, z["quant"][0], z["err_scale"][0]))
    rq = [_lib.RdoqSource(d_s.data_ptr(), d_t.data_ptr(), d_l.data_ptr(), _lib.RdoqTables(d_q.data_ptr(), d_e.data_ptr()), len(sets), skip) for skip in (0, 1)]
    print("%-34s %12s %9s %10s %18s %10s %10s" % ("kernel", "variant", "launches", "ms", "min..max ms", "TUs", "ns / TU"))
    pictures = (("inter_residual_rdoq_1080p", None), ("intra_recon_rdoq_1080p_mixed", 0.1), ("intra_recon_rdoq_1080p_all", 1.0))
    for name, share in pictures:
        if not any(o in name for o in only):
            continue
        up2 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
        if share is None:
            cus, _ = RC.make_map(W, H, 41, intra_share=0.0, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
            pred = RC.smooth_planes(W, H, 42)
            src, modes, signhide = RC.make_source(pred, cus, 43), None, 0
            n_tus, launches = len(RC.walk_tus(cus, W, H)), 5
        else:
            cus, _, modes = XC.make_map(W, H, 51, intra_share=share, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
            (src, pred), signhide = XC.make_planes(cus, 52), 1
            n_tus, launches = len(XC.walk_tus(cus, modes, W, H)), 1 + lx + 2 * (ly - 1)
        src_d, master, cus_d = [up2(p) for p in src], [up2(p) for p in pred], up2(cus)
        modes_d = up2(modes) if modes is not None else None
        recs = [[torch.empty_like(m) for m in master] for _ in range(iters + 1)]
        shapes = api.coeff_shapes(W, H)
        co_d = [torch.empty(shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)]
        cbf_d = torch.empty(cus.shape, dtype=torch.uint8, device=dev)
        cost_d = torch.empty(cus.shape + (6,), dtype=torch.int32, device=dev)
        table = api.ref_picture_table([(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2)], W, H)
        prm = api.inter_residual_params(RDOQ_QP, 0, signhide, 1)
        turn = [0]

        def call(source):
            r = recs[turn[0] % len(recs)]                # the inter stage works in place: a fresh copy of the prediction per call
            turn[0] += 1
            head = (table.ctypes.data, r[0].data_ptr(), W, r[1].data_ptr(), r[2].data_ptr(), W // 2, cus_d.data_ptr())
            outs = (co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(), cbf_d.data_ptr(), cost_d.data_ptr())
            ref = C.byref(source) if source is not None else None
            if modes_d is None:
                return L.kvz_hip_inter_residual_frame_rdoq(*head, *outs, None, None, ref, prm.ctypes.data, st)
            return L.kvz_hip_intra_recon_frame_rdoq(*head, modes_d.data_ptr(), *outs, None, None, None, ref, prm.ctypes.data, st)

        def refresh():
            for r in recs:
                for d, m in zip(r, master):
                    d.copy_(m)
            torch.cuda.synchronize()
            turn[0] = 0
        variants = (("rdoq == NULL", None), ("rdoq_skip 0", rq[0]), ("rdoq_skip 1", rq[1]))
        t = {v[0]: [] for v in variants}
        for _ in range(rounds):                          # interleaved round by round
            for what, source in variants:
                refresh()
                t[what].append(timed(L, st, lambda: _lib.check(call(source), name), iters=iters - 1, warm=1))
        for what, _ in variants:
            ms = float(np.median(t[what]))
            print("%-34s %12s %9d %10.4f %18s %10d %10.1f" % (name, what, launches, ms, "%.4f..%.4f" % (min(t[what]), max(t[what])), n_tus, ms * 1e6 / n_tus))


def rdoq_chain_multi_rows(L, st, dev, rounds, only, iters=3, n_pic=4):
    """RDOQ in the multi-picture entries: four 1080p P pictures through kvz_hip_inter_residual_frames_rdoq and four all-intra 1080p pictures
    through kvz_hip_intra_recon_frames_rdoq (the pictures, QP, sets and sign hiding of rdoq_chain_rows, rdoq_skip 0, every picture with
    outputs of its own), against four calls of the single-picture _rdoq entry on the same records; the two interleaved round by round in
    one process.  Device time by events, ms for the four pictures: median and min..max over the rounds."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inter_residual_cases as RC
    import intra_recon_cases as XC
    import rdoq_cases as K
    W, H = 1920, 1080
    lx, ly = (W + 63) // 64, (H + 63) // 64
    z = np.load(os.path.join(ROOT, "tests", "golden", "rdoq.npz"))
    dumps = z["dumps"][np.random.default_rng(61).integers(0, len(z["dumps"]), ly)]
    sets = np.array([api.coeff_ctx_from_dump(d, 256) for d in dumps], dtype=api.COEFF_CTX)
    states = np.array([api.rdoq_state_from_dump(d, K.lambda_of(RDOQ_QP), RDOQ_QP) for d in dumps], dtype=api.RDOQ_STATE)
    lcu_ctx = np.repeat(np.arange(ly, dtype=np.uint16), lx)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    up2 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
    d_s, d_t, d_l, d_q, d_e = (up(a) for a in (sets, states, lcu_ctx, z["quant"][0], z["err_scale"][0]))
    rq = _lib.RdoqSource(d_s.data_ptr(), d_t.data_ptr(), d_l.data_ptr(), _lib.RdoqTables(d_q.data_ptr(), d_e.data_ptr()), len(sets), 0)
    print("%-34s %16s %9s %10s %18s" % ("kernel", "variant", "launches", "ms", "min..max ms"))
    for name, intra in (("inter_residual_frames_rdoq_1080p_x4", False), ("intra_recon_frames_rdoq_1080p_all_x4", True)):
        if not any(o in name for o in only):
            continue
        if not intra:
            cus, _ = RC.make_map(W, H, 41, intra_share=0.0, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
            pred = RC.smooth_planes(W, H, 42)
            src, modes, signhide, launches = RC.make_source(pred, cus, 43), None, 0, 5
        else:
            cus, _, modes = XC.make_map(W, H, 51, intra_share=1.0, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
            (src, pred), signhide, launches = XC.make_planes(cus, 52), 1, 1 + lx + 2 * (ly - 1)
        src_d, master = [up2(p) for p in src], [up2(p) for p in pred]
        modes_d = up2(modes) if modes is not None else None
        table = api.ref_picture_table([(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2)], W, H)
        prm = api.inter_residual_params(RDOQ_QP, 0, signhide, 1)
        shapes = api.coeff_shapes(W, H)
        # per picture: a map, coefficients, flags and costs of its own, and a prediction per call of a round (the stages work in place)
        pics = []
        for _ in range(n_pic):
            pics.append(dict(cus=up2(cus), co=[torch.empty(shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)],
                             cbf=torch.empty(cus.shape, dtype=torch.uint8, device=dev), cost=torch.empty(cus.shape + (6,), dtype=torch.int32, device=dev),
                             recs=[[torch.empty_like(m) for m in master] for _ in range(iters + 1)]))
        turn = [0]

        def records():
            recs = (_lib.ChainPictureRdoq * n_pic)()
            for r, p in zip(recs, pics):
                rec = p["recs"][turn[0] % (iters + 1)]
                r.pic.src = _lib.RefPicture(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2, W, H)
                r.pic.rec_y, r.pic.rec_u, r.pic.rec_v, r.pic.stride_y, r.pic.stride_c = rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), W, W // 2
                r.pic.cus, r.pic.intra_modes = p["cus"].data_ptr(), modes_d.data_ptr() if intra else None
                r.pic.coeff_y, r.pic.coeff_u, r.pic.coeff_v = (c.data_ptr() for c in p["co"])
                r.pic.cbf_out, r.pic.costs = p["cbf"].data_ptr(), p["cost"].data_ptr()
                r.pic.params = _lib.InterResidualParams(RDOQ_QP, 0, signhide, 0, 1, 0)
                r.rdoq = C.pointer(rq)
            turn[0] += 1
            return recs

        def one_call():
            entry = L.kvz_hip_intra_recon_frames_rdoq if intra else L.kvz_hip_inter_residual_frames_rdoq
            _lib.check(entry(records(), n_pic, st), name)

        def four_calls():
            for r in records():
                p = r.pic
                head = (table.ctypes.data, p.rec_y, W, p.rec_u, p.rec_v, W // 2, p.cus)
                outs = (p.coeff_y, p.coeff_u, p.coeff_v, p.cbf_out, p.costs)
                if intra:
                    _lib.check(L.kvz_hip_intra_recon_frame_rdoq(*head, p.intra_modes, *outs, None, None, None, C.byref(rq), prm.ctypes.data, st), name)
                else:
                    _lib.check(L.kvz_hip_inter_residual_frame_rdoq(*head, *outs, None, None, C.byref(rq), prm.ctypes.data, st), name)

        def refresh():
            for p in pics:
                for r in p["recs"]:
                    for d, m in zip(r, master):
                        d.copy_(m)
            torch.cuda.synchronize()
            turn[0] = 0
        variants = (("four calls", four_calls, n_pic * launches), ("one call", one_call, launches))
        t = {v[0]: [] for v in variants}
        for _ in range(rounds):                          # interleaved round by round
            for what, fn, _n in variants:
                refresh()
                t[what].append(timed(L, st, fn, iters=iters - 1, warm=1))
        for what, _fn, n in variants:
            ms = float(np.median(t[what]))
            print("%-34s %16s %9d %10.4f %18s" % (name, what, n, ms, "%.4f..%.4f" % (min(t[what]), max(t[what]))))
        print("%-34s %16s %9s %10.2f" % (name, "four / one", "", float(np.median(t["four calls"])) / float(np.median(t["one call"]))))


def rdoq_cpu_rows(limit=4000):
    """the compiled reference's kvz_rdoq, one thread, on the first `limit` TUs of every rdoq_batch row (through ctypes: the call's own cost
    of a few microseconds is inside the figure)"""
    import time
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_rdoq as R
    if not R.available():
        print("rdoq_cpu: the compiled reference or its sources are not on this machine")
        return
    print("%-32s %10s %12s" % ("reference kvz_rdoq, 1 thread", "TUs", "us / TU"))
    for n in (4, 8, 16, 32):
        count = min(limit, 1920 * 1088 // (n * n))
        coef, descs, dumps, lam, _ = rdoq_inputs(n, count)
        R.rdoq(coef[0], n, 0, 0, 1, 0, RDOQ_QP, lam, dumps[0])
        t0 = time.perf_counter()
        for i in range(count):
            R.rdoq(coef[i], n, 0, 0, int(descs["block_type"][i]), int(descs["tr_depth"][i]), RDOQ_QP, lam, dumps[int(descs["ctx_index"][i])], 1, 0)
        dt = time.perf_counter() - t0
        print("%-32s %10d %12.2f" % ("kvz_rdoq_%dx%d" % (n, n), count, dt * 1e6 / count))


def coeff_cost_rows(L, st, dev, rounds, only, iters=10):
    """The CABAC coefficient pricing: kvz_hip_coeff_cost_batch over the luma TUs of one 1080p picture (1920 x 1088) cut into TUs of one
    size, every TU addressed in place, one context set per LCU.  The coefficients are what a quantiser leaves at a middling QP: levels
    of -3..3 whose density falls off from the DC corner (about a third of a 4x4 TU's positions hold a level, a twentieth of a 32x32
    TU's), one TU in six empty.  Device time by events, ms per call: median and min..max over the rounds, and ns per TU."""
    import numpy as np
    from kvazaar_amd import api
    g = torch.Generator(device=dev); g.manual_seed(43)
    W, H = 1920, 1088
    lcus = api.lcu_count(W, H)
    host = np.random.default_rng(43)
    sets = np.zeros(lcus, dtype=api.COEFF_CTX)
    sets["range"] = host.integers(256, 511, lcus)
    sets["ctx"][:, :138] = host.integers(0, 126, (lcus, 138))
    d_sets = torch.from_numpy(sets.view(np.uint8).reshape(-1).copy()).to(dev)
    prm = _lib.CoeffCostParams(1, 1, 0, 0)
    print("%-32s %9s %10s %18s %10s %10s" % ("kernel", "launches", "ms", "min..max ms", "TUs", "ns / TU"))
    for n in (4, 8, 16, 32):
        name = "coeff_cost_batch_1080p_%dx%d" % (n, n)
        if not any(o in name for o in only):
            continue
        count = W * H // (n * n)
        yy, xx = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
        keep = torch.exp(-(xx + yy).float() / (n / 4.0)).reshape(1, n * n)
        level = torch.randint(-3, 4, (count, n * n), dtype=torch.int16, device=dev, generator=g)
        level *= (torch.rand((count, n * n), device=dev, generator=g) < keep).to(torch.int16)
        level *= (torch.rand((count, 1), device=dev, generator=g) < 5.0 / 6.0).to(torch.int16)
        descs = np.zeros(count, dtype=api.COEFF_COST_DESC)
        descs["offset"] = np.arange(count, dtype=np.int64) * n * n
        descs["width"], descs["ctx_index"] = n, descs["offset"] // 4096
        d_descs = torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).to(dev)
        bits = torch.zeros(count, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def fn():
            _lib.check(L.kvz_hip_coeff_cost_batch(level.data_ptr(), d_descs.data_ptr(), count, d_sets.data_ptr(), lcus, C.byref(prm), bits.data_ptr(), st), name)
        t = [timed(L, st, fn, iters=iters, warm=2) for _ in range(rounds)]
        ms = float(np.median(t))
        print("%-32s %9d %10.4f %18s %10d %10.2f   mean %.1f bits / TU" % (name, 2, ms, "%.4f..%.4f" % (min(t), max(t)), count, ms * 1e6 / count,
                                                                        float(bits.float().mean())))


def picture_hash_rows(L, st, dev, rounds, iters=20):
    """The hash stage: kvz_hip_picture_hash_frame for one 1080p (1088 coded rows) and one 4K 4:2:0 picture with its source,
    kvz_hip_picture_hash_frames for sixteen 1080p pictures, kvz_hip_array_checksum_batch for the three planes of the 1080p picture.
    Device time by events, ms per call: median and min..max over the rounds; GB/s = bytes read (source and reconstruction, 3 per luma
    pixel; the plane entry reads the reconstruction alone) / time.  Beside them, in the same run, what a host does today for the same
    picture: kvz_hip_memcpy_d2h of the three planes (host wall clock, synchronised), then the compiled reference's generic8 per plane and
    the squared error as a numpy sum (the reference's own loop is a static function of its command-line tool) on the CPU -- where the
    reference is not built, numpy stands in for generic8 too and the row says so."""
    import time
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from kvazaar_amd import api
    g = torch.Generator(device=dev); g.manual_seed(41)
    print("%-32s %9s %10s %18s %10s" % ("kernel", "launches", "ms", "min..max ms", "GB/s"))

    def picture(W, H):
        src = [torch.randint(0, 256, (H >> c, W >> c), dtype=torch.uint8, device=dev, generator=g) for c in (0, 1, 1)]
        rec = [(p.to(torch.int16) + torch.randint(-6, 7, p.shape, dtype=torch.int16, device=dev, generator=g)).clamp_(0, 255).to(torch.uint8) for p in src]
        lcu = torch.empty(api.lcu_count(W, H) * 6, dtype=torch.int32, device=dev)
        out = torch.empty(5, dtype=torch.int64, device=dev)
        r = _lib.HashPicture()
        r.width, r.height, r.chroma = W, H, 1
        r.src = _lib.RefPicture(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), W, W // 2, W, H)
        r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c = rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), W, W // 2
        r.lcu_out, r.out = lcu.data_ptr(), out.data_ptr()
        return r, (src, rec, lcu, out)

    def row(name, launches, fn, nbytes):
        t = [timed(L, st, lambda: _lib.check(fn(), name), iters=iters, warm=3) for _ in range(rounds)]
        ms = float(np.median(t))
        print("%-32s %9d %10.4f %18s %10.1f" % (name, launches, ms, "%.4f..%.4f" % (min(t), max(t)), nbytes / ms / 1e6))

    def single(r):
        return lambda: L.kvz_hip_picture_hash_frame(C.byref(r.src), r.rec_y, r.stride_y, r.rec_u, r.rec_v, r.stride_c, r.width, r.height, 1, r.lcu_out, r.out, st)
    hd, keep_hd = picture(1920, 1088)
    uhd, keep_uhd = picture(3840, 2160)
    many = [picture(1920, 1088) for _ in range(16)]
    recs = (_lib.HashPicture * 16)(*[m[0] for m in many])
    planes = (_lib.HashPlane * 3)(*[_lib.HashPlane(p.data_ptr(), p.shape[1], p.shape[0], p.shape[1], 0) for p in keep_hd[1]])
    blocks = sum(L.kvz_hip_array_checksum_blocks(p.shape[1], p.shape[0]) for p in keep_hd[1])
    scratch, sums = torch.empty(blocks, dtype=torch.int32, device=dev), torch.empty(3, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    row("picture_hash_frame_1080p", 2, single(hd), 3.0 * 1920 * 1088)
    row("picture_hash_frame_4k", 2, single(uhd), 3.0 * 3840 * 2160)
    row("picture_hash_frames_1080p_x16", 2, lambda: L.kvz_hip_picture_hash_frames(recs, 16, st), 16 * 3.0 * 1920 * 1088)
    row("array_checksum_batch_1080p", 2, lambda: L.kvz_hip_array_checksum_batch(planes, 3, scratch.data_ptr(), sums.data_ptr(), st), 1.5 * 1920 * 1088)

    # what a host does today: the planes copied back, then the checksum and the squared error on the CPU
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import picture_hash_model as M
    import ref_lib as R
    fn = None
    if R.available():
        import gen_picture_hash_golden as G
        fn = G.reference_functions()["generic8"]
    for name, (r, keep) in (("1080p", (hd, keep_hd)), ("4k", (uhd, keep_uhd))):
        src, rec = keep[0], keep[1]
        host = [np.empty(tuple(p.shape), np.uint8) for p in rec]
        host_src = [p.cpu().numpy() for p in src]
        t_copy, t_sum, t_sse = [], [], []
        for _ in range(rounds):
            _lib.check(L.kvz_hip_stream_sync(st), "sync")
            t0 = time.perf_counter()
            for p, h in zip(rec, host):
                _lib.check(L.kvz_hip_memcpy_d2h(h.ctypes.data, p.data_ptr(), h.nbytes, st), "d2h")
            _lib.check(L.kvz_hip_stream_sync(st), "sync")
            t1 = time.perf_counter()
            sums_host = [G.call(fn, h, h.shape[1], h.shape[0]) if fn else M.plane_checksum(h, h.shape[1], h.shape[0]) for h in host]
            t2 = time.perf_counter()
            sse_host = [M.plane_sse(a, b, b.shape[1], b.shape[0]) for a, b in zip(host_src, host)]
            t3 = time.perf_counter()
            t_copy.append((t1 - t0) * 1e3); t_sum.append((t2 - t1) * 1e3); t_sse.append((t3 - t2) * 1e3)
        _lib.check(single(r)(), "picture_hash_frame")
        _lib.check(L.kvz_hip_stream_sync(st), "sync")
        got = keep[3].cpu().numpy()
        assert [int(v) & 0xFFFFFFFF for v in (got[0], got[0] >> 32, got[1])] == sums_host and [int(v) for v in got[2:5]] == sse_host, "the device and the host disagree"
        print("host today, %-5s: d2h of the planes %.3f ms, %s %.3f ms, squared error (numpy) %.3f ms  (medians of %d)" % (
            name, float(np.median(t_copy)), "generic8" if fn else "checksum (numpy, no reference built)", float(np.median(t_sum)), float(np.median(t_sse)), rounds))


def inter_recon_multi_rows(L, st, dev, rounds, only, pictures=4, iters=20):
    """Four distinct 1080p 4:2:0 CU maps from the generator of the inter_recon_frame rows (seeds of their own) through ONE call of
    kvz_hip_inter_recon_frames and, in the same rounds, interleaved, through four back-to-back calls of kvz_hip_inter_recon_frame.  _p: all
    four pictures name one shared reference; _b: every PU bi-predicted, each picture from two of three pool pictures.  ms per batch of
    four pictures: median and min..max over the rounds, and the ratio of the medians; `launches` is one call / four calls."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inter_recon_cases as IC
    from kvazaar_amd import api
    W, H = 1920, 1080
    g = torch.Generator(device=dev); g.manual_seed(29)
    planes = [[torch.randint(0, 256, (H >> c, W >> c), dtype=torch.uint8, device=dev, generator=g) for c in (0, 1, 1)] for _ in range(3)]
    pool = (_lib.RefPicture * 3)(*[_lib.RefPicture(p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), W, W // 2, W, H) for p in planes])
    dest = [[torch.empty((H >> c, W >> c), dtype=torch.uint8, device=dev) for c in (0, 1, 1)] for _ in range(pictures)]
    print("%-36s %9s %10s %18s %10s %18s %7s" % ("kernel", "launches", "ms", "min..max ms", "4 calls ms", "min..max ms", "ratio"))
    for name, n_refs in (("inter_recon_frames_1080p_p_x4", 1), ("inter_recon_frames_1080p_b_x4", 2)):
        if not any(o in name for o in only):
            continue
        recs, keep, single = (_lib.ReconPicture * pictures)(), [], []
        for i in range(pictures):
            cus, ref_LX = IC.random_cu_map(W, H, 331 + 10 * i, 1, False, intra_share=0.0, blank_share=0.0, bad_share=0.0, far=0.0)
            refs = (0,)
            if n_refs == 2:                                               # the same kind of map, every PU from both lists
                rs = np.random.default_rng(332 + 10 * i)
                cus["mv_dir"][cus["type"] == IC.CU_INTER] = 3
                cus["mv"][:, :, 1, :] = rs.integers(-160, 161, cus["mv"][:, :, 1, :].shape)
                ref_LX[1, 0] = 1
                refs = ((0, 1), (1, 2), (2, 0), (0, 2))[i % 4]
            cus_d = torch.from_numpy(cus.view(np.uint8).copy()).to(dev)
            prm = np.zeros(1, dtype=api.INTER_RECON_PARAMS)
            prm["chroma"], prm["n_refs"], prm["ref_LX"] = 1, n_refs, ref_LX
            table = (_lib.RefPicture * n_refs)(*[pool[k] for k in refs])
            d, r = dest[i], recs[i]
            r.pred_y, r.pred_u, r.pred_v, r.stride_y, r.stride_c = d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), W, W // 2
            r.width, r.height, r.cus = W, H, cus_d.data_ptr()
            r.refs[:n_refs] = refs
            r.params = _lib.InterReconParams.from_buffer_copy(prm.tobytes())
            keep.append((cus_d, prm, table))
            single.append((d[0].data_ptr(), W, d[1].data_ptr(), d[2].data_ptr(), W // 2, W, H, cus_d.data_ptr(), table, prm.ctypes.data, st))
        torch.cuda.synchronize()

        def multi():
            return L.kvz_hip_inter_recon_frames(recs, pictures, pool, 3, st)

        def four():
            for a in single:
                rc = L.kvz_hip_inter_recon_frame(*a)
                if rc:
                    return rc
            return 0
        t = {"multi": [], "single": []}
        for _ in range(rounds):                          # interleaved round by round
            t["multi"].append(timed(L, st, lambda: _lib.check(multi(), name), iters=iters, warm=3))
            t["single"].append(timed(L, st, lambda: _lib.check(four(), name + " (4 calls)"), iters=iters, warm=3))
        ms, ms4 = float(np.median(t["multi"])), float(np.median(t["single"]))
        print("%-36s %9s %10.4f %18s %10.4f %18s %7.2f" % (name, "%d/%d" % (1, pictures), ms, "%.4f..%.4f" % (min(t["multi"]), max(t["multi"])),
                                                           ms4, "%.4f..%.4f" % (min(t["single"]), max(t["single"])), ms4 / ms))


def chain_filter_multi_rows(L, st, dev, rounds, only, pictures=4, iters=20):
    """Four distinct 1080p 4:2:0 pictures of the kind the cu_qp_frame_1080p, deblock_frame_1080p, sao_stats_frame_1080p and sao_frame_1080p
    rows use (the same generators, seeds of their own) through ONE call of kvz_hip_cu_qp_frames / kvz_hip_deblock_frames /
    kvz_hip_sao_stats_frames / kvz_hip_sao_frames and, in the same rounds, interleaved, through four back-to-back calls of the
    single-picture entry that takes the same options: the untiled entries, and for *_tiles4x2_x4 the *_tiles entries with 4 x 2 uniform
    tiles in every picture.  ms per batch of four pictures: median and min..max over the rounds, and the ratio of the medians; `launches`
    counts dependent launches (one call / four calls).  Deblocking works in place on planes that earlier iterations have filtered, as in the
    deblock_frame_1080p row: both sides of a row see the same sequence of contents."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import intra_recon_cases as XC
    from patterns import deblock_case, deblock_params, sao_records
    from kvazaar_amd import api
    W, H, DH = 1920, 1080, 1088
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
    grid = api.uniform_tile_grid(W, H, 4, 2)                     # 1080 and the 1088 coded rows are the same 17 LCU rows
    grid_p = C.cast(grid.ctypes.data, C.POINTER(_lib.TileGrid))
    n_lcu = api.lcu_count(W, H)
    g = torch.Generator(device=dev); g.manual_seed(23)
    dbp = deblock_params(qp=36)
    qprm, tprm = np.zeros(1, dtype=api.CU_QP_PARAMS), np.zeros(1, dtype=api.CU_QP_TILES_PARAMS)
    qprm["start_qp"] = tprm["start_qp"] = 27
    luma_d, chro_d = torch.from_numpy(sao_records(n_lcu, 7)).to(dev), torch.from_numpy(sao_records(n_lcu, 8)).to(dev)
    keep, plain, tiled = [], (_lib.FilterPicture * pictures)(), (_lib.FilterPicture * pictures)()
    single = {k: [] for k in ("cu_qp", "deblock", "deblock_tiles", "sao_stats", "sao", "sao_tiles")}
    for i in range(pictures):
        # the QP map: a quadtree with about 10 % intra CUs, random coded flags, a QP per LCU
        cus, _, _ = XC.make_map(W, H, 171 + 10 * i, intra_share=0.1, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
        cus_d = up(cus)
        cbf_d = (torch.rand(cus.shape, device=dev, generator=g) < 0.5).to(torch.uint8)
        qp_d = up(np.random.default_rng(172 + 10 * i).integers(22, 43, n_lcu).astype(np.int8))
        last_d = torch.empty(n_lcu, dtype=torch.int8, device=dev)
        # deblocking: the picture of the deblock_frame_1080p row from another seed (1088 coded rows)
        ty, tu, tv, tcus = deblock_case(256, 128, 21 + i, qp=36)
        reps = (DH // 128 + 1, W // 256 + 1)
        dby, dbu, dbv = (up(np.tile(p, reps)[:DH >> c, :W >> c]) for p, c in ((ty, 0), (tu, 1), (tv, 1)))
        dbc = up(np.tile(tcus, reps)[:DH // 4, :W // 4])
        # SAO: a random source and a reconstruction near it, records as after a decision
        src = [torch.randint(0, 256, (H >> c, W >> c), dtype=torch.uint8, device=dev, generator=g) for c in (0, 1, 1)]
        rec = [(p.to(torch.int16) + torch.randint(-8, 9, p.shape, dtype=torch.int16, device=dev, generator=g)).clamp_(0, 255).to(torch.uint8) for p in src]
        dst = [torch.empty_like(p) for p in rec]
        stats = torch.empty(3 * n_lcu * 104, dtype=torch.int32, device=dev)
        cands = torch.empty(3 * n_lcu * 30, dtype=torch.int32, device=dev)
        table = api.ref_picture_table([(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), W, W // 2)], W, H)
        keep.append((cus_d, cbf_d, qp_d, last_d, dby, dbu, dbv, dbc, src, rec, dst, stats, cands, table))
        # one record per stage and picture would do; the rows share one with the fields of the stage they time, so the QP map and the
        # SAO stages (1080 rows) and deblocking (1088 rows) get records of their own
        for recs, gp in ((plain, None), (tiled, grid_p)):
            r = recs[i]
            r.width, r.height, r.chroma, r.deblock, r.grid = W, H, 1, _lib.DeblockParams.from_buffer_copy(dbp.tobytes()), gp
            r.src = _lib.RefPicture(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), W, W // 2, W, H)
            r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c = rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), W, W // 2
            r.dst_y, r.dst_u, r.dst_v, r.dst_stride_y, r.dst_stride_c = dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), W, W // 2
            r.cus, r.cbf, r.lcu_qp, r.lcu_last_qp = cus_d.data_ptr(), cbf_d.data_ptr(), qp_d.data_ptr(), last_d.data_ptr()
            r.stats, r.cands, r.sao_luma, r.sao_chroma = stats.data_ptr(), cands.data_ptr(), luma_d.data_ptr(), chro_d.data_ptr()
            r.cu_qp = _lib.CuQpTilesParams(27, 0)
        planes = (rec[0].data_ptr(), W, rec[1].data_ptr(), rec[2].data_ptr(), W // 2)
        dplanes = (dby.data_ptr(), W, dbu.data_ptr(), dbv.data_ptr(), W // 2)
        sao_args = planes + (dst[0].data_ptr(), W, dst[1].data_ptr(), dst[2].data_ptr(), W // 2, W, H, luma_d.data_ptr(), chro_d.data_ptr(), 1)
        single["cu_qp"].append((L.kvz_hip_cu_qp_frame, (cus_d.data_ptr(), cbf_d.data_ptr(), W, H, qp_d.data_ptr(), last_d.data_ptr(), qprm.ctypes.data, st)))
        single["deblock"].append((L.kvz_hip_deblock_frame, dplanes + (W, DH, dbc.data_ptr(), dbp.ctypes.data, st)))
        single["deblock_tiles"].append((L.kvz_hip_deblock_frame_tiles, dplanes + (W, DH, dbc.data_ptr(), grid.ctypes.data, dbp.ctypes.data, st)))
        single["sao_stats"].append((L.kvz_hip_sao_stats_frame, (table.ctypes.data,) + planes + (1, stats.data_ptr(), cands.data_ptr(), st)))
        single["sao"].append((L.kvz_hip_sao_frame, sao_args + (st,)))
        single["sao_tiles"].append((L.kvz_hip_sao_frame_tiles, sao_args + (grid.ctypes.data, st)))
    # deblocking: the records of the 1088-row pictures
    deb, deb_tiled = (_lib.FilterPicture * pictures)(), (_lib.FilterPicture * pictures)()
    for recs, gp in ((deb, None), (deb_tiled, grid_p)):
        for i, k in enumerate(keep):
            r = recs[i]
            r.width, r.height, r.chroma, r.deblock, r.grid = W, DH, 1, _lib.DeblockParams.from_buffer_copy(dbp.tobytes()), gp
            r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c, r.cus = k[4].data_ptr(), k[5].data_ptr(), k[6].data_ptr(), W, W // 2, k[7].data_ptr()
    rows = (("cu_qp_frames_1080p_x4", 3, L.kvz_hip_cu_qp_frames, plain, "cu_qp"), ("deblock_frames_1080p_x4", 2, L.kvz_hip_deblock_frames, deb, "deblock"),
            ("sao_stats_frames_1080p_x4", 1, L.kvz_hip_sao_stats_frames, plain, "sao_stats"), ("sao_frames_1080p_x4", 1, L.kvz_hip_sao_frames, plain, "sao"),
            ("deblock_frames_1080p_tiles4x2_x4", 2, L.kvz_hip_deblock_frames, deb_tiled, "deblock_tiles"),
            ("sao_frames_1080p_tiles4x2_x4", 1, L.kvz_hip_sao_frames, tiled, "sao_tiles"))
    print("%-36s %9s %10s %18s %10s %18s %7s" % ("kernel", "launches", "ms", "min..max ms", "4 calls ms", "min..max ms", "ratio"))
    torch.cuda.synchronize()
    for name, launches, entry, recs, key in rows:
        if not any(o in name for o in only):
            continue

        def multi():
            return entry(recs, pictures, st)

        def four():
            for fn, a in single[key]:
                rc = fn(*a)
                if rc:
                    return rc
            return 0
        t = {"multi": [], "single": []}
        for _ in range(rounds):                          # interleaved round by round
            t["multi"].append(timed(L, st, lambda: _lib.check(multi(), name), iters=iters, warm=3))
            t["single"].append(timed(L, st, lambda: _lib.check(four(), name + " (4 calls)"), iters=iters, warm=3))
        ms, ms4 = float(np.median(t["multi"])), float(np.median(t["single"]))
        print("%-36s %9s %10.4f %18s %10.4f %18s %7.2f" % (name, "%d/%d" % (launches, pictures * launches), ms, "%.4f..%.4f" % (min(t["multi"]), max(t["multi"])),
                                                           ms4, "%.4f..%.4f" % (min(t["single"]), max(t["single"])), ms4 / ms))


def chain_multi_ts_rows(L, st, dev, rounds, only, pictures=4):
    """The pictures of chain_multi_rows through ONE call of kvz_hip_intra_recon_frames_ts / kvz_hip_inter_residual_frames_ts and, in the same
    rounds, interleaved, through four back-to-back calls of the single-picture entry that takes the same options: *_tiles4x2_x4 with 4 x 2
    uniform tiles in every picture against kvz_hip_intra_recon_frame_tiles, *_trskip_x4 untiled with one bit cost against
    kvz_hip_intra_recon_frame_ts, the inter row with one bit cost against kvz_hip_inter_residual_frame_ts.  One QP per picture, flat lists.
    ms per batch of four pictures: median and min..max over the rounds, and the ratio of the medians; `launches` counts dependent launches."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inter_residual_cases as RC
    import intra_recon_cases as XC
    from kvazaar_amd import api
    W, H = 1920, 1080
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
    shapes = api.coeff_shapes(W, H)
    grid = api.uniform_tile_grid(W, H, 4, 2)
    grid_p = C.cast(grid.ctypes.data, C.POINTER(_lib.TileGrid))
    waves = {False: (W + 63) // 64 + 2 * ((H + 63) // 64 - 1),
             True: int(max(np.diff(grid["col_bd"][0, :5])) + 2 * (max(np.diff(grid["row_bd"][0, :3])) - 1))}
    ts = _lib.TrSkip(58, 0, None)                       # (int)(lambda + 0.5) at QP 32
    print("%-46s %9s %10s %18s %10s %18s %7s" % ("kernel", "launches", "ms", "min..max ms", "4 calls ms", "min..max ms", "ratio"))

    def outputs(cus):
        return ([torch.empty(shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)],
                torch.zeros(cus.shape, dtype=torch.uint8, device=dev), torch.empty(cus.shape + (6,), dtype=torch.int32, device=dev),
                torch.zeros(cus.shape, dtype=torch.uint8, device=dev))

    def record(src_d, rec_d, cus_d, modes_d, co_d, cbf_d, cost_d, skip_d, prm, tiled, skip):
        r = _lib.ChainPictureTs()
        r.pic.src = _lib.RefPicture(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2, W, H)
        r.pic.rec_y, r.pic.rec_u, r.pic.rec_v, r.pic.stride_y, r.pic.stride_c = rec_d[0].data_ptr(), rec_d[1].data_ptr(), rec_d[2].data_ptr(), W, W // 2
        r.pic.cus, r.pic.intra_modes = cus_d.data_ptr(), modes_d.data_ptr() if modes_d is not None else None
        r.pic.coeff_y, r.pic.coeff_u, r.pic.coeff_v = co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr()
        r.pic.cbf_out, r.pic.costs = cbf_d.data_ptr(), cost_d.data_ptr()
        r.pic.params = _lib.InterResidualParams(int(prm["qp"][0]), int(prm["slice_is_intra"][0]), int(prm["signhide"][0]), 0, 1, 0)
        if tiled:
            r.grid = grid_p
        if skip:
            r.ts, r.tr_skip_out = C.pointer(ts), skip_d.data_ptr()
        return r

    def report(name, launches, multi, single):
        ms, ms4 = float(np.median(multi)), float(np.median(single))
        print("%-46s %9s %10.3f %18s %10.3f %18s %7.2f" % (name, "%d/%d" % (launches, pictures * launches), ms, "%.3f..%.3f" % (min(multi), max(multi)), ms4,
                                                           "%.3f..%.3f" % (min(single), max(single)), ms4 / ms))

    for name, share, tiled, skip in (("intra_recon_frames_ts_1080p_mixed_tiles4x2_x4", 0.1, True, False),
                                     ("intra_recon_frames_ts_1080p_all_tiles4x2_x4", 1.0, True, False),
                                     ("intra_recon_frames_ts_1080p_all_trskip_x4", 1.0, False, True)):
        if not any(o in name for o in only):
            continue
        prm = api.inter_residual_params(32, 0, 1, 1)
        keep, calls = [], []
        for i in range(pictures):
            cus, _, modes = XC.make_map(W, H, 151 + 10 * i, intra_share=share, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
            src, rec = XC.make_planes(cus, 152 + 10 * i)
            src_d, rec_d, cus_d, modes_d = [up(p) for p in src], [up(p) for p in rec], up(cus), up(modes)
            co_d, cbf_d, cost_d, skip_d = outputs(cus)
            table = api.ref_picture_table([(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2)], W, H)
            keep.append((src_d, rec_d, cus_d, modes_d, co_d, cbf_d, cost_d, skip_d, table))
            planes = (table.ctypes.data, rec_d[0].data_ptr(), W, rec_d[1].data_ptr(), rec_d[2].data_ptr(), W // 2, cus_d.data_ptr(), modes_d.data_ptr(),
                      co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(), cbf_d.data_ptr(), cost_d.data_ptr(), None)
            if skip:
                calls.append(planes + (None, None, C.byref(ts), skip_d.data_ptr(), prm.ctypes.data, st))
            else:
                calls.append(planes + (grid.ctypes.data, prm.ctypes.data, st))
        records = (_lib.ChainPictureTs * pictures)(*[record(*k[:8], prm, tiled, skip) for k in keep])
        entry = L.kvz_hip_intra_recon_frame_ts if skip else L.kvz_hip_intra_recon_frame_tiles

        def multi():                                     # in place and independent of what the intra CUs hold: no fresh copy needed
            return L.kvz_hip_intra_recon_frames_ts(records, pictures, st)

        def single():
            for a in calls:
                rc = entry(*a)
                if rc:
                    return rc
            return 0
        torch.cuda.synchronize()
        t = {"multi": [], "single": []}
        for _ in range(rounds):                          # interleaved round by round
            t["multi"].append(timed(L, st, lambda: _lib.check(multi(), name), iters=3, warm=1))
            t["single"].append(timed(L, st, lambda: _lib.check(single(), name + " (4 calls)"), iters=3, warm=1))
        report(name, waves[tiled] + 1, t["multi"], t["single"])
    name = "inter_residual_frames_ts_1080p_x4"
    if any(o in name for o in only):
        iters = 6
        prm = api.inter_residual_params(32, 0, 0, 1)
        keep = []
        for i in range(pictures):
            cus, _ = RC.make_map(W, H, 141 + 10 * i, intra_share=0.0, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
            pred = RC.smooth_planes(W, H, 142 + 10 * i)
            src = RC.make_source(pred, cus, 143 + 10 * i)
            src_d, master, cus_d = [up(p) for p in src], [up(p) for p in pred], up(cus)
            recs = [[torch.empty_like(m) for m in master] for _ in range(iters)]
            co_d, cbf_d, cost_d, skip_d = outputs(cus)
            table = api.ref_picture_table([(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2)], W, H)
            keep.append((src_d, master, recs, cus_d, co_d, cbf_d, cost_d, skip_d, table))
        # one table of records and one argument list per picture for every set of fresh predictions
        batches = [(_lib.ChainPictureTs * pictures)(*[record(k[0], k[2][j], k[3], None, k[4], k[5], k[6], k[7], prm, False, True) for k in keep])
                   for j in range(iters)]
        calls = [[(k[8].ctypes.data, k[2][j][0].data_ptr(), W, k[2][j][1].data_ptr(), k[2][j][2].data_ptr(), W // 2, k[3].data_ptr(), k[4][0].data_ptr(),
                   k[4][1].data_ptr(), k[4][2].data_ptr(), k[5].data_ptr(), k[6].data_ptr(), None, None, C.byref(ts), k[7].data_ptr(), prm.ctypes.data, st)
                  for k in keep] for j in range(iters)]
        turn = [0]

        def multi():
            turn[0] += 1
            return L.kvz_hip_inter_residual_frames_ts(batches[(turn[0] - 1) % iters], pictures, st)

        def single():
            turn[0] += 1
            for a in calls[(turn[0] - 1) % iters]:
                rc = L.kvz_hip_inter_residual_frame_ts(*a)
                if rc:
                    return rc
            return 0

        def refresh():
            for k in keep:
                for r in k[2]:
                    for d, m in zip(r, k[1]):
                        d.copy_(m)
            torch.cuda.synchronize()
            turn[0] = 0
        t = {"multi": [], "single": []}
        for _ in range(rounds):
            refresh()
            t["multi"].append(timed(L, st, lambda: _lib.check(multi(), name), iters=iters - 1, warm=1))
            refresh()
            t["single"].append(timed(L, st, lambda: _lib.check(single(), name + " (4 calls)"), iters=iters - 1, warm=1))
        report(name, 5, t["multi"], t["single"])


def chain_multi_rows(L, st, dev, rounds, only, pictures=4):
    """Four distinct 1080p pictures of the kind the intra_recon_frame_1080p_* and inter_residual_frame_1080p rows use (the same generators,
    seeds of their own) through ONE call of kvz_hip_intra_recon_frames / kvz_hip_inter_residual_frames, and in the same rounds, interleaved,
    through four back-to-back calls of the single-picture _qp entry (lcu_qp NULL, one QP: the kernels the plain rows time).  ms per
    batch of four pictures: median and min..max over the rounds, and the ratio of the medians.  `launches` counts dependent launches.
    The inter entry works in place, so every timed call gets fresh copies of the predictions (copied outside the timed region)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inter_residual_cases as RC
    import intra_recon_cases as XC
    from kvazaar_amd import api
    W, H = 1920, 1080
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
    shapes = api.coeff_shapes(W, H)
    waves = (W + 63) // 64 + 2 * ((H + 63) // 64 - 1)
    print("%-36s %9s %10s %18s %10s %18s %7s" % ("kernel", "launches", "ms", "min..max ms", "4 calls ms", "min..max ms", "ratio"))

    def outputs(cus):
        return ([torch.empty(shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)],
                torch.zeros(cus.shape, dtype=torch.uint8, device=dev), torch.empty(cus.shape + (6,), dtype=torch.int32, device=dev))

    def record(src_d, rec_d, cus_d, modes_d, co_d, cbf_d, cost_d, prm):
        r = _lib.ChainPicture()
        r.src = _lib.RefPicture(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2, W, H)
        r.rec_y, r.rec_u, r.rec_v, r.stride_y, r.stride_c = rec_d[0].data_ptr(), rec_d[1].data_ptr(), rec_d[2].data_ptr(), W, W // 2
        r.cus, r.intra_modes = cus_d.data_ptr(), modes_d.data_ptr() if modes_d is not None else None
        r.coeff_y, r.coeff_u, r.coeff_v, r.cbf_out, r.costs = co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(), cbf_d.data_ptr(), cost_d.data_ptr()
        r.params = _lib.InterResidualParams(int(prm["qp"][0]), int(prm["slice_is_intra"][0]), int(prm["signhide"][0]), 0, 1, 0)
        return r

    def report(name, launches, multi, single):
        ms, ms4 = float(np.median(multi)), float(np.median(single))
        print("%-36s %9s %10.3f %18s %10.3f %18s %7.2f" % (name, "%d/%d" % (launches, pictures * launches), ms, "%.3f..%.3f" % (min(multi), max(multi)), ms4,
                                                           "%.3f..%.3f" % (min(single), max(single)), ms4 / ms))

    for name, share in (("intra_recon_frames_1080p_mixed_x4", 0.1), ("intra_recon_frames_1080p_all_x4", 1.0)):
        if not any(o in name for o in only):
            continue
        prm = api.inter_residual_params(32, 0, 1, 1)
        keep, calls = [], []
        for i in range(pictures):
            cus, _, modes = XC.make_map(W, H, 151 + 10 * i, intra_share=share, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
            src, rec = XC.make_planes(cus, 152 + 10 * i)
            src_d, rec_d, cus_d, modes_d = [up(p) for p in src], [up(p) for p in rec], up(cus), up(modes)
            co_d, cbf_d, cost_d = outputs(cus)
            table = api.ref_picture_table([(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2)], W, H)
            keep.append((src_d, rec_d, cus_d, modes_d, co_d, cbf_d, cost_d, table))
            calls.append((table.ctypes.data, rec_d[0].data_ptr(), W, rec_d[1].data_ptr(), rec_d[2].data_ptr(), W // 2, cus_d.data_ptr(), modes_d.data_ptr(),
                          co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(), cbf_d.data_ptr(), cost_d.data_ptr(), None, prm.ctypes.data, st))
        records = (_lib.ChainPicture * pictures)(*[record(k[0], k[1], k[2], k[3], k[4], k[5], k[6], prm) for k in keep])

        def multi():                                     # in place and independent of what the intra CUs hold: no fresh copy needed
            return L.kvz_hip_intra_recon_frames(records, pictures, st)

        def single():
            for a in calls:
                rc = L.kvz_hip_intra_recon_frame_qp(*a)
                if rc:
                    return rc
            return 0
        torch.cuda.synchronize()
        t = {"multi": [], "single": []}
        for _ in range(rounds):                          # interleaved round by round
            t["multi"].append(timed(L, st, lambda: _lib.check(multi(), name), iters=3, warm=1))
            t["single"].append(timed(L, st, lambda: _lib.check(single(), name + " (4 calls)"), iters=3, warm=1))
        report(name, waves + 1, t["multi"], t["single"])
    name = "inter_residual_frames_1080p_x4"
    if any(o in name for o in only):
        iters = 6
        prm = api.inter_residual_params(32, 0, 0, 1)
        keep = []
        for i in range(pictures):
            cus, _ = RC.make_map(W, H, 141 + 10 * i, intra_share=0.0, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
            pred = RC.smooth_planes(W, H, 142 + 10 * i)
            src = RC.make_source(pred, cus, 143 + 10 * i)
            src_d, master, cus_d = [up(p) for p in src], [up(p) for p in pred], up(cus)
            recs = [[torch.empty_like(m) for m in master] for _ in range(iters)]
            co_d, cbf_d, cost_d = outputs(cus)
            table = api.ref_picture_table([(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2)], W, H)
            keep.append((src_d, master, recs, cus_d, co_d, cbf_d, cost_d, table))
        # one table of records and one argument list per picture for every set of fresh predictions
        batches = [(_lib.ChainPicture * pictures)(*[record(k[0], k[2][j], k[3], None, k[4], k[5], k[6], prm) for k in keep]) for j in range(iters)]
        calls = [[(k[7].ctypes.data, k[2][j][0].data_ptr(), W, k[2][j][1].data_ptr(), k[2][j][2].data_ptr(), W // 2, k[3].data_ptr(), k[4][0].data_ptr(),
                   k[4][1].data_ptr(), k[4][2].data_ptr(), k[5].data_ptr(), k[6].data_ptr(), None, prm.ctypes.data, st) for k in keep] for j in range(iters)]
        turn = [0]

        def multi():
            turn[0] += 1
            return L.kvz_hip_inter_residual_frames(batches[(turn[0] - 1) % iters], pictures, st)

        def single():
            turn[0] += 1
            for a in calls[(turn[0] - 1) % iters]:
                rc = L.kvz_hip_inter_residual_frame_qp(*a)
                if rc:
                    return rc
            return 0

        def refresh():
            for k in keep:
                for r in k[2]:
                    for d, m in zip(r, k[1]):
                        d.copy_(m)
            torch.cuda.synchronize()
            turn[0] = 0
        t = {"multi": [], "single": []}
        for _ in range(rounds):
            refresh()
            t["multi"].append(timed(L, st, lambda: _lib.check(multi(), name), iters=iters - 1, warm=1))
            refresh()
            t["single"].append(timed(L, st, lambda: _lib.check(single(), name + " (4 calls)"), iters=iters - 1, warm=1))
        report(name, 5, t["multi"], t["single"])


def deblock_tiles_rows(L, st, rounds, picture, iters=20):
    """kvz_hip_deblock_frame_tiles with 4 x 2 uniform tiles on the picture of the deblock_frame_1080p row, interleaved round by round with
    the untiled entry; medians and min..max over the rounds (two launches each)."""
    import numpy as np
    from kvazaar_amd import api
    y, u, v, cus, prm, W, H = picture
    grid = api.uniform_tile_grid(W, H, 4, 2)
    fns = {"deblock_frame_1080p": lambda: L.kvz_hip_deblock_frame(y.data_ptr(), W, u.data_ptr(), v.data_ptr(), W // 2, W, H, cus.data_ptr(), prm.ctypes.data, st),
           "deblock_frame_1080p_tiles4x2": lambda: L.kvz_hip_deblock_frame_tiles(y.data_ptr(), W, u.data_ptr(), v.data_ptr(), W // 2, W, H, cus.data_ptr(),
                                                                                 grid.ctypes.data, prm.ctypes.data, st)}
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(L, st, lambda fn=fn, k=k: _lib.check(fn(), k), iters=iters, warm=3))
    print("%-30s %10s %12s %8s %16s" % ("kernel", "launches", "frames/s", "ms", "min..max ms"))
    for k in fns:
        ms = float(np.median(t[k]))
        print("%-30s %10d %12.1f %8.4f %7.4f..%7.4f" % (k, 2, 1e3 / ms, ms, min(t[k]), max(t[k])))


def intra_recon_rows(L, st, dev, rounds, iters=3):
    """Intra prediction + residual coding of whole 1080p 4:2:0 pictures in coding order (kvz_hip_intra_recon_frame): a random quadtree
    with about 10 % of its CUs intra (the rest inter: their LCU-workgroups leave after reading the map) and an all-intra one, modes
    and tr_depth as tests/intra_recon_cases.py sets them.  The stage is a chain of dependent launches (one per wavefront of LCUs) and
    of dependent TUs inside an LCU, so the figure is a latency, not a throughput: ms per picture, medians (and min..max) over the
    rounds.  On the mixed picture the same call with a QP per LCU (kvz_hip_intra_recon_frame_qp, QPs 22..42 drawn per LCU) and the QP
    map from its flags (kvz_hip_cu_qp_frame) are timed in the same rounds, interleaved with the one-QP row.  Both pictures also go
    through kvz_hip_intra_recon_frame_tiles with 4 x 2 uniform tiles (rows *_tiles4x2; the mixed picture's QP map through
    kvz_hip_cu_qp_frame_tiles as well), interleaved with their untiled rows; `launches` is the number of dependent wavefront launches.
    Rows *_ts: the untiled call through kvz_hip_intra_recon_frame_ts with one bit cost (transform skip: every 4x4 luma TU coded twice),
    in the same rounds; *_ts_null: the same entry with ts == NULL, which runs the kernel of the _tiles entry on one tile -- the
    instantiation the _ts kernel extends, and so its baseline (the one-QP kernel of the plain row is another instantiation).
    Rows *_lossless: the same pictures through kvz_hip_intra_recon_frame_lossless (implicit_rdpcm on), in the same rounds: one launch,
    no dependence between TUs.  Its traffic -- source read, rec and 2-byte coefficients written, over the intra share of the 4:2:0
    picture -- and that traffic's share of the 8 TB/s HBM figure are printed below the rows."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import intra_recon_cases as XC
    from kvazaar_amd import api
    W, H = 1920, 1080
    print("%-38s %8s %10s %9s %12s %10s %18s" % ("kernel", "intra %", "TUs", "launches", "frames/s", "ms", "min..max ms"))
    grid = api.uniform_tile_grid(W, H, 4, 2)
    waves = lambda bx, by: max(np.diff(bx)) + 2 * (max(np.diff(by)) - 1)
    n_launch = {False: waves([0, (W + 63) // 64], [0, (H + 63) // 64]), True: waves(grid["col_bd"][0, :5], grid["row_bd"][0, :3])}
    tprm = np.zeros(1, dtype=api.CU_QP_TILES_PARAMS)
    tprm["start_qp"] = 32
    for name, share in (("intra_recon_frame_1080p_mixed", 0.1), ("intra_recon_frame_1080p_all", 1.0)):
        cus, _, modes = XC.make_map(W, H, 51, intra_share=share, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
        src, rec = XC.make_planes(cus, 52)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
        src_d, rec_d, cus_d, modes_d = [up(p) for p in src], [up(p) for p in rec], up(cus), up(modes)
        shapes = api.coeff_shapes(W, H)
        co_d = [torch.empty(shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)]
        cbf_d = torch.empty(cus.shape, dtype=torch.uint8, device=dev)
        cost_d = torch.empty(cus.shape + (6,), dtype=torch.int32, device=dev)
        table = api.ref_picture_table([(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2)], W, H)
        prm = api.inter_residual_params(32, 0, 1, 1)

        def frame():                                     # in place and independent of what the intra CUs hold: no fresh copy needed
            return L.kvz_hip_intra_recon_frame(table.ctypes.data, rec_d[0].data_ptr(), W, rec_d[1].data_ptr(), rec_d[2].data_ptr(), W // 2,
                                               cus_d.data_ptr(), modes_d.data_ptr(), co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(),
                                               cbf_d.data_ptr(), cost_d.data_ptr(), prm.ctypes.data, st)
        lcu_qp_d = up(np.random.default_rng(53).integers(22, 43, api.lcu_count(W, H)).astype(np.int8))
        last_d = torch.empty(api.lcu_count(W, H), dtype=torch.int8, device=dev)
        qprm = np.zeros(1, dtype=api.CU_QP_PARAMS)
        qprm["start_qp"] = 32

        def frame_qp():
            return L.kvz_hip_intra_recon_frame_qp(table.ctypes.data, rec_d[0].data_ptr(), W, rec_d[1].data_ptr(), rec_d[2].data_ptr(), W // 2,
                                                  cus_d.data_ptr(), modes_d.data_ptr(), co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(),
                                                  cbf_d.data_ptr(), cost_d.data_ptr(), lcu_qp_d.data_ptr(), prm.ctypes.data, st)

        def qp_map():                                    # cbf_d: the flags of the intra CUs as the call before left them, 0 elsewhere
            return L.kvz_hip_cu_qp_frame(cus_d.data_ptr(), cbf_d.data_ptr(), W, H, lcu_qp_d.data_ptr(), last_d.data_ptr(), qprm.ctypes.data, st)

        def frame_tiles():                               # one QP per call, as `frame`
            return L.kvz_hip_intra_recon_frame_tiles(table.ctypes.data, rec_d[0].data_ptr(), W, rec_d[1].data_ptr(), rec_d[2].data_ptr(), W // 2,
                                                     cus_d.data_ptr(), modes_d.data_ptr(), co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(),
                                                     cbf_d.data_ptr(), cost_d.data_ptr(), None, grid.ctypes.data, prm.ctypes.data, st)

        def qp_map_tiles():
            return L.kvz_hip_cu_qp_frame_tiles(cus_d.data_ptr(), cbf_d.data_ptr(), W, H, lcu_qp_d.data_ptr(), last_d.data_ptr(), grid.ctypes.data,
                                               tprm.ctypes.data, st)
        skip_d = torch.zeros(cus.shape, dtype=torch.uint8, device=dev)
        ts = _lib.TrSkip(58, 0, None)                   # (int)(lambda + 0.5) at QP 32

        def frame_ts():                                  # one QP per call, no tiles, flat lists, as `frame`
            return L.kvz_hip_intra_recon_frame_ts(table.ctypes.data, rec_d[0].data_ptr(), W, rec_d[1].data_ptr(), rec_d[2].data_ptr(), W // 2,
                                                  cus_d.data_ptr(), modes_d.data_ptr(), co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(),
                                                  cbf_d.data_ptr(), cost_d.data_ptr(), None, None, None, C.byref(ts), skip_d.data_ptr(),
                                                  prm.ctypes.data, st)

        def frame_ts_null():                             # ts == NULL: the _sl entry, i.e. the _tiles kernel on one tile -- the kernel the _ts one extends
            return L.kvz_hip_intra_recon_frame_ts(table.ctypes.data, rec_d[0].data_ptr(), W, rec_d[1].data_ptr(), rec_d[2].data_ptr(), W // 2,
                                                  cus_d.data_ptr(), modes_d.data_ptr(), co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(),
                                                  cbf_d.data_ptr(), cost_d.data_ptr(), None, None, None, None, None, prm.ctypes.data, st)
        ll = _lib.Lossless(1, 1, (0, 0))

        def frame_lossless():                            # reads the source only: in place, no fresh copy needed
            return L.kvz_hip_intra_recon_frame_lossless(table.ctypes.data, rec_d[0].data_ptr(), W, rec_d[1].data_ptr(), rec_d[2].data_ptr(), W // 2,
                                                        cus_d.data_ptr(), modes_d.data_ptr(), co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(),
                                                        cbf_d.data_ptr(), cost_d.data_ptr(), None, C.byref(ll), st)
        rows = [(name, frame, iters), (name + "_ts", frame_ts, iters), (name + "_ts_null", frame_ts_null, iters), (name + "_tiles4x2", frame_tiles, iters),
                (name + "_lossless", frame_lossless, 20)]
        if share < 1.0:
            rows += [(name + "_lcu_qp", frame_qp, iters), ("cu_qp_frame_1080p", qp_map, 20), ("cu_qp_frame_1080p_tiles4x2", qp_map_tiles, 20)]
        cbf_d.zero_()
        torch.cuda.synchronize()
        t = {r[0]: [] for r in rows}
        for _ in range(rounds):                          # interleaved round by round
            for (rname, fn, it) in rows:
                t[rname].append(timed(L, st, lambda: _lib.check(fn(), rname), iters=it, warm=1))
        m, _, _ = XC.intra_mask(cus, W, H)
        for (rname, fn, it) in rows:
            ms = float(np.median(t[rname]))
            launches = 3 if rname.startswith("cu_qp") else (1 if rname.endswith("_lossless") else n_launch[rname.endswith("_tiles4x2")])
            print("%-38s %8.1f %10d %9d %12.1f %10.3f %18s" % (rname, 100 * m.mean(), len(XC.walk_tus(cus, modes, W, H)), launches, 1e3 / ms, ms,
                                                               "%.3f..%.3f" % (min(t[rname]), max(t[rname]))))
            if rname.endswith("_lossless"):
                nbytes = m.mean() * 1.5 * W * H * (1 + 1 + 2) + 22.0 * W * H / 16     # source, rec, coefficients; the map and the modes
                print("#   %s: %.2f MB moved, %.1f GB/s, fraction of the 8 TB/s HBM roofline %.4f" % (rname, nbytes / 1e6, nbytes / ms / 1e6,
                                                                                                    nbytes / ms / 1e6 / 8000))


def inter_recon_rows(L, st, dev, rounds, frames=64):
    """Motion compensation of whole pictures (kvz_hip_inter_recon_frame) against the chain of entries that could produce the same
    planes before it existed, on the same PU list, interleaved round by round, medians.  1080p pictures of a random quadtree
    (depths 0..3, every part mode, random quarter-pel vectors), `frames` of them stacked in one tall picture per launch (1088 rows
    apart, so that the LCU grid of every picture starts on a multiple of 64).  _p: one reference; _b: the same map bi-predicted from
    two.  Algorithmic bytes: 1.5 W H written + 1.5 W H read per reference."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inter_recon_cases as IC
    from kvazaar_amd import api
    W, H, PITCH = 1920, 1080, 1088
    TH = PITCH * frames
    g = torch.Generator(device=dev); g.manual_seed(7)
    planes = [[torch.randint(0, 256, (TH >> c, W >> c), dtype=torch.uint8, device=dev, generator=g) for c in (0, 1, 1)] for _ in range(2)]
    dest = [torch.empty((TH >> c, W >> c), dtype=torch.uint8, device=dev) for c in (0, 1, 1)]
    table = api.ref_picture_table([(p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), W, W // 2) for p in planes], W, TH)
    print("%-26s %10s %12s %10s %8s %8s" % ("kernel", "frames", "frames/s", "GB/s", "ms", "vs chain"))
    for name, n_refs in (("inter_recon_frame_p", 1), ("inter_recon_frame_b", 2)):
        one = np.zeros((PITCH // 4, W // 4), dtype=IC.CU_INFO)
        cus, ref_LX = IC.random_cu_map(W, H, 31, 1, False, intra_share=0.0, blank_share=0.0, bad_share=0.0, far=0.0)
        if n_refs == 2:                                                   # the same map, every PU from both lists
            rs = np.random.default_rng(32)
            cus["mv_dir"][cus["type"] == IC.CU_INTER] = 3
            cus["mv"][:, :, 1, :] = rs.integers(-160, 161, cus["mv"][:, :, 1, :].shape)
            ref_LX[1, 0] = 1
        one[:H // 4] = cus
        pus1 = IC.walk_pus(one, ref_LX, W, PITCH)
        pus = np.tile(pus1, frames)
        pus["y"] += np.repeat(np.arange(frames, dtype=np.int32) * PITCH, len(pus1))
        cus_d = torch.from_numpy(np.tile(one, (frames, 1)).view(np.uint8).copy()).to(dev)
        prm = np.zeros(1, dtype=api.INTER_RECON_PARAMS)
        prm["chroma"], prm["n_refs"], prm["ref_LX"] = 1, n_refs, ref_LX

        def fused():
            return L.kvz_hip_inter_recon_frame(dest[0].data_ptr(), W, dest[1].data_ptr(), dest[2].data_ptr(), W // 2, W, TH, cus_d.data_ptr(),
                                               table.ctypes.data, prm.ctypes.data, st)
        # the chain: per reference sample_luma_batch + 2 x sample_chroma_batch into compact blocks (14-bit for _b), then 3 x bipred_blend_batch
        area = pus["width"].astype(np.int64) * pus["height"]
        offs = [torch.from_numpy(np.concatenate([[0], np.cumsum(area >> (2 * c))[:-1]]).astype(np.int64)).to(dev) for c in (0, 1)]
        total = [int(area.sum()) >> (2 * c) for c in (0, 1)]
        blocks = []
        for lst in range(n_refs):
            per = []
            for c in (0, 1):
                b = np.zeros((len(pus), 6), dtype=np.int32)
                mv = pus["mv"][:, lst, :].astype(np.int32)
                b[:, 0], b[:, 1] = (pus["x"] >> c) + (mv[:, 0] >> (2 + c)), (pus["y"] >> c) + (mv[:, 1] >> (2 + c))
                b[:, 2], b[:, 3] = mv[:, 0] & (7 if c else 3), mv[:, 1] & (7 if c else 3)
                b[:, 4], b[:, 5] = pus["width"] >> c, pus["height"] >> c
                per.append(torch.from_numpy(b).to(dev))
            blocks.append(per)
        esz = 2 if n_refs == 2 else 1
        mid = [[torch.empty(total[1 if k else 0] * esz, dtype=torch.uint8, device=dev) for k in range(3)] for _ in range(n_refs)]
        out = [torch.empty(total[1 if k else 0], dtype=torch.uint8, device=dev) for k in range(3)]

        def chain():
            for lst in range(n_refs):
                for k in range(3):
                    c = 1 if k else 0
                    f = L.kvz_hip_sample_chroma_batch if k else L.kvz_hip_sample_luma_batch
                    rc = f(planes[lst][k].data_ptr(), W >> c, W >> c, TH >> c, blocks[lst][c].data_ptr(), offs[c].data_ptr(), len(pus),
                           int(n_refs == 2), mid[lst][k].data_ptr(), st)
                    if rc:
                        return rc
            if n_refs == 2:
                for k in range(3):
                    rc = L.kvz_hip_bipred_blend_batch(8 if k == 0 else 4, 4 if k == 0 else 2, 1, mid[0][k].data_ptr(), 1, mid[1][k].data_ptr(),
                                                      out[k].data_ptr(), total[1 if k else 0] // (32 if k == 0 else 8), st)
                    if rc:
                        return rc
            return 0
        torch.cuda.synchronize()
        t = {"fused": [], "chain": []}
        for _ in range(rounds):
            t["fused"].append(timed(L, st, lambda: _lib.check(fused(), name), iters=5, warm=1))
            t["chain"].append(timed(L, st, lambda: _lib.check(chain(), name + " chain"), iters=5, warm=1))
        ms, ms_chain = float(np.median(t["fused"])), float(np.median(t["chain"]))
        nbytes = 1.5 * W * H * frames * (1 + n_refs)
        print("%-26s %10d %12.1f %10.1f %8.4f %8.2f" % (name, frames, frames / ms * 1e3, nbytes / ms / 1e6, ms, ms_chain / ms))
        print("%-26s %10d %12.1f %10.1f %8.4f %8s" % (name + "(chain)", frames, frames / ms_chain * 1e3, nbytes / ms_chain / 1e6, ms_chain, "-"))
        print("#   %d PUs per picture; fraction of the 8 TB/s HBM roofline: fused %.3f, chain %.3f" % (len(pus1), nbytes / ms / 1e6 / 8000, nbytes / ms_chain / 1e6 / 8000))


def inter_residual_rows(L, st, dev, rounds, iters=6):
    """Residual coding of whole pictures (kvz_hip_inter_residual_frame: all-inter random quadtree with tr_depth as the search sets it and
    a share of deeper trees, 4:2:0, source = prediction + noise of one amplitude per CU) against kvz_hip_quantize_residual_batch over the
    SAME TU population laid out contiguously, one call per size and plane, summed: the same arithmetic without plane addressing and
    without the gather a caller would add -- a lower bound of what the picture cost before the entry existed.  Interleaved round by
    round in one process, medians.  The entry works in place, so every timed call gets a fresh copy of the prediction (copied outside
    the timed region).  At 1080p the same picture with a QP per LCU (kvz_hip_inter_residual_frame_qp, QPs 22..42 drawn per LCU) is timed
    in the same rounds, interleaved, and so is kvz_hip_inter_residual_frame_ts with one bit cost (transform skip: the 4x4 launch codes
    every luma TU twice), and so is kvz_hip_inter_residual_frame_lossless (one launch: source and prediction read, rec and coefficients
    written, the same 7.5 bytes per luma pixel).  Then the three-call chain prediction -> residual coding -> deblocking per 1080p picture.
    Algorithmic bytes: 5 per sample = 7.5 per luma pixel, + 20 per 16 luma pixels of map."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import inter_recon_cases as IC
    import inter_residual_cases as RC
    from patterns import deblock_params
    from kvazaar_amd import api
    print("%-28s %10s %12s %10s %8s %8s" % ("kernel", "TUs", "frames/s", "GB/s", "ms", "contig/ms"))
    for name, W, H in (("inter_residual_frame_1080p", 1920, 1080), ("inter_residual_frame_4k", 3840, 2160)):
        cus, ref_LX = RC.make_map(W, H, 41, intra_share=0.0, blank_share=0.0, bad_share=0.0, far=0.0, edge_cu=False)
        pred = RC.smooth_planes(W, H, 42)
        src = RC.make_source(pred, cus, 43)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
        src_d, master = [up(p) for p in src], [up(p) for p in pred]
        recs = [[torch.empty_like(m) for m in master] for _ in range(iters + 1)]
        cus_d = up(cus)
        shapes = api.coeff_shapes(W, H)
        co_d = [torch.empty(shapes[1 if k else 0], dtype=torch.int16, device=dev) for k in range(3)]
        cbf_d = torch.empty(cus.shape, dtype=torch.uint8, device=dev)
        cost_d = torch.empty(cus.shape + (6,), dtype=torch.int32, device=dev)
        table = api.ref_picture_table([(src_d[0].data_ptr(), src_d[1].data_ptr(), src_d[2].data_ptr(), W, W // 2)], W, H)
        prm = api.inter_residual_params(32, 0, 0, 1)
        turn = [0]

        def frame():
            r = recs[turn[0] % len(recs)]
            turn[0] += 1
            return L.kvz_hip_inter_residual_frame(table.ctypes.data, r[0].data_ptr(), W, r[1].data_ptr(), r[2].data_ptr(), W // 2, cus_d.data_ptr(),
                                                  co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(), cbf_d.data_ptr(), cost_d.data_ptr(),
                                                  prm.ctypes.data, st)
        lcu_qp_d = up(np.random.default_rng(44).integers(22, 43, api.lcu_count(W, H)).astype(np.int8))

        def frame_qp():
            r = recs[turn[0] % len(recs)]
            turn[0] += 1
            return L.kvz_hip_inter_residual_frame_qp(table.ctypes.data, r[0].data_ptr(), W, r[1].data_ptr(), r[2].data_ptr(), W // 2, cus_d.data_ptr(),
                                                     co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(), cbf_d.data_ptr(), cost_d.data_ptr(),
                                                     lcu_qp_d.data_ptr(), prm.ctypes.data, st)
        skip_d = torch.zeros(cus.shape, dtype=torch.uint8, device=dev)
        ts = _lib.TrSkip(58, 0, None)                   # (int)(lambda + 0.5) at QP 32

        def frame_ts():
            r = recs[turn[0] % len(recs)]
            turn[0] += 1
            return L.kvz_hip_inter_residual_frame_ts(table.ctypes.data, r[0].data_ptr(), W, r[1].data_ptr(), r[2].data_ptr(), W // 2, cus_d.data_ptr(),
                                                     co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(), cbf_d.data_ptr(), cost_d.data_ptr(),
                                                     None, None, C.byref(ts), skip_d.data_ptr(), prm.ctypes.data, st)
        ll = _lib.Lossless(1, 0, (0, 0))

        def frame_lossless():
            r = recs[turn[0] % len(recs)]
            turn[0] += 1
            return L.kvz_hip_inter_residual_frame_lossless(table.ctypes.data, r[0].data_ptr(), W, r[1].data_ptr(), r[2].data_ptr(), W // 2,
                                                           cus_d.data_ptr(), co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(), cbf_d.data_ptr(),
                                                           cost_d.data_ptr(), C.byref(ll), st)
        # the same TUs, contiguous, per (plane, size)
        groups = {}
        for t in RC.walk_tus(cus, W, H):
            groups.setdefault((t[0], t[3]), []).append(t)
        contig = []
        qp = _lib.QuantParams()
        qp.qp = 32
        for (p, n), lst in sorted(groups.items()):
            a = np.array(lst, dtype=np.int64)
            xs, ys = a[:, 1] >> (1 if p else 0), a[:, 2] >> (1 if p else 0)
            rb, pb = RC._blocks(src[p], xs, ys, n)[0], RC._blocks(pred[p], xs, ys, n)[0]
            rb_d, pb_d = up(rb), up(pb)
            contig.append((n, p, len(lst), rb_d, pb_d, torch.empty_like(pb_d), torch.empty(len(lst) * n * n, dtype=torch.int16, device=dev),
                           torch.empty(len(lst), dtype=torch.int32, device=dev)))

        def batches():
            for (n, p, count, rb_d, pb_d, rec_d, c_d, has_d) in contig:
                rc = L.kvz_hip_quantize_residual_batch(C.byref(qp), 0, n, p, 0, 0, rb_d.data_ptr(), pb_d.data_ptr(), rec_d.data_ptr(), c_d.data_ptr(),
                                                       has_d.data_ptr(), count, st)
                if rc:
                    return rc
            return 0

        def refresh():
            for r in recs:
                for d, m in zip(r, master):
                    d.copy_(m)
            torch.cuda.synchronize()
            turn[0] = 0
        t = {"frame": [], "contig": [], "lcu_qp": [], "ts": [], "lossless": []}
        for _ in range(rounds):
            refresh()
            t["frame"].append(timed(L, st, lambda: _lib.check(frame(), name), iters=iters - 1, warm=1))
            if W == 1920:
                refresh()
                t["lcu_qp"].append(timed(L, st, lambda: _lib.check(frame_qp(), name + "_lcu_qp"), iters=iters - 1, warm=1))
                refresh()
                t["ts"].append(timed(L, st, lambda: _lib.check(frame_ts(), name + "_ts"), iters=iters - 1, warm=1))
                refresh()
                t["lossless"].append(timed(L, st, lambda: _lib.check(frame_lossless(), name + "_lossless"), iters=iters - 1, warm=1))
            t["contig"].append(timed(L, st, lambda: _lib.check(batches(), name + " contiguous"), iters=iters - 1, warm=1))
        ms, ms_c = float(np.median(t["frame"])), float(np.median(t["contig"]))
        n_tus = sum(c[2] for c in contig)
        nbytes = 7.5 * W * H + 20.0 * W * H / 16
        print("%-28s %10d %12.1f %10.1f %8.4f %8.2f" % (name, n_tus, 1e3 / ms, nbytes / ms / 1e6, ms, ms_c / ms))
        print("%-28s %10d %12.1f %10.1f %8.4f %8s" % (name + "(contig)", n_tus, 1e3 / ms_c, 7.5 * W * H / ms_c / 1e6, ms_c, "-"))
        print("#   %s over the %d rounds: min..max %.4f..%.4f ms" % (name, rounds, min(t["frame"]), max(t["frame"])))
        if t["lcu_qp"]:
            ms_q = float(np.median(t["lcu_qp"]))
            print("%-28s %10d %12.1f %10.1f %8.4f %8s" % (name + "_lcu_qp", n_tus, 1e3 / ms_q, nbytes / ms_q / 1e6, ms_q, "-"))
            print("#   %s_lcu_qp over the %d rounds: min..max %.4f..%.4f ms" % (name, rounds, min(t["lcu_qp"]), max(t["lcu_qp"])))
            ms_t = float(np.median(t["ts"]))
            print("%-28s %10d %12.1f %10.1f %8.4f %8s" % (name + "_ts", n_tus, 1e3 / ms_t, nbytes / ms_t / 1e6, ms_t, "-"))
            print("#   %s_ts over the %d rounds: min..max %.4f..%.4f ms" % (name, rounds, min(t["ts"]), max(t["ts"])))
            ms_l = float(np.median(t["lossless"]))
            print("%-28s %10d %12.1f %10.1f %8.4f %8s" % (name + "_lossless", n_tus, 1e3 / ms_l, nbytes / ms_l / 1e6, ms_l, "-"))
            print("#   %s_lossless over the %d rounds: min..max %.4f..%.4f ms; %.2f MB moved, fraction of the 8 TB/s HBM roofline %.4f; 1 launch" %
                  (name, rounds, min(t["lossless"]), max(t["lossless"]), nbytes / 1e6, nbytes / ms_l / 1e6 / 8000))
        print("#   fraction of the 8 TB/s HBM roofline: frame %.3f, contiguous sum %.3f; %d launches against %d" %
              (nbytes / ms / 1e6 / 8000, 7.5 * W * H / ms_c / 1e6 / 8000, 5, len(contig)))
        if W != 1920:
            continue
        # the chain on one stream: kvz_hip_inter_recon_frame -> kvz_hip_inter_residual_frame -> kvz_hip_deblock_frame
        g = torch.Generator(device=dev); g.manual_seed(9)
        ref = [torch.randint(0, 256, (H >> c, W >> c), dtype=torch.uint8, device=dev, generator=g) for c in (0, 1, 1)]
        rtab = api.ref_picture_table([(ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), W, W // 2)], W, H)
        rprm = np.zeros(1, dtype=api.INTER_RECON_PARAMS)
        rprm["chroma"], rprm["n_refs"], rprm["ref_LX"] = 1, 1, ref_LX
        dprm = deblock_params(qp=32)
        dprm["ref_LX"] = ref_LX
        r = recs[0]

        def chain():
            rc = L.kvz_hip_inter_recon_frame(r[0].data_ptr(), W, r[1].data_ptr(), r[2].data_ptr(), W // 2, W, H, cus_d.data_ptr(), rtab.ctypes.data,
                                             rprm.ctypes.data, st)
            rc = rc or L.kvz_hip_inter_residual_frame(table.ctypes.data, r[0].data_ptr(), W, r[1].data_ptr(), r[2].data_ptr(), W // 2, cus_d.data_ptr(),
                                                      co_d[0].data_ptr(), co_d[1].data_ptr(), co_d[2].data_ptr(), cbf_d.data_ptr(), cost_d.data_ptr(),
                                                      prm.ctypes.data, st)
            return rc or L.kvz_hip_deblock_frame(r[0].data_ptr(), W, r[1].data_ptr(), r[2].data_ptr(), W // 2, W, H, cus_d.data_ptr(), dprm.ctypes.data, st)
        torch.cuda.synchronize()
        tc = [timed(L, st, lambda: _lib.check(chain(), "chain"), iters=5, warm=1) for _ in range(rounds)]
        print("%-28s %10s %12.1f %10s %8.4f %8s" % ("recon+residual+deblock_1080p", "-", 1e3 / float(np.median(tc)), "-", float(np.median(tc)), "-"))


def sao_frame_rows(L, st, dev, rounds, iters=20):
    """SAO of a whole 1080p 4:2:0 picture (kvz_hip_sao_stats_frame, kvz_hip_sao_frame) against the way the block-list entries offer:
    statistics -- every LCU block of the three planes of source and reconstruction blitted contiguously with kvz_hip_copy_rects_batch
    (16 rectangles per call), then kvz_hip_sao_edge_stats / edge_ddistortion / band_stats / band_ddistortion_batch per plane and block
    shape (the last LCU row of 1080p is 56 high); reconstruction -- a copy of each plane and one kvz_hip_sao_reconstruct_color_batch per
    plane over host-trimmed rectangles.  Old and new interleaved round by round in one process; median and min..max over the rounds.
    Algorithmic bytes: statistics read source + reconstruction (3 per luma pixel), reconstruction reads and writes the picture (3)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sao_frame_cases as SC
    from patterns import sao_records
    from kvazaar_amd import api
    W, H = 1920, 1080
    g = torch.Generator(device=dev); g.manual_seed(17)
    src = [torch.randint(0, 256, (H >> c, W >> c), dtype=torch.uint8, device=dev, generator=g) for c in (0, 1, 1)]
    rec = [(p.to(torch.int16) + torch.randint(-8, 9, p.shape, dtype=torch.int16, device=dev, generator=g)).clamp_(0, 255).to(torch.uint8) for p in src]
    dst = [torch.empty_like(p) for p in rec]
    n_lcu = api.lcu_count(W, H)
    table = api.ref_picture_table([(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), W, W // 2)], W, H)
    stats = torch.empty(3 * n_lcu * 104, dtype=torch.int32, device=dev)
    cands = torch.empty(3 * n_lcu * 30, dtype=torch.int32, device=dev)
    luma, chro = sao_records(n_lcu, 5), sao_records(n_lcu, 6)
    luma_d, chro_d = torch.from_numpy(luma).to(dev), torch.from_numpy(chro).to(dev)

    def new_stats():
        return L.kvz_hip_sao_stats_frame(table.ctypes.data, rec[0].data_ptr(), W, rec[1].data_ptr(), rec[2].data_ptr(), W // 2, 1, stats.data_ptr(),
                                         cands.data_ptr(), st)

    def new_frame():
        return L.kvz_hip_sao_frame(rec[0].data_ptr(), W, rec[1].data_ptr(), rec[2].data_ptr(), W // 2, dst[0].data_ptr(), W, dst[1].data_ptr(),
                                   dst[2].data_ptr(), W // 2, W, H, luma_d.data_ptr(), chro_d.data_ptr(), 1, st)
    grid = api.uniform_tile_grid(W, H, 4, 2)

    def new_frame_tiles():
        return L.kvz_hip_sao_frame_tiles(rec[0].data_ptr(), W, rec[1].data_ptr(), rec[2].data_ptr(), W // 2, dst[0].data_ptr(), W, dst[1].data_ptr(),
                                         dst[2].data_ptr(), W // 2, W, H, luma_d.data_ptr(), chro_d.data_ptr(), 1, grid.ctypes.data, st)
    # ---- the block-list way ----
    blit, groups, keep = [], [], []
    for color in range(3):
        blocks = SC.lcu_blocks(W, H, color)
        stride = W >> (1 if color else 0)
        for shape in sorted({b[2:] for b in blocks}):
            idx = [i for i, b in enumerate(blocks) if b[2:] == shape]
            bw, bh = shape
            o_d = torch.empty(len(idx) * bw * bh, dtype=torch.uint8, device=dev)
            r_d = torch.empty_like(o_d)
            for plane, out in ((src[color], o_d), (rec[color], r_d)):
                for k, i in enumerate(idx):
                    x, y = blocks[i][:2]
                    blit.append((plane.data_ptr() + y * stride + x, out.data_ptr() + k * bw * bh, stride, bw, bw, bh))
            out = [torch.empty(len(idx) * n, dtype=torch.int32, device=dev) for n in (40, 4, 64, 1)]
            offs = torch.ones(len(idx) * 20, dtype=torch.int32, device=dev)
            bpos = torch.zeros(len(idx), dtype=torch.int32, device=dev)
            bands = torch.ones(len(idx) * 4, dtype=torch.int32, device=dev)
            keep += [o_d, r_d, out, offs, bpos, bands]
            groups.append((bw, bh, len(idx), o_d, r_d, out, offs, bpos, bands))
    rects = (_lib.RectCopy * len(blit))(*[_lib.RectCopy(*b) for b in blit])
    chunks = [(C.byref(rects, i * C.sizeof(_lib.RectCopy)), min(_lib.MAX_RECTS, len(blit) - i)) for i in range(0, len(blit), _lib.MAX_RECTS)]

    def old_stats():
        for ptr, n in chunks:
            rc = L.kvz_hip_copy_rects_batch(ptr, n, st)
            if rc:
                return rc
        for (bw, bh, n, o_d, r_d, out, offs, bpos, bands) in groups:
            rc = (L.kvz_hip_sao_edge_stats_batch(o_d.data_ptr(), r_d.data_ptr(), bw, bh, n, out[0].data_ptr(), st) or
                  L.kvz_hip_sao_edge_ddistortion_batch(o_d.data_ptr(), r_d.data_ptr(), bw, bh, n, offs.data_ptr(), out[1].data_ptr(), st) or
                  L.kvz_hip_sao_band_stats_batch(o_d.data_ptr(), r_d.data_ptr(), bw, bh, n, out[2].data_ptr(), st) or
                  L.kvz_hip_sao_band_ddistortion_batch(o_d.data_ptr(), r_d.data_ptr(), bw, bh, n, bpos.data_ptr(), bands.data_ptr(), out[3].data_ptr(), st))
            if rc:
                return rc
        return 0
    trimmed = []
    for color in range(3):
        infos = luma if color == 0 else chro
        ph, pw = H >> (1 if color else 0), W >> (1 if color else 0)
        r = []
        for i, (x, y, bw, bh) in enumerate(SC.lcu_blocks(W, H, color)):
            if infos[i][0] == 2:
                x, y, bw, bh = SC.trim(x, y, bw, bh, int(infos[i][1]), pw, ph)
            r.append((x, y, bw, bh, i))
        trimmed.append(torch.from_numpy(np.array(r, dtype=np.int32)).to(dev))

    def old_frame():
        for color in range(3):
            ph, pw = H >> (1 if color else 0), W >> (1 if color else 0)
            rc = (L.kvz_hip_memcpy_d2d(dst[color].data_ptr(), rec[color].data_ptr(), pw * ph, st) or
                  L.kvz_hip_sao_reconstruct_color_batch(rec[color].data_ptr(), pw, pw, ph, dst[color].data_ptr(), pw, trimmed[color].data_ptr(), n_lcu,
                                                        (luma_d if color == 0 else chro_d).data_ptr(), n_lcu, color, st))
            if rc:
                return rc
        return 0
    torch.cuda.synchronize()
    # what both ways compute is the same
    _lib.check(new_frame(), "sao_frame")
    _lib.check(L.kvz_hip_stream_sync(st), "sync")
    want = [d.clone() for d in dst]
    _lib.check(old_frame(), "block-list reconstruction")
    _lib.check(L.kvz_hip_stream_sync(st), "sync")
    assert all(torch.equal(a, b) for a, b in zip(want, dst)), "sao_frame differs from the block-list reconstruction"
    t = {k: [] for k in ("new_stats", "old_stats", "new_frame", "old_frame", "new_frame_tiles")}
    fns = {"new_stats": new_stats, "old_stats": old_stats, "new_frame": new_frame, "old_frame": old_frame, "new_frame_tiles": new_frame_tiles}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(L, st, lambda fn=fn, k=k: _lib.check(fn(), k), iters=iters, warm=3))
    print("%-28s %10s %12s %10s %8s %16s %8s" % ("kernel", "launches", "frames/s", "GB/s", "ms", "min..max ms", "old/new"))
    nbytes = 3.0 * W * H
    for new, old, name, n_new, n_old in (("new_stats", "old_stats", "sao_stats_frame_1080p", 1, len(chunks) + 4 * len(groups)),
                                         ("new_frame", "old_frame", "sao_frame_1080p", 1, 6)):
        ms, ms_o = float(np.median(t[new])), float(np.median(t[old]))
        print("%-28s %10d %12.1f %10.1f %8.4f %7.4f..%7.4f %8.2f" % (name, n_new, 1e3 / ms, nbytes / ms / 1e6, ms, min(t[new]), max(t[new]), ms_o / ms))
        print("%-28s %10d %12.1f %10.1f %8.4f %7.4f..%7.4f %8s" % (name + "(blocks)", n_old, 1e3 / ms_o, nbytes / ms_o / 1e6, ms_o, min(t[old]), max(t[old]), "-"))
    ms = float(np.median(t["new_frame_tiles"]))                  # 4 x 2 uniform tiles, in the same rounds as the untiled row
    print("%-28s %10d %12.1f %10.1f %8.4f %7.4f..%7.4f %8s" % ("sao_frame_1080p_tiles4x2", 1, 1e3 / ms, nbytes / ms / 1e6, ms, min(t["new_frame_tiles"]),
                                                             max(t["new_frame_tiles"]), "-"))


if __name__ == "__main__":
    main()
