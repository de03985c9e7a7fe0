"""CPU: the four tile entries of the picture chain are declared, exported and bound with the signatures of their untiled counterparts
plus the grid; kvz_hip_tile_grid and kvz_hip_cu_qp_tiles_params have the documented layout in C, in ctypes and in numpy; the numpy
conveniences take tiles=; the ABI version is unchanged; without a device the entries refuse."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import test_abi as A

ENTRIES = {"kvz_hip_intra_recon_frame_tiles": ("kvz_hip_intra_recon_frame_qp", -2), "kvz_hip_cu_qp_frame_tiles": ("kvz_hip_cu_qp_frame", -2),
           "kvz_hip_deblock_frame_tiles": ("kvz_hip_deblock_frame", -2), "kvz_hip_sao_frame_tiles": ("kvz_hip_sao_frame", -1)}


def _lib():
    if not os.path.exists(A.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(A.LIB)


def test_header_declares_and_library_exports_the_four_entries():
    L = _lib()
    from kvazaar_amd import _lib as B
    src = re.sub(r"/\*.*?\*/", "", open(A.HEADER).read(), flags=re.S)
    for name, (old, at) in ENTRIES.items():
        assert name in A.declared_symbols() and hasattr(L, name) and hasattr(B.load(), name)
        # the untiled entry's arguments with the grid before params where there is one, else before the stream
        res, args = B.SIGNATURES[name]
        was = B.SIGNATURES[old][1]
        assert res is ctypes.c_int and args == was[:at] + [ctypes.c_void_p] + was[at:]
        decl = re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % name, src).group(1)
        params = [p.strip() for p in decl.split(",")]
        assert params[at - 1] == "const kvz_hip_tile_grid *grid" and params[-1] == "kvz_hip_stream s"
        old_params = [p.strip() for p in re.search(r"KVZ_HIP_API int %s\(([^;]*)\);" % old, src).group(1).split(",")]
        rest = params[:at - 1] + params[at:]
        if name == "kvz_hip_cu_qp_frame_tiles":
            old_params[-2] = old_params[-2].replace("kvz_hip_cu_qp_params", "kvz_hip_cu_qp_tiles_params")
        assert rest == old_params, name


def test_struct_layouts_in_c_ctypes_and_numpy(tmp_path):
    from kvazaar_amd import _lib as B, api
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kvz_hip.h"', 'int main(void) {',
             '  printf("%d %zu %zu\\n", KVZ_HIP_MAX_TILES_PER_DIM, sizeof(kvz_hip_tile_grid), sizeof(kvz_hip_cu_qp_tiles_params));',
             '  printf("%zu %zu %zu %zu\\n", offsetof(kvz_hip_tile_grid, cols), offsetof(kvz_hip_tile_grid, rows), offsetof(kvz_hip_tile_grid, col_bd),'
             ' offsetof(kvz_hip_tile_grid, row_bd));',
             '  printf("%zu %zu %d\\n", offsetof(kvz_hip_cu_qp_tiles_params, start_qp), offsetof(kvz_hip_cu_qp_tiles_params, chain_rows), KVZ_HIP_ABI_VERSION);',
             '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(A.ROOT, "include"), str(src), "-o", str(exe)])
    out = [[int(v) for v in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert out == [[48, 392, 8], [0, 4, 8, 200], [0, 4, 4]]
    assert ctypes.sizeof(B.TileGrid) == 392 and ctypes.sizeof(B.CuQpTilesParams) == 8 and B.MAX_TILES_PER_DIM == 48
    assert [getattr(B.TileGrid, f).offset for f in ("cols", "rows", "col_bd", "row_bd")] == [0, 4, 8, 200]
    assert api.TILE_GRID.itemsize == 392 and [api.TILE_GRID.fields[f][1] for f in api.TILE_GRID.names] == [0, 4, 8, 200]
    assert api.TILE_GRID.names == ("cols", "rows", "col_bd", "row_bd")
    assert api.CU_QP_TILES_PARAMS.itemsize == 8 and api.CU_QP_TILES_PARAMS.names == ("start_qp", "chain_rows")


def test_numpy_conveniences_take_tiles_and_default_to_the_untiled_entries():
    from kvazaar_amd import api
    for f in (api.intra_recon_frame, api.deblock_frame, api.sao_frame):
        assert inspect.signature(f).parameters["tiles"].default is None
    # the QP map's convenience keeps the parameter list that tests/test_lcu_qp_abi.py pins; its tiled form is a function of its own
    assert list(inspect.signature(api.cu_qp_frame_tiles).parameters) == ["cus", "cbf", "lcu_qp", "start_qp", "tiles", "chain_rows"]
    assert inspect.signature(api.cu_qp_frame_tiles).parameters["chain_rows"].default == 0
    assert callable(api.tile_grid) and callable(api.uniform_tile_grid)
    with pytest.raises(ValueError):
        api.tile_grid(64 * 60, 64, list(range(49)), [0, 1])


def test_abi_version_is_still_4():
    L = _lib()
    L.kvz_hip_abi_version.restype = ctypes.c_int
    assert L.kvz_hip_abi_version() == 4


def test_without_a_device_the_entries_return_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from kvazaar_amd import _lib as B
    L = B.load()
    no_device = int(re.search(r"KVZ_HIP_ERR_NO_DEVICE\s*=?\s*(-?\d+)", open(A.HEADER).read()).group(1))
    for name in ENTRIES:
        n = len(B.SIGNATURES[name][1])
        args = [None if t is ctypes.c_void_p else 0 for t in B.SIGNATURES[name][1]]
        assert len(args) == n and getattr(L, name)(*args) == no_device, name
