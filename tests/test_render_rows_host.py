"""The three original render entry points without a GPU — rtx_render_rows, rtx_render_tiles_device, rtx_render_frame: every
argument check that needs no device, in the order the library makes them, on the 16 x 12 scene of test_view_rows_host.py.
Device 99 is none on any machine, so RTX_ERR_NO_DEVICE marks a call that passed its argument checks."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 16, 12


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def scene(rtx, samples_half):
    tris, rgb = rtx.default_primitives([os.path.join(ROOT, "models", "bunny.obj")])
    with rtx.Scene(W, H, tris, rgb, samples_half[:64], tie_rank=None, eye=(3.0, 90.0, 210.0), look_at=(1.0, 20.0, -7.0),
                   up=(0.1, 1.0, 0.0), distance=40.0) as s:
        yield s


def test_render_rows_argument_checks_need_no_device(rtx, scene):
    L, h = rtx.rtx._lib, scene.handle
    BAD, NO_DEVICE = rtx.ERR_BAD_ARG, rtx.ERR_NO_DEVICE
    rgb = np.full(W * H * 3, 7, np.uint8)
    st = rtx.rtx.Stats()

    def rows(row0, nrows, handle=h, device=0, out=rgb.ctypes.data, stats=None):
        return L.rtx_render_rows(handle, device, row0, nrows, out, stats)

    assert rows(0, H, handle=None) == BAD and rows(0, H, out=None) == BAD
    assert rows(H + 1, 0) == BAD and rows(4, H - 3) == BAD
    # the arguments come first: a bad range on a device that does not exist is a bad argument
    assert rows(H + 1, 0, device=99) == BAD and rows(4, H - 3, device=-1) == BAD
    for device in (99, -1):
        assert rows(0, H, device=device) == NO_DEVICE and rows(4, H - 4, device=device, stats=C.byref(st)) == NO_DEVICE
    # this family looks for its device before it answers an empty call (the view families answer first)
    assert rows(0, 0, device=99) == NO_DEVICE and rows(H, 0, device=99, stats=C.byref(st)) == NO_DEVICE
    if rtx.device_count() == 0:
        assert rows(0, H) == NO_DEVICE and rows(0, 0) == NO_DEVICE
        with pytest.raises(rtx.RtxError) as e:
            scene.render_rows(0, H, device=0)
        assert e.value.code == NO_DEVICE
    assert (rgb == 7).all()


def test_render_tiles_device_argument_checks_need_no_device(rtx, scene):
    L, h = rtx.rtx._lib, scene.handle
    BAD, NO_DEVICE = rtx.ERR_BAD_ARG, rtx.ERR_NO_DEVICE

    def tiles(first_tile, tile_stride, tile_rows, handle=h, device=99, d_out=256, d_bytes=1 << 40):
        return L.rtx_render_tiles_device(handle, device, first_tile, tile_stride, tile_rows, d_out, d_bytes, None, None)

    assert tiles(0, 1, 8, handle=None) == BAD and tiles(0, 1, 8, d_out=None) == BAD
    assert tiles(0, 1, 0) == BAD and tiles(0, 0, 8) == BAD
    # the buffer holds the share's rows: rtx_tiles_bytes of them at least
    for share in ((0, 1, 8), (1, 2, 5), (0, 3, 1), (1, 1, 8)):
        need = scene.tiles_bytes(*share)
        assert need == L.rtx_tiles_rows(h, *share) * W * 3 and need > 0
        assert tiles(*share, d_bytes=need - 1) == BAD and tiles(*share, d_bytes=need) == NO_DEVICE
    # first row and stride of a share are 32-bit row numbers
    assert tiles(1 << 30, 1, 8) == BAD and tiles(1 << 30, 1, 8, d_bytes=0) == BAD
    assert tiles(0, 1 << 30, 8) == BAD
    assert tiles(1 << 30, 1, 3) == NO_DEVICE and tiles(0, 1 << 30, 3) == NO_DEVICE          # (3 * 2^30 < 2^32)
    # everything else gets as far as looking for its device — a share without rows included
    assert tiles(0, 1, 8) == NO_DEVICE and tiles(0, 1, 8, device=-1) == NO_DEVICE
    assert scene.tiles_bytes(2, 1, 8) == 0 and tiles(2, 1, 8, d_bytes=0) == NO_DEVICE
    assert tiles(H, 4, 1, d_bytes=0) == NO_DEVICE
    if rtx.device_count() == 0:
        assert tiles(0, 1, 8, device=0) == NO_DEVICE


def test_render_frame_argument_checks_need_no_device(rtx, scene):
    L, h = rtx.rtx._lib, scene.handle
    BAD, NO_DEVICE = rtx.ERR_BAD_ARG, rtx.ERR_NO_DEVICE
    rgb = np.full(W * H * 3, 7, np.uint8)
    st = rtx.rtx.Stats()

    def frame(devices, n_devices, tile_rows, handle=h, out=rgb.ctypes.data, stats=None):
        devs = (C.c_int * len(devices))(*devices) if devices is not None else None
        return L.rtx_render_frame(handle, devs, n_devices, tile_rows, out, stats)

    assert frame([0], 1, 8, handle=None) == BAD and frame(None, 1, 8) == BAD
    assert frame([0], 0, 8) == BAD and frame([0], -1, 8) == BAD
    assert frame([0], 1, 0) == BAD and frame([0], 1, 8, out=None) == BAD
    # stride of a share = n_devices * tile_rows rows: a 32-bit row number
    assert frame([0, 0], 2, 0x80000000) == BAD and frame([99, 99], 2, 0x80000000) == BAD
    assert frame([99, 99], 2, 0x7FFFFFFF) == NO_DEVICE
    assert frame([99], 1, 8) == NO_DEVICE and frame([99], 1, 8, stats=C.byref(st)) == NO_DEVICE
    assert frame([-1], 1, 8) == NO_DEVICE and frame([99, 99, 99], 3, 1) == NO_DEVICE
    if rtx.device_count() == 0:
        assert frame([0], 1, 8) == NO_DEVICE
        with pytest.raises(rtx.RtxError) as e:
            scene.render_frame([0], tile_rows=8)
        assert e.value.code == NO_DEVICE
    assert (rgb == 7).all()
