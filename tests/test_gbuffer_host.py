"""The host side of the G-buffer pass (include/dsrt.h, dsrt_render_gbuffer): the PFM writer, the binding's struct, argument checks that need
no device, and the CLI's flag.  No GPU involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _read_pfm(path):
    """-> (image in image order, top row first, as float32 (H, W) or (H, W, 3); the header's type line; scale)"""
    raw = open(path, "rb").read()
    lines, pos = [], 0
    for _ in range(3):
        end = raw.index(b"\n", pos)
        lines.append(raw[pos:end].decode())
        pos = end + 1
    kind = lines[0]
    w, h = (int(v) for v in lines[1].split())
    scale = float(lines[2])
    ch = 3 if kind == "PF" else 1
    data = np.frombuffer(raw[pos:], "<f4" if scale < 0 else ">f4")
    assert data.size == w * h * ch
    img = data.reshape((h, w, ch) if ch == 3 else (h, w))[::-1]          # the file holds the bottom row first
    return img.astype(np.float32), kind, scale


@pytest.mark.parametrize("shape", [(5, 7), (3, 11, 3), (1, 1), (2, 9, 3)])
def test_pfm_writer_round_trip(dsrt, tmp_path, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.standard_normal(shape).astype(np.float32)
    img.flat[0] = np.inf                                                   # the G-buffer's miss value survives the trip
    img.flat[-1] = -0.0
    path = tmp_path / "x.pfm"
    dsrt.write_pfm(path, img)
    got, kind, scale = _read_pfm(path)
    assert kind == ("PF" if len(shape) == 3 else "Pf") and scale == -1.0
    assert got.shape == img.shape
    assert np.array_equal(got.view(np.uint32), img.view(np.uint32))
    # rows are stored bottom-up: the first row in the file is the image's last
    raw = open(path, "rb").read()
    row_bytes = img.shape[1] * (3 if len(shape) == 3 else 1) * 4
    assert raw[-row_bytes * img.shape[0]:][:row_bytes] == img[-1].astype("<f4").tobytes()


def test_pfm_writer_refuses_bad_arguments(dsrt, tmp_path):
    img = np.zeros((4, 4), np.float32)
    lib = dsrt.lib
    assert lib.dsrt_write_pfm(str(tmp_path / "a.pfm").encode(), img.ctypes.data, 4, 4, 2) == -1        # 1 or 3 channels only
    assert lib.dsrt_write_pfm(str(tmp_path / "a.pfm").encode(), img.ctypes.data, 0, 4, 1) == -1
    assert lib.dsrt_write_pfm(str(tmp_path / "a.pfm").encode(), None, 4, 4, 1) == -1
    assert lib.dsrt_write_pfm(str(tmp_path / "no_such_dir" / "a.pfm").encode(), img.ctypes.data, 4, 4, 1) == -2


def test_gbuffer_struct_matches_the_library(dsrt):
    from dsrt_amd import capi
    assert dsrt.lib.dsrt_sizeof(6) == C.sizeof(capi.DsrtGBuffer) == 11 * C.sizeof(C.c_void_p)
    assert [n for n, _ in capi.DsrtGBuffer._fields_] == list(capi.GBUFFER_CHANNELS)
    assert capi.ABI_VERSION == dsrt.lib.dsrt_abi_version() == 8
    for name in ("dsrt_render_gbuffer", "dsrt_render_gbuffer_to_host", "dsrt_write_pfm"):
        assert name in capi.EXPORTS and hasattr(dsrt.lib, name)


def test_gbuffer_on_a_null_context_is_invalid(dsrt):
    from dsrt_amd import capi
    desc = dsrt.make_desc(16, 16, 1)
    gb = capi.DsrtGBuffer()
    assert dsrt.lib.dsrt_render_gbuffer(None, C.byref(desc), C.byref(gb), None, None) == -1
    assert dsrt.lib.dsrt_render_gbuffer_to_host(None, C.byref(desc), C.byref(gb), None) == -1
    assert b"null" in dsrt.lib.dsrt_last_error()


def test_cli_usage_names_gbuffer():
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    assert os.path.exists(exe), "build the CLI with `make tools`"
    r = subprocess.run([exe, "--no-such-flag"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "usage:" in r.stderr and "[--gbuffer]" in r.stderr
