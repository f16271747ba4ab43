"""The oracle's rng_mode 1 (oracle/dsrt_oracle.c, dsrt_oracle_render_rect) on its own, on the CPU: its generator against rocRAND's own host
engine, its quantisation edges, its determinism, its statistics against the oracle's mode 0, and its pixel rectangles against whole rows.
The GPU kernel is compared with it in tests/test_gpu_rng_mode1.py; the contract both follow is written out in include/dsrt.h
(DsrtRenderDesc.rng_mode)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_world
from test_oracle import CASES, SUN
from _oracle_mode1 import RectOracle

ROCRAND_HEADER = "/opt/rocm/include/rocrand/rocrand_philox4x32_10.h"

# rocrand_init(seed, sub, offset) followed by n calls of rocrand(), printed as raw little-endian words
_DRIVER = r"""
#include <rocrand/rocrand_philox4x32_10.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const unsigned long long seed = std::strtoull(argv[1], nullptr, 0), sub = std::strtoull(argv[2], nullptr, 0), off = std::strtoull(argv[3], nullptr, 0);
    const int n = std::atoi(argv[4]);
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, sub, off, &st);
    std::vector<unsigned int> w((size_t)n);
    for (int i = 0; i < n; ++i) w[(size_t)i] = rocrand(&st);
    return std::fwrite(w.data(), 4, w.size(), stdout) == w.size() ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def rect(dsrt):
    return RectOracle()


@pytest.fixture(scope="module")
def rocrand_host(tmp_path_factory):
    if not os.path.exists(ROCRAND_HEADER) or shutil.which("g++") is None:
        pytest.skip("rocRAND's Philox header or g++ not on this machine")
    d = tmp_path_factory.mktemp("rocrand_host")
    (d / "drv.cpp").write_text(_DRIVER)
    exe = d / "drv"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", str(d / "drv.cpp"), "-o", str(exe)], check=True)

    def words(seed, sub, first, n):
        out = subprocess.run([str(exe), str(seed), str(sub), str(first), str(n)], check=True, capture_output=True).stdout
        return np.frombuffer(out, np.uint32)
    return words


def test_philox_known_answer(rect):
    # Random123's known answer for Philox4x32-10, counter 0, key 0 -- what rocRAND returns for seed 0, sub-sequence 0
    assert rect.philox_words(0, 0, 0, 4).tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


@pytest.mark.parametrize("seed, sub, first", [
    (0, 0, 0),
    (1337, 0, 0),
    (0xDEADBEEFDEADBEEF, 0, 3),                      # a nonzero high word of the key; an offset inside a block
    (0x00000001_00000000, 7, 0),                     # the key's high word alone
    (1337, (1 << 32) - 1, 5),
    (1337, 1 << 32, 1),                              # sub-sequences at and above 2^32: the counter's third and fourth words
    (0xDEADBEEFDEADBEEF, (1 << 32) + 12345, 6),
    (0xFFFFFFFF_FFFFFFFF, 1 << 63, 2),               # 2^63
    (42, (1 << 64) - 1, (1 << 34) + 1),              # an offset beyond 32-bit block numbers
])
def test_philox_equals_rocrand_host_engine(rect, rocrand_host, seed, sub, first):
    n = 4096
    want = rocrand_host(seed, sub, first, n)
    got = rect.philox_words(seed, sub, first, n)
    assert want.shape == (n,)
    assert np.array_equal(got, want), (hex(seed), hex(sub), first, int((got != want).sum()))


def test_philox_distinguishes_every_part_of_its_input(rect):
    base = rect.philox_words(0xDEADBEEFDEADBEEF, (1 << 32) + 3, 0, 16)
    for seed, sub in ((0xDEADBEEF, (1 << 32) + 3), (0xDEADBEEFDEADBEEF, 3), (0xDEADBEEFDEADBEEF ^ (1 << 40), (1 << 32) + 3)):
        assert not np.array_equal(rect.philox_words(seed, sub, 0, 16), base)
    assert np.array_equal(rect.philox_words(0xDEADBEEFDEADBEEF, (1 << 32) + 3, 5, 11), base[5:])


def test_quantisation_and_mean_edges(rect):
    one = 1 << 20
    assert rect.quantize(1.0) == one                                  # a sample that clamps to 1 is exactly 2^20
    assert rect.quantize(0.0) == 0
    assert rect.quantize(0.5 / one) == 1                              # half a unit rounds up
    # the + 0.5f is an fp32 addition: one ulp below half a unit the sum 1 - 2^-25 is a tie and rounds (to even) up to 1.0; two ulps below it is 1 - 2^-24
    below = np.nextafter(np.float32(0.5 / one), np.float32(0))
    assert rect.quantize(float(below)) == 1
    assert rect.quantize(float(np.nextafter(below, np.float32(0)))) == 0
    assert rect.quantize(1.5 / one) == 2 and rect.quantize(2.5 / one) == 3
    assert rect.quantize(0.75) == 786432
    # the largest value below 1: fp32's c * 2^20 + 0.5f rounds to 2^20 there
    assert rect.quantize(float(np.nextafter(np.float32(1.0), np.float32(0)))) == one
    # the mean: in double, then one conversion to float
    for s, spp in ((one * 7, 7), (0, 1), (one * 4095 * 3 + 1, 4095 * 3), (2**40 + 3, 5000), (123456789, 13)):
        assert rect.mean(s, spp) == np.float32(np.float64(s) * (1.0 / 1048576.0 / spp)), (s, spp)
    assert rect.mean(one * 5000, 5000) == 1.0
    assert rect.mean(2**32 * 3 + 7, 4096) != rect.mean(7, 4096)       # the high word of a 64-bit sum counts


def _scene(dsrt, name, spp=None, seed=None):
    world, cam_args, spp0 = CASES[name]
    spp = spp0 if spp is None else spp
    hs = load_world(dsrt, world)
    W, H = cam_args[3], cam_args[4]
    cam = dsrt.camera_look_at(cam_args[0], cam_args[1], cam_args[2], W, H, spp, cam_args[5])
    scene = hs.view(cam, SUN)
    if seed is not None:
        scene.seed = seed
    return hs, scene, W, H, spp


def test_mode1_image_is_deterministic_and_seed_determined(dsrt, rect):
    hs, scene, W, H, spp = _scene(dsrt, "lights", seed=0xDEADBEEF00000539)
    a, a32, ca = rect.render(scene, W, H)
    b, b32, cb = rect.render(scene, W, H, threads=3)
    assert np.array_equal(a, b) and np.array_equal(a32.view(np.uint32), b32.view(np.uint32)) and ca == cb
    assert ca["samples"] == W * H * spp and a.max() > 0
    scene.seed = 0x0000000000000539                                   # only the key's high word changed: a different image
    c, _, _ = rect.render(scene, W, H)
    assert not np.array_equal(a, c)


def test_light_that_fills_the_view_quantises_to_exactly_one(dsrt, rect):
    # every sample of every pixel is an emissive hit with radiance > 1: clamped to 1, 2^20 per sample, mean exactly 1.0, byte 255
    sph, mats = _big_light(dsrt)
    hs = dsrt.HostScene().add_arrays(spheres=sph, mats=mats)
    hs.build_bvh()
    cam = dsrt.camera_look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 10.0, 8, 6, 37, 4)
    scene = hs.view(cam, SUN)
    rgb, f32, cnt = rect.render(scene, 8, 6)
    assert cnt["samples"] == 8 * 6 * 37
    assert (f32 == 1.0).all() and (rgb == 255).all()


def _big_light(dsrt):
    capi = dsrt.capi
    sph = np.zeros(1, capi.SPHERE_DTYPE)
    sph["center"] = (0.0, 0.0, 0.0)
    sph["radius"] = 50.0
    sph["material_id"] = 0
    mats = np.zeros(1, capi.MAT_DTYPE)
    mats["type"] = 3
    mats["emissive"] = (4.0, 2.0, 7.0)
    mats["albedo_tex"] = -1
    return sph, mats


@pytest.mark.parametrize("name", ["station_near", "lights", "c1_spheres"])
def test_mode1_is_statistically_mode0(dsrt, rect, name):
    """rng_mode 1 is not the reference's stream, so not its bytes, but the same picture: no bias, and pixel differences at the noise level."""
    hs, scene, W, H, spp = _scene(dsrt, name, spp=64, seed=1337)
    _, f0, _ = rect.render(scene, W, H, rng_mode=0)
    m1, f1, c1 = rect.render(scene, W, H, rng_mode=1)
    assert c1["samples"] == W * H * spp
    d = f1.astype(np.float64) - f0.astype(np.float64)
    assert abs(d.mean()) < 2e-3, d.mean()
    assert np.abs(d).mean() < 0.04, np.abs(d).mean()
    assert (d != 0).mean() > 0.05                                     # ... and it is a different stream


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_rect_is_the_same_window_of_whole_rows(dsrt, rect, oracle, rng_mode):
    hs, scene, W, H, spp = _scene(dsrt, "station_near", spp=4, seed=0xDEADBEEFDEADBEEF)
    if rng_mode == 0:
        full, full32, _ = oracle.render(scene, W, H)                  # dsrt_oracle_render_rows
    else:
        full, full32, _ = rect.render(scene, W, H)
    x0, x1, y0, y1 = 37, 151, 20, 77
    win, win32, cnt = rect.render(scene, W, H, rng_mode=rng_mode, x0=x0, x1=x1, y0=y0, y1=y1)
    assert cnt["samples"] == (x1 - x0) * (y1 - y0) * spp
    r0, r1 = H - y1, H - y0                                           # kernel row y is image row H-1-y
    assert np.array_equal(win[r0:r1, x0:x1], full[r0:r1, x0:x1]) and win[r0:r1, x0:x1].max() > 0
    assert np.array_equal(win32[r0:r1, x0:x1].view(np.uint32), full32[r0:r1, x0:x1].view(np.uint32))
    mask = np.ones((H, W), bool)
    mask[r0:r1, x0:x1] = False
    assert not win[mask].any() and not win32[mask].any()             # nothing outside the rectangle is written
    # rows given one by one are the same rows
    some, _, _ = rect.render(scene, W, H, rng_mode=rng_mode, rows=[0, 55, H - 1])
    for y in (0, 55, H - 1):
        assert np.array_equal(some[H - 1 - y], full[H - 1 - y])
    # the old entry point is the rectangle in mode 0
    if rng_mode == 0:
        rows, _, _ = oracle.render(scene, W, H, y0, y1)
        assert np.array_equal(rows[r0:r1], full[r0:r1])


def test_rect_refuses_bad_arguments(dsrt, rect):
    import ctypes as C
    hs, scene, W, H, spp = _scene(dsrt, "lights", spp=1)
    buf = np.zeros((H, W, 3), np.uint8)
    f = np.zeros((H, W, 3), np.float32)
    for args in ((0, W + 1, 0, H, 1), (-1, W, 0, H, 1), (5, 4, 0, H, 1), (0, W, 0, H + 1, 1), (0, W, 0, H, 2), (0, W, 0, H, -1)):
        assert rect.lib.dsrt_oracle_render_rect(C.byref(scene), W, H, *args, buf.ctypes.data, f.ctypes.data, None) < 0, args
    assert not buf.any()
