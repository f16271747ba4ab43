"""ctypes bindings of the CPU model of sample sets (tests/oracle_sample_sets.c, built by the top-level Makefile's `oracle` target next to this file):
per-pixel sums S / S2 of any set {first + j*stride} of a pixel's rng_mode 1 samples, and their resolve (include/dsrt.h, SAMPLE SETS).  Shared by
tests/test_sample_sets_host.py (CPU) and tests/test_gpu_accumulate.py."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import ROOT
from test_oracle import CASES, SUN

LIB = os.path.join(ROOT, "tests", "liboracle_sample_sets.so")
MAX_THREADS = 16


def variance_of_mean(S, S2, n):
    """The header's formula in numpy float64, in its order: every step a correctly rounded IEEE operation."""
    s = S.astype(np.float64) * 2.0 ** -20
    s2 = S2.astype(np.float64) * 2.0 ** -20
    v = (s2 - s * s / float(n)) / float(n - 1)
    v = np.where(v > 0, v, 0.0)
    return (v / float(n)).astype(np.float32)


class SetOracle:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(f"{LIB} is missing: `make oracle` (or __graft_entry__.build()) builds it")
        self.lib = L = C.CDLL(LIB)
        L.dsrt_sets_sum_rect.restype = C.c_int
        L.dsrt_sets_sum_rect.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.c_void_p] * 2
        L.dsrt_sets_resolve.restype = C.c_int
        L.dsrt_sets_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]

    def sums(self, scene, W, H, first, count, stride=1, x0=0, x1=None, y0=0, y1=None, moments=True, threads=MAX_THREADS):
        """(S, S2) of the set over the rectangle x in [x0, x1), y in [y0, y1) (y = 0 the bottom row): (H, W, 3) uint64 in image order, zero
        outside the rectangle (S2 is None without moments)."""
        x1 = W if x1 is None else x1
        y1 = H if y1 is None else y1
        S = np.zeros((H, W, 3), np.uint64)
        S2 = np.zeros((H, W, 3), np.uint64) if moments else None

        def row(y):
            rc = self.lib.dsrt_sets_sum_rect(C.byref(scene), W, H, x0, x1, y, y + 1, first, count, stride, S.ctypes.data,
                                             S2.ctypes.data if moments else None)
            assert rc == 0, rc
        rows = list(range(y0, y1))
        with ThreadPoolExecutor(max_workers=max(1, min(threads, len(rows)))) as ex:
            list(ex.map(row, rows))
        return S, S2

    def resolve(self, S, S2, samples_done, gamma, want_var=False):
        """(rgb8, f32, var) of the sums after samples_done samples (var None unless asked for)."""
        S = np.ascontiguousarray(S, np.uint64)
        rgb = np.zeros(S.shape, np.uint8)
        f32 = np.zeros(S.shape, np.float32)
        var = np.zeros(S.shape, np.float32) if want_var else None
        S2c = np.ascontiguousarray(S2, np.uint64) if S2 is not None else None
        rc = self.lib.dsrt_sets_resolve(S.ctypes.data, S2c.ctypes.data if S2c is not None else None, S.size // 3, int(samples_done), float(gamma),
                                        rgb.ctypes.data, f32.ctypes.data, var.ctypes.data if want_var else None)
        assert rc == 0, rc
        return rgb, f32, var


def parity_case(dsrt, name, seed, spp=None):
    """A parity scene of tests/test_oracle.py as a host view with rng_mode 1's seed: (hs, scene, W, H, spp, depth)."""
    from conftest import load_world
    world, cam_args, spp0 = CASES[name]
    spp = spp0 if spp is None else spp
    hs = load_world(dsrt, world)
    W, H, depth = cam_args[3], cam_args[4], cam_args[5]
    cam = dsrt.camera_look_at(cam_args[0], cam_args[1], cam_args[2], W, H, spp, depth)
    scene = hs.view(cam, SUN)
    scene.seed = seed
    return hs, scene, W, H, spp, depth


def interleaved(spp, passes):
    """(first, count, stride) of `passes` interleaved passes over [0, spp) (empty passes left out)."""
    return [(p, len(range(p, spp, passes)), passes) for p in range(passes) if p < spp]


def contiguous(spp, cuts):
    """(first, count, 1) of [0, spp) cut at the given points (uneven pieces)."""
    edges = [0] + sorted(c for c in set(cuts) if 0 < c < spp) + [spp]
    return [(a, b - a, 1) for a, b in zip(edges, edges[1:])]
