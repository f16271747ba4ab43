"""ctypes bindings of the oracle's rng_mode 1 entry points (oracle/dsrt_oracle.h): dsrt_oracle_render_rect, the Philox words and the
per-sample quantisation / per-pixel mean.  Shared by tests/test_oracle_rng_mode1.py (CPU) and tests/test_gpu_rng_mode1.py."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import ROOT, Oracle

MAX_THREADS = 16            # the oracle runs outside the GIL (ctypes releases it): rows in parallel, at most 16 at a time


class RectOracle:
    COUNTER_NAMES = Oracle.COUNTER_NAMES

    def __init__(self, libm=False):
        self.lib = C.CDLL(os.path.join(ROOT, "oracle", "libdsrt_oracle_libm.so" if libm else "libdsrt_oracle.so"))
        L = self.lib
        L.dsrt_oracle_render_rect.restype = C.c_int
        L.dsrt_oracle_render_rect.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 3
        L.dsrt_oracle_philox_words.restype = None
        L.dsrt_oracle_philox_words.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
        L.dsrt_oracle_mode1_quantize.restype = C.c_uint32
        L.dsrt_oracle_mode1_quantize.argtypes = [C.c_float]
        L.dsrt_oracle_mode1_mean.restype = C.c_float
        L.dsrt_oracle_mode1_mean.argtypes = [C.c_uint64, C.c_int]

    def philox_words(self, seed, sub, first, n):
        out = np.zeros(n, np.uint32)
        self.lib.dsrt_oracle_philox_words(seed, sub, first, n, out.ctypes.data)
        return out

    def quantize(self, c):
        return self.lib.dsrt_oracle_mode1_quantize(c)

    def mean(self, s, spp):
        return self.lib.dsrt_oracle_mode1_mean(s, spp)

    def _call(self, scene, W, H, x0, x1, y0, y1, rng_mode, rgb, f32):
        cnt = (C.c_uint64 * len(self.COUNTER_NAMES))()
        rc = self.lib.dsrt_oracle_render_rect(C.byref(scene), W, H, x0, x1, y0, y1, rng_mode, rgb.ctypes.data, f32.ctypes.data, cnt)
        assert rc == 0, rc
        return list(cnt)

    def render(self, scene, W, H, rng_mode=1, x0=0, x1=None, y0=0, y1=None, rows=None, threads=MAX_THREADS):
        """Full-size (H, W, 3) rgb8 and float32 images with only the rectangle x in [x0, x1), y in [y0, y1) -- or only the kernel rows
        `rows` (y = 0 at the bottom), whole width -- rendered; everything else stays zero.  Returns (rgb8, f32, counters)."""
        x1 = W if x1 is None else x1
        if rows is None:
            y1 = H if y1 is None else y1
            rows = range(y0, y1)
        rgb = np.zeros((H, W, 3), np.uint8)
        f32 = np.zeros((H, W, 3), np.float32)
        rows = list(rows)
        with ThreadPoolExecutor(max_workers=max(1, min(threads, len(rows)))) as ex:
            parts = list(ex.map(lambda y: self._call(scene, W, H, x0, x1, y, y + 1, rng_mode, rgb, f32), rows))
        tot = [0] * len(self.COUNTER_NAMES)
        for p in parts:
            for i, v in enumerate(p):
                tot[i] = max(tot[i], v) if self.COUNTER_NAMES[i] == "max_stack" else tot[i] + v
        return rgb, f32, dict(zip(self.COUNTER_NAMES, tot))
