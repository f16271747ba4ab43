"""The coverage pass with one sample is the G-buffer pass (include/dsrt.h, COVERAGE) on the parity scenes with textured albedo and with spheres: the two kernels
take the hit's record and its channel stores from one place (csrc/hit_record.h).  tests/test_gpu_coverage.py holds the same identity on station_near, which has
triangles and no textures.  Every float comparison is on uint32 views."""
import pytest

import _coverage_model as M
from test_gpu_coverage import DIAG, GRID, _cd, _same, _scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["textured", "mixed"])
def test_one_sample_is_the_gbuffer_on_textures_and_spheres(dsrt, gpu_ctx, name):
    W, H = 29, 17                                                        # the oracle's centre rays: textured 220 hits / 273 misses, mixed 30 / 463 with 14 on spheres
    hs, scene = _scene(dsrt, name, W, H)
    gpu_ctx.upload(scene)
    desc = dsrt.make_desc(W, H, 1)
    gb = gpu_ctx.gbuffer_to_host(desc)
    centre = (gb["flags"] & 1).astype(bool)
    assert centre.any() and not centre.all()
    assert name != "mixed" or (gb["flags"] & 4).any()
    for pattern in (GRID, DIAG):
        got = gpu_ctx.coverage_to_host(desc, _cd(dsrt, pattern, 1), rep=True)
        for k in M.GB_KEYS:
            _same(got["rep"][k], gb[k], (name, "samples = 1", pattern, k))
