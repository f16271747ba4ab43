"""The CPU model of sample sets (tests/oracle_sample_sets.c over the oracle's own rng_mode 1 path) on its own, on the CPU: the full set resolves to
the oracle's mode-1 image, the sums of disjoint sets add up to the sum of their union, and the header's variance formula (include/dsrt.h, SAMPLE SETS)
behaves.  tests/test_gpu_accumulate.py holds the kernel to this model."""
import numpy as np
import pytest

from test_oracle import CASES
from _oracle_mode1 import RectOracle
from _sample_sets import SetOracle, contiguous, interleaved, parity_case, variance_of_mean

SEED = 0xDEADBEEF00001337


@pytest.fixture(scope="module")
def sets(dsrt):
    return SetOracle()


@pytest.fixture(scope="module")
def rect(dsrt):
    return RectOracle()


@pytest.mark.parametrize("name", sorted(CASES))
def test_full_set_resolves_to_the_oracle_mode1_image(dsrt, sets, rect, name):
    hs, scene, W, H, spp, depth = parity_case(dsrt, name, SEED)
    band = dict(y0=3 * H // 8, y1=5 * H // 8)                       # a band of whole rows through the middle of the frame (the CPU is slow)
    want, want32, _ = rect.render(scene, W, H, **band)
    S, S2 = sets.sums(scene, W, H, 0, spp, 1, **band)
    rgb, f32, _ = sets.resolve(S, S2, spp, scene.params.gamma)
    assert want.max() > 0
    assert np.array_equal(rgb, want), (rgb != want).any(axis=-1).sum()
    assert np.array_equal(f32.view(np.uint32), want32.view(np.uint32))


@pytest.mark.parametrize("name", ["mixed", "station_near"])
def test_disjoint_sets_add_up_to_their_union(dsrt, sets, name):
    hs, scene, W, H, spp, depth = parity_case(dsrt, name, SEED)
    box = dict(x0=W // 3, x1=W // 3 + 24, y0=H // 3, y1=H // 3 + 16)
    S, S2 = sets.sums(scene, W, H, 0, spp, 1, **box)
    assert S.any()
    mixed = [(0, 2, 1)] + [(2 + p, c, 2) for p, c, _ in interleaved(spp - 2, 2)]          # a contiguous head, then two interleaved passes
    for split in (contiguous(spp, [1, 5]), interleaved(spp, 3), mixed):
        covered = sorted(f + j * s for f, c, s in split for j in range(c))
        assert covered == list(range(spp)), split
        tot, tot2 = np.zeros_like(S), np.zeros_like(S2)
        for f, c, s in split:
            a, a2 = sets.sums(scene, W, H, f, c, s, **box)
            tot += a
            tot2 += a2
        assert np.array_equal(tot, S) and np.array_equal(tot2, S2), split


def _light_scene(dsrt):
    """The camera inside an emissive sphere brighter than 1 in every channel: every sample clamps to exactly 1.0 (2^20 units)."""
    capi = dsrt.capi
    sph = np.zeros(1, capi.SPHERE_DTYPE)
    sph["radius"] = 50.0
    mats = np.zeros(1, capi.MAT_DTYPE)
    mats["type"] = 3
    mats["emissive"] = (4.0, 2.0, 7.0)
    mats["albedo_tex"] = -1
    hs = dsrt.HostScene().add_arrays(spheres=sph, mats=mats)
    hs.build_bvh()
    return hs


def test_variance_is_zero_where_every_sample_clamps(dsrt, sets):
    hs = _light_scene(dsrt)
    W, H, spp = 16, 8, 37
    cam = dsrt.camera_look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 40.0, W, H, spp, 8)
    scene = hs.view(cam, None)
    scene.seed = SEED
    S, S2 = sets.sums(scene, W, H, 3, 11, 3)
    assert (S == 11 << 20).all() and (S2 == 11 << 20).all()
    var = variance_of_mean(S, S2, 11)
    assert not var.view(np.uint32).any()
    _, _, var_c = sets.resolve(S, S2, 11, scene.params.gamma, want_var=True)
    assert not var_c.view(np.uint32).any()


def test_variance_formula_in_numpy_is_the_models_bit_for_bit(dsrt, sets):
    hs, scene, W, H, spp, depth = parity_case(dsrt, "station_near", SEED)
    S, S2 = sets.sums(scene, W, H, 1, 5, 3, x0=90, x1=120, y0=40, y1=60)
    _, _, var = sets.resolve(S, S2, 5, scene.params.gamma, want_var=True)
    want = variance_of_mean(S, S2, 5)
    assert (var > 0).sum() > 100
    assert np.array_equal(var.view(np.uint32), want.view(np.uint32))
    # and it estimates what it says: the sample variance of the mean of sq-rounded squares, within the rounding of sq
    s = S.astype(np.float64) / 2 ** 20 / 5
    assert np.all(var.astype(np.float64) <= (s * (1 - s) * 5 / 4) / 5 + 1e-5)
