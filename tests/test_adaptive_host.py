"""Adaptive sampling without a GPU (include/dsrt.h, ADAPTIVE SAMPLING): the numpy model of the convergence test (tests/_adaptive_model.py) against a
plain-Python loop of the header's lines, the new structs' sizes against their ctypes mirrors, and the CLI's usage errors.  tests/test_gpu_adaptive.py
holds the kernels to the model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT
from _adaptive_model import UINT32_MAX, converged, exact_limit_case, needed_tolerance, select_unconverged, select_unconverged_python


def edge_pixels():
    """(S, S2, n) rows of hand-made pixels, and what each is there for."""
    one = 1 << 20
    lim_S, lim_S2 = exact_limit_case(2, one, 0.5)
    rows = [
        ((0, 0, 0), (0, 0, 0), 0, "n = 0"),
        ((one, one, one), (one, one, one), 1, "n = 1"),
        ((2 * one, 2 * one, 2 * one), (2 * one, 2 * one, 2 * one), 2, "n = 2, two equal samples: v = 0"),
        ((0, 0, 0), (0, 0, 0), 5, "S = S2 = 0"),
        ((3 * one, 3 * one, 3 * one), (1, 1, 1), 3, "S2 far too small: v negative, clamps to 0"),
        ((lim_S,) * 3, (lim_S2,) * 3, 2, "vm == lim*lim exactly (rel_tol 0.5, floor 0)"),
        ((lim_S,) * 3, (lim_S2 + 1,) * 3, 2, "one unit past the limit"),
        ((lim_S,) * 3, (lim_S2, lim_S2 + 4096, lim_S2), 2, "one channel fails, two pass"),
        ((40, 40, 40), (30, 30, 30), 4, "mean below the floor"),
        ((4 * one, 4 * one, 4 * one), (5 * one, 5 * one, 5 * one), 4, "mean above the floor"),
        ((7 * one, 6 * one, 5 * one), (9 * one, 8 * one, 7 * one), 9, "n >= n_max"),
        ((7 * one, 6 * one, 5 * one), (7 * one, 6 * one, 5 * one), 3, "n < n_min, converged otherwise"),
    ]
    S = np.array([r[0] for r in rows], np.uint64)
    S2 = np.array([r[1] for r in rows], np.uint64)
    n = np.array([r[2] for r in rows], np.uint32)
    return S, S2, n, [r[3] for r in rows]


SETTINGS = [(0.5, 0.0, 0, UINT32_MAX), (0.5, 0.25, 0, UINT32_MAX), (0.5, 0.0, 4, 9), (0.0, 0.0, 0, UINT32_MAX), (1e30, 0.0, 0, UINT32_MAX),
            (0.01, 1e-3, 2, 6)]


def test_the_edge_pixels_say_what_they_are_for():
    S, S2, n, what = edge_pixels()
    m = dict(zip(what, select_unconverged(S, S2, n, 0.5, 0.0)))
    assert m["n = 0"] == 1 and m["n = 1"] == 1                                     # never converged below two samples
    assert m["n = 2, two equal samples: v = 0"] == 0 and m["S = S2 = 0"] == 0      # vm = 0 <= anything
    assert m["S2 far too small: v negative, clamps to 0"] == 0
    assert m["vm == lim*lim exactly (rel_tol 0.5, floor 0)"] == 0                  # <=, not <
    assert m["one unit past the limit"] == 1 and m["one channel fails, two pass"] == 1
    # the floor takes over for a dark pixel: with it the limit is rel_tol * floor, without it rel_tol * m
    dark = what.index("mean below the floor")
    assert needed_tolerance(S[dark], S2[dark], n[dark], 0.0) > needed_tolerance(S[dark], S2[dark], n[dark], 0.25)
    bright = what.index("mean above the floor")
    assert needed_tolerance(S[bright], S2[bright], n[bright], 0.0) == needed_tolerance(S[bright], S2[bright], n[bright], 0.25)
    capped = select_unconverged(S, S2, n, 0.0, 0.0, 4, 9)
    assert capped[what.index("n >= n_max")] == 0 and capped[what.index("n < n_min, converged otherwise")] == 1


def test_numpy_model_is_the_plain_python_loop():
    S, S2, n, what = edge_pixels()
    for tol, floor, n_min, n_max in SETTINGS:
        assert np.array_equal(select_unconverged(S, S2, n, tol, floor, n_min, n_max), select_unconverged_python(S, S2, n, tol, floor, n_min, n_max)), (tol, floor)
    rng = np.random.default_rng(20261018)
    # random sums of n quantised samples in [0, 2^20], the squares rounded as the kernel rounds them (include/dsrt.h, SAMPLE SETS)
    n = rng.integers(0, 40, size=(30, 40)).astype(np.uint32)
    S = np.zeros(n.shape + (3,), np.uint64)
    S2 = np.zeros_like(S)
    spread = rng.random(n.shape + (3,)) ** 4                                        # most pixels nearly constant, some noisy
    for k in range(int(n.max())):
        q = np.clip((0.5 + spread * (rng.random(n.shape + (3,)) - 0.5)) * (1 << 20), 0, 1 << 20).astype(np.uint64)
        live = (k < n)[..., None]
        S += np.where(live, q, 0).astype(np.uint64)
        S2 += np.where(live, (q * q + (1 << 19)) >> 20, 0).astype(np.uint64)
    seen = set()
    for tol, floor, n_min, n_max in SETTINGS + [(0.05, 0.0, 0, UINT32_MAX), (0.2, 0.6, 3, 30)]:
        got = select_unconverged(S, S2, n, tol, floor, n_min, n_max)
        assert np.array_equal(got, select_unconverged_python(S, S2, n, tol, floor, n_min, n_max)), (tol, floor, n_min, n_max)
        seen.update(np.unique(got).tolist())
    assert seen == {0, 1}
    assert converged(S, S2, n, 1e30, 0.0)[n >= 2].all() and not converged(S, S2, n, 1e30, 0.0)[n < 2].any()


def test_struct_sizes_and_exports(dsrt):
    from dsrt_amd import capi
    assert dsrt.lib.dsrt_sizeof(10) == C.sizeof(capi.DsrtAdaptive) == 16
    assert dsrt.lib.dsrt_sizeof(11) == C.sizeof(capi.DsrtAdaptiveStats) == 16 + 64 * 4
    assert [f for f, _ in capi.DsrtAdaptive._fields_] == ["passes", "min_passes", "rel_tol", "floor"]
    assert [f for f, _ in capi.DsrtAdaptiveStats._fields_] == ["passes_run", "samples_total", "active"]
    assert capi.ABI_VERSION == dsrt.lib.dsrt_abi_version() == 8                       # additive: the version stays
    for name in ("dsrt_render_accumulate_masked", "dsrt_render_accumulate_masked_to_host", "dsrt_select_unconverged", "dsrt_resolve_accumulated_counts",
                 "dsrt_render_adaptive", "dsrt_render_adaptive_to_host"):
        assert name in capi.EXPORTS and hasattr(dsrt.lib, name)
    for m in ("render_accumulate_masked", "select_unconverged", "resolve_accumulated_counts", "render_adaptive"):
        assert hasattr(dsrt.Context, m)
    assert hasattr(dsrt.Accumulator, "resolve_counts")


def test_null_arguments_are_invalid_without_a_device(dsrt):
    from dsrt_amd import capi
    lib = dsrt.lib
    desc = dsrt.make_desc(16, 16, 4, rng_mode=1)
    acc = capi.DsrtAccum()
    ad = capi.DsrtAdaptive(2, 1, 0.1, 0.0)
    assert lib.dsrt_render_accumulate_masked(None, C.byref(desc), 0, 1, 1, C.byref(acc), None, None, None, None) == -1
    assert lib.dsrt_select_unconverged(None, C.byref(desc), C.byref(acc), None, 0.1, 0.0, 0, 0, None, None, None) == -1
    assert lib.dsrt_resolve_accumulated_counts(None, C.byref(desc), C.byref(acc), None, None, None, None, None) == -1
    assert lib.dsrt_render_adaptive(None, C.byref(desc), C.byref(ad), C.byref(acc), None, None, None, None, None, None) == -1
    assert lib.dsrt_render_adaptive_to_host(None, C.byref(desc), C.byref(ad), None, None, None, None, None) == -1
    assert b"null" in lib.dsrt_last_error()


@pytest.mark.parametrize("flags, says", [
    (["--adaptive", "0.05"], "rng-mode 1"),                                                   # rng_mode 0
    (["--rng-mode", "1", "--adaptive", "0.05", "--passes", "2"], "--passes"),
    (["--rng-mode", "1", "--adaptive", "0.05", "--gbuffer"], "--gbuffer"),
    (["--rng-mode", "1", "--adaptive-passes", "4"], "--adaptive TOL"),
    (["--rng-mode", "1", "--adaptive", "0.05", "--adaptive-passes", "0"], "--adaptive-passes"),
    (["--rng-mode", "1", "--adaptive", "0.05", "--adaptive-passes", "65"], "--adaptive-passes"),
    (["--rng-mode", "1", "--spp", "4", "--adaptive", "0.05", "--adaptive-passes", "5"], "--adaptive-passes"),
    (["--rng-mode", "1", "--adaptive", "0.05", "--adaptive-passes", "4", "--adaptive-min-passes", "5"], "--adaptive-min-passes"),
    (["--rng-mode", "1", "--adaptive", "-1"], ">= 0"),
    (["--rng-mode", "1", "--adaptive"], "needs a value"),
])
def test_cli_usage_errors(flags, says, tmp_path):
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    assert os.path.exists(exe), "build the CLI with `make tools`"
    r = subprocess.run([exe, "--obj", os.path.join(ASSETS, "station_3k.obj"), "--output_dir", str(tmp_path / "out")] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert says in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


def test_cli_usage_names_adaptive():
    exe = os.path.join(ROOT, "deep-space-ray-tracer_amd", "dsrt_render")
    r = subprocess.run([exe, "--no-such-flag"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--adaptive TOL [--adaptive-passes P] [--adaptive-min-passes M] [--adaptive-floor F]]" in r.stderr
