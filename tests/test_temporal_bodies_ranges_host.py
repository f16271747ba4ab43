"""The motion stage's body search on the CPU (include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES; host/body_motion.cpp) at the sizes
tests/test_temporal_bodies_host.py does not reach: all 16 ranges, empty ones among them, every edge of every range planted; and triangle ranges that end at
2^31 or reach beyond it, where a 32-bit unsigned range test alone would take negative prim_id values for a body's.  The shared pieces (ranges16,
prims16, poses16, prims_around_2_31, ranges_to_2_31) also feed tests/test_gpu_temporal_bodies_ranges.py."""
import numpy as np
import pytest

import _bodies_model as B
import _motion_model as model
from _denoise_model import F
from test_temporal_bodies_host import _bits, _random_motion

SPECIAL_PRIMS = [-1, -2, -7, 0, 10 ** 6, 2 ** 31 - 1, -2 ** 31]
UNMOVED16 = (5, 11)                          # every other non-empty body >= 1 moves


def ranges16(last_live=False):
    """(first_tri, num_tris) of 16 bodies that tile [0, 600): three empty ranges -- body 2 between two live ones, with its successor's first; body 7; and the last
    body, 15.  last_live: bodies 14 and 15 share what body 14 had, so that the last entry of every table is in use."""
    num = np.array([40, 37, 0, 51, 33, 45, 29, 0, 60, 41, 38, 47, 35, 52, 92, 0], np.int32)
    if last_live:
        num[14:] = (50, 42)
    first = (np.cumsum(num) - num).astype(np.int32)
    assert first[15] + num[15] == 600 and first[2] == first[3] and (num == 0).sum() == (2 if last_live else 3)
    return first, num


def prims16(rng, shape, first, num):
    """prim_id random over [-4, 604) with every edge of every range planted -- first - 1, first, first + num - 1, first + num -- and the special values."""
    edges = sorted({int(f) + d for f, n in zip(first, num) for d in (-1, 0, int(n) - 1, int(n))} | set(SPECIAL_PRIMS))
    prim = rng.integers(-4, 604, size=shape)
    flat = prim.reshape(-1)
    assert flat.size >= 4 * len(edges)
    flat[rng.choice(flat.size, size=len(edges), replace=False)] = edges
    assert set(edges) <= set(flat.tolist())
    return prim.astype(np.int32)


def poses16(rng, make):
    """(poses_prev, poses_cur), (16, 12) each: make() per body and frame; the bodies of UNMOVED16 keep their pose; entry 0 holds what must be ignored."""
    pp, pc = np.zeros((16, 12), F), np.zeros((16, 12), F)
    for b in range(1, 16):
        pp[b], pc[b] = make(), make()
    for b in UNMOVED16:
        pc[b] = pp[b]
    pp[0], pc[0] = 1.0, 2.0
    return pp, pc


@pytest.mark.parametrize("last_live", [False, True])
def test_host_form_equals_the_model_on_sixteen_ranges(dsrt, last_live):
    rng = np.random.default_rng(160 + last_live)
    n = 6000
    first, num = ranges16(last_live)
    pp, pc = poses16(rng, lambda: B._pose(B._rot(rng.standard_normal(3), rng.uniform(0, np.pi)), rng.uniform(-50, 50, 3)))
    prim = prims16(rng, n, first, num)
    X = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 4, (n, 1))).astype(F)
    N = rng.standard_normal((n, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F)
    body = model.body_of(prim, first, num)
    assert all(((body == b).sum() > 0) == (num[b] > 0) for b in range(16))                    # every non-empty body owns points, no empty one does
    moved = model.moved_bodies(pp, pc)
    assert [b for b in range(1, 16) if not moved[b]] == list(UNMOVED16)
    for f, k in zip(first, num):                                                              # the planted edges fall where the header's rule puts them
        for p in (int(f) - 1, int(f), int(f) + int(k) - 1, int(f) + int(k)):
            owner = [b for b in range(1, 16) if first[b] <= p < first[b] + num[b]]
            assert (body[prim == p] == (owner[0] if owner else 0)).all() and (prim == p).any()
    wantN, wantX = model.motion(first, num, pp, pc, prim, N, X)
    gotN, gotX = dsrt.body_motion_host(first, num, pp, pc, prim, N, X)
    assert np.array_equal(_bits(gotX), _bits(wantX)) and np.array_equal(_bits(gotN), _bits(wantN))
    on_moved = moved[body]
    assert (_bits(gotX)[on_moved] != _bits(X)[on_moved]).any(axis=1).all() and np.array_equal(_bits(gotX)[~on_moved], _bits(X)[~on_moved])
    # fewer bodies on the same arrays: the ranges beyond `bodies` are not looked at
    N5, X5 = dsrt.body_motion_host(first[:5], num[:5], pp[:5], pc[:5], prim, N, X)
    w5N, w5X = model.motion(first[:5], num[:5], pp[:5], pc[:5], prim, N, X)
    assert np.array_equal(_bits(X5), _bits(w5X)) and np.array_equal(_bits(N5), _bits(w5N)) and np.array_equal(_bits(X5)[body >= 5], _bits(X)[body >= 5])


def prims_around_2_31(n):
    """prim_id at both ends of int32: -2^31 .. -2^31 + 200, 2^31 - 11 .. 2^31 - 1, -1 and 0, repeated to n entries."""
    vals = np.concatenate([np.arange(-2 ** 31, -2 ** 31 + 201), np.arange(2 ** 31 - 11, 2 ** 31), [-1, 0]])
    assert n >= vals.size
    return np.resize(vals, n).astype(np.int32)


def ranges_to_2_31(past=False):
    """Four bodies; body 1's range ends at 2^31 exactly or, `past`, reaches 90 beyond it: for a 32-bit unsigned range test alone prim_id -2^31 + 5 would then lie
    on body 1, for the header's rule (and the int64 of the host form and the model) it never does."""
    return np.array([0, 2 ** 31 - 10, 100, 131], np.int32), np.array([40, 100 if past else 10, 31, 19], np.int32)


@pytest.mark.parametrize("past", [False, True])
def test_ranges_next_to_2_31_equal_the_model(dsrt, past):
    """The header's rule is first <= prim < first + num in exact arithmetic: a range that ends at 2^31 holds the last ten int32 values, one that reaches beyond holds
    the same ten, and no negative prim_id lies in either."""
    rng = np.random.default_rng(31)
    n = 561
    _, _, pp, pc, _, N, X = _random_motion(rng, n)
    prim = prims_around_2_31(n)
    first, num = ranges_to_2_31(past)
    assert int(first[1]) + int(num[1]) == 2 ** 31 + (90 if past else 0) and model.moved_bodies(pp, pc)[1]
    body = model.body_of(prim, first, num)
    assert set(prim[body == 1].tolist()) == set(range(2 ** 31 - 10, 2 ** 31)) and not body[prim < 0].any()
    wantN, wantX = model.motion(first, num, pp, pc, prim, N, X)
    gotN, gotX = dsrt.body_motion_host(first, num, pp, pc, prim, N, X)
    assert np.array_equal(_bits(gotX), _bits(wantX)) and np.array_equal(_bits(gotN), _bits(wantN))
    assert (_bits(gotX)[body == 1] != _bits(X)[body == 1]).any(axis=1).all() and np.array_equal(_bits(gotX)[body != 1], _bits(X)[body != 1])
