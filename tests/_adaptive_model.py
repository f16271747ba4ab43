"""The CPU model of adaptive sampling's convergence test (include/dsrt.h, ADAPTIVE SAMPLING: dsrt_select_unconverged) in numpy float64, in the header's
order -- every step a correctly rounded IEEE operation, as tests/_sample_sets.py: variance_of_mean -- and a plain-Python form of the same to pin the
numpy one.  Shared by tests/test_adaptive_host.py (CPU) and tests/test_gpu_adaptive.py."""
import numpy as np

UINT32_MAX = 0xFFFFFFFF


def channel_terms(S, S2, n):
    """(vm, m) per channel: the variance of the mean and the mean, float64, for sums (..., 3) uint64 and counts (...) uint32.  Pixels with n < 2 hold
    whatever 0/0 gives: the caller never looks at them."""
    nd = np.asarray(n, np.uint32).astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        s = np.asarray(S, np.uint64).astype(np.float64) * 2.0 ** -20
        s2 = np.asarray(S2, np.uint64).astype(np.float64) * 2.0 ** -20
        v = (s2 - s * s / nd) / (nd - 1.0)
        v = np.where(v > 0, v, 0.0)
        return v / nd, s / nd


def converged(S, S2, n, rel_tol, floor):
    """bool (...): n >= 2 and all three channels have vm <= (rel_tol * max(m, floor))^2, rel_tol and floor being the floats the ABI passes."""
    vm, m = channel_terms(S, S2, n)
    f = np.float64(np.float32(floor))
    with np.errstate(all="ignore"):
        r = np.where(m > f, m, f)
        lim = np.float64(np.float32(rel_tol)) * r
        ok = vm <= lim * lim
    return (np.asarray(n, np.uint32) >= 2) & ok.all(axis=-1)


def select_unconverged(S, S2, n, rel_tol, floor, n_min=0, n_max=UINT32_MAX):
    """The mask dsrt_select_unconverged writes: uint8 (...), 1 where the pixel still needs samples."""
    n = np.asarray(n, np.uint32)
    return ((n < np.uint32(n_max)) & ((n < np.uint32(n_min)) | ~converged(S, S2, n, rel_tol, floor))).astype(np.uint8)


def select_unconverged_python(S, S2, n, rel_tol, floor, n_min=0, n_max=UINT32_MAX):
    """The same, pixel by pixel with Python floats (IEEE doubles): the header's lines, one statement each."""
    S, S2, n = np.asarray(S, np.uint64), np.asarray(S2, np.uint64), np.asarray(n, np.uint32)
    out = np.zeros(n.shape, np.uint8)
    tol, fl = float(np.float32(rel_tol)), float(np.float32(floor))
    for idx in np.ndindex(n.shape):
        cnt = int(n[idx])
        conv = cnt >= 2
        if conv:
            nn = float(cnt)
            for ch in range(3):
                s = float(int(S[idx][ch])) * 2.0 ** -20
                s2 = float(int(S2[idx][ch])) * 2.0 ** -20
                v = (s2 - s * s / nn) / (nn - 1.0)
                v = v if v > 0 else 0.0
                vm = v / nn
                m = s / nn
                r = m if m > fl else fl
                lim = tol * r
                conv = conv and vm <= lim * lim
        out[idx] = 1 if cnt < n_max and (cnt < n_min or not conv) else 0
    return out


def needed_tolerance(S, S2, n, floor):
    """float64 (...): roughly the smallest rel_tol at which the pixel counts as converged -- max over the channels of sqrt(vm) / max(m, floor); inf for n < 2.
    For CHOOSING a tolerance between two pixels' values (with a gap around it); the verdict itself is converged()'s."""
    vm, m = channel_terms(S, S2, n)
    f = np.float64(np.float32(floor))
    with np.errstate(all="ignore"):
        need = (np.sqrt(vm) / np.where(m > f, m, f))
    need = np.where(np.isnan(need), 0.0, need).max(axis=-1)          # 0 / 0: a black pixel without a floor has vm = 0 <= 0
    return np.where(np.asarray(n, np.uint32) >= 2, need, np.inf)


def exact_limit_case(n=2, mean_q=1 << 20, rel_tol=0.5):
    """(S, S2) of one channel with vm == lim*lim EXACTLY, found by search over S2 with the model's own arithmetic: the last S2 that still converges must
    sit on the limit, and S2 + 1 must not converge."""
    S = np.uint64(n * mean_q)
    lo = int(S) * int(S) // (n << 20)                                 # about s*s/n in units of 2^-20: v = 0 there
    cand = np.arange(lo, lo + (1 << 21), dtype=np.uint64)
    Sv = np.broadcast_to(np.array([S, S, S], np.uint64), (cand.size, 3)).copy()
    S2v = np.stack([cand, cand, cand], axis=1)
    nv = np.full(cand.size, n, np.uint32)
    vm, m = channel_terms(Sv, S2v, nv)
    lim = np.float64(np.float32(rel_tol)) * m
    hit = np.flatnonzero(vm[:, 0] == (lim * lim)[:, 0])
    assert hit.size, "no S2 with vm == lim*lim in the searched range"
    k = int(hit[-1])
    assert converged(Sv[k], S2v[k], nv[k], rel_tol, 0.0) and not converged(Sv[k + 1], S2v[k + 1], nv[k + 1], rel_tol, 0.0)
    return int(S), int(cand[k])
