"""The detector model of include/dsrt.h (SENSOR MODEL) in numpy, operation for operation: float32 arrays vectorised over the pixels, a Python loop over the taps in the
header's order (ky outer, kx inner), Philox4x32-10 on uint64 products, kInvSigma derived in float64.  numpy's float32 +, *, /, sqrt and floor are the correctly
rounded IEEE operations and nothing here is fused, so the result is the header's, bit for bit.  Shared by tests/test_sensor_host.py (CPU) and tests/test_gpu_sensor.py."""
import numpy as np

F = np.float32
U32 = np.uint32
U64 = np.uint64

DEFAULTS = dict(mono=0, gain_e=20000.0, prnu=0.0, dark_e=0.0, dsnu_e=0.0, read_e=10.0, full_well_e=20000.0, e_per_dn=5.0, offset_dn=64.0, bits=12, noise=1, seed=1337, frame=0)

S_MEAN = 8 * 65535 / 2                       # 262140: eight uniform 16-bit terms
S_VAR = 8 * (2 ** 32 - 1) // 12              # 2863311530: the variance of their sum, 8 (2^32 - 1) / 12
assert 8 * (2 ** 32 - 1) % 12 == 0 and S_VAR == 2863311530 and S_MEAN == 262140
K_INV_SIGMA = F(1.0 / np.sqrt(np.float64(S_VAR)))          # float64 arithmetic, rounded once to fp32
assert K_INV_SIGMA == F(float.fromhex("0x1.3988e2p-16")), float(K_INV_SIGMA).hex()      # the header's literal

TAG = 0x53454E53                             # the last counter word
KIND_TEMPORAL, KIND_PRNU, KIND_DSNU = 0, 1, 2


def philox4x32_10(k0, k1, c0, c1, c2, c3):
    """One Philox4x32-10 block per element: key words k0, k1 and counter words c0 .. c3 (uint32 arrays or scalars, broadcast) -> four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, U64) & U64(0xFFFFFFFF) for c in (c0, c1, c2, c3)))
    k0, k1 = U64(int(k0) & 0xFFFFFFFF), U64(int(k1) & 0xFFFFFFFF)
    m0, m1, mask, s32 = U64(0xD2511F53), U64(0xCD9E8D57), U64(0xFFFFFFFF), U64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                                  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + U64(0x9E3779B9)) & mask, (k1 + U64(0xBB67AE85)) & mask
    return tuple(c.astype(U32) for c in (c0, c1, c2, c3))


def draw(seed, pixel, plane, kind, frame):
    """z of step 3 for every element of `pixel` (uint32 pixel numbers y*W + x): float32."""
    words = philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, pixel, plane + 4 * kind, frame if kind == KIND_TEMPORAL else 0, TAG)
    S = sum((w & U32(0xFFFF)).astype(np.int64) + (w >> U32(16)).astype(np.int64) for w in words)
    return (S.astype(F) - F(262140.0)) * K_INV_SIGMA              # S < 2^24: the conversion is exact


def planes_of(linear, mono):
    """Step 1: (H, W, C) float32, C = 1 (the luminance) or 3."""
    x = np.ascontiguousarray(linear, F)
    if not mono:
        return x
    return ((F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2])[..., None]


def blur(planes, psf):
    """Step 2: the convolution with the skip outside the image; psf None is the single tap 1.0f."""
    taps = np.ones((1, 1), F) if psf is None else np.ascontiguousarray(psf, F)
    n = taps.shape[0]
    assert taps.shape == (n, n) and n % 2 == 1
    r = (n - 1) // 2
    H, W, _ = planes.shape
    s = np.zeros(planes.shape, F)                                  # +0.0f
    for ky in range(-r, r + 1):
        y0, y1 = max(0, -ky), min(H, H - ky)                       # the pixels whose row y + ky is inside
        if y0 >= y1:
            continue
        for kx in range(-r, r + 1):
            x0, x1 = max(0, -kx), min(W, W - kx)
            if x0 >= x1:
                continue
            w = taps[r - ky, r - kx]
            s[y0:y1, x0:x1] = s[y0:y1, x0:x1] + w * planes[y0 + ky:y1 + ky, x0 + kx:x1 + kx]
    return s


def detect(s, gain_e, prnu, dark_e, dsnu_e, read_e, full_well_e, e_per_dn, offset_dn, bits, noise, seed, frame, **_):
    """Steps 3 to 5 on the blurred signal s (H, W, C): DN as uint16 (H, W, C)."""
    H, W, C = s.shape
    pixel = np.arange(H * W, dtype=U32).reshape(H, W)
    gain_e, prnu, dark_e, dsnu_e, read_e, full_well_e, e_per_dn, offset_dn = (F(v) for v in (gain_e, prnu, dark_e, dsnu_e, read_e, full_well_e, e_per_dn, offset_dn))
    dn = np.zeros(s.shape, np.uint16)
    top = F((1 << bits) - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(C):
            zero = np.zeros((H, W), F)
            z1 = draw(seed, pixel, k, KIND_PRNU, frame) if prnu != 0 else zero
            z2 = draw(seed, pixel, k, KIND_DSNU, frame) if dsnu_e != 0 else zero
            z0 = draw(seed, pixel, k, KIND_TEMPORAL, frame) if noise else zero
            e = s[..., k] * gain_e
            e = e * (F(1.0) + prnu * z1)
            d = np.fmax(dark_e + dsnu_e * z2, F(0.0))
            m = np.fmax(e, F(0.0)) + d
            sg = np.sqrt(m + read_e * read_e)
            q = np.fmin(m + sg * z0, full_well_e)
            v = np.floor((q / e_per_dn + offset_dn) + F(0.5))
            for a in (e, d, m, sg, q, v):
                assert a.dtype == F
            low, high = ~(v >= 0), v > top
            inside = np.where(low | high, F(0.0), v).astype(np.uint16)      # (uint16_t)v where neither clamp applies
            dn[..., k] = np.where(low, np.uint16(0), np.where(high, np.uint16(top), inside))
    return dn


def apply(linear, psf=None, **params):
    """The whole call: (dn, signal, rgb8) -- uint16 and float32 of shape (H, W, 3), or (H, W) when mono, and uint8 (H, W, 3)."""
    p = {**DEFAULTS, **params}
    s = blur(planes_of(linear, p["mono"]), psf)
    dn = detect(s, **p)
    rgb8 = (dn >> np.uint16(p["bits"] - 8)).astype(np.uint8)
    if p["mono"]:
        return dn[..., 0], s[..., 0], np.repeat(rgb8, 3, axis=2)
    return dn, s, rgb8


def read_pnm(path):
    """A P5 / P6 file of any maxval as (H, W) or (H, W, 3): uint8, or uint16 from big-endian samples when maxval > 255.  Returns (array, maxval)."""
    data = open(path, "rb").read()
    magic, dims, maxval, rest = data.split(b"\n", 3)
    w, h = map(int, dims.split())
    maxval = int(maxval)
    ch = {b"P5": 1, b"P6": 3}[magic]
    a = np.frombuffer(rest, ">u2" if maxval > 255 else "u1").astype(np.uint16 if maxval > 255 else np.uint8)
    return (a.reshape(h, w) if ch == 1 else a.reshape(h, w, 3)), maxval
