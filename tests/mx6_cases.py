"""The 6-bit storage restated in numpy (include/lmi_hip.h, "the MXFP6 format"):
quantise, distances in float64 and float32, independent of li/.

  block      32 consecutive columns of the row as float32, zeros past d
  scale      !(m >= 2^-100) (m the block's max |v|, NaN included): codes +0,
             byte 127; else e = floor(log2 m) - 2, byte e + 127
  code       t = v 2^-e; the E2M3 value nearest |t| -- k/8 for k < 8, then
             (1 + m/8) {1, 2, 4}, index 8 E + M -- ties to the even mantissa,
             saturating at 7.5; bit 5 the sign, never set on a zero code
  fragment   column j of a block in bits [6j, 6j + 6) of the block's 24 bytes
             read as one little-endian number; a row's fragments back to back
  scales     byte of block b at (b & 1) * d_pad/64 + (b >> 1)
  norm       n^2 = sum_b S_b 2^(2e_b - 6) in float64 in block order, S_b the
             integer sum of (8c)^2; inv = 1 if n^2 == 0 else float32(1/sqrt(n^2))
  distance   d = fma(-acc, invq * invy, 1), acc = sum over blocks of the scaled
             code products
"""
import numpy as np

from mx4_cases import distances32, distances64  # noqa: F401  (the same two formulas)

E2M3 = np.array([k / 8 for k in range(8)] + [(1 + m / 8) * s for s in (1.0, 2.0, 4.0) for m in range(8)])
D_PAD = 768


def quantize(v, d_pad=D_PAD):
    """(codes uint8 [n, d_pad*3/4], scales uint8 [n, d_pad/32], inv float32 [n],
    values float64 [n, d_pad]: every column's code times its block scale)."""
    v = np.asarray(v)
    assert v.ndim == 2 and v.dtype in (np.float16, np.float32, np.float64) and v.shape[1] <= d_pad
    n, nb = v.shape[0], d_pad // 32
    x = np.zeros((n, d_pad), np.float32)
    x[:, :v.shape[1]] = v.astype(np.float32)
    xb = x.reshape(n, nb, 32)
    with np.errstate(invalid="ignore"):
        m = np.abs(xb).max(axis=2)                       # (a NaN makes the maximum NaN)
        live = m >= np.float32(2.0 ** -100)
    ef = np.where(live, (m.view(np.uint32) >> 23) & 0xFF, 129).astype(np.int64)   # e = ef - 129
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(live[..., None], xb.astype(np.float64) * 2.0 ** (129 - ef)[..., None], 0.0)
    a = np.minimum(np.abs(t), 7.5)
    # nearest grid value; of two equally near, the even index (the grid ascends with the index)
    lo = np.clip(np.searchsorted(E2M3, a, side="right") - 1, 0, 30)
    dl, dh = a - E2M3[lo], E2M3[lo + 1] - a
    idx = np.where((dh < dl) | ((dh == dl) & (lo % 2 == 1)), lo + 1, lo)
    six = (idx | np.where((t < 0) & (idx != 0), 32, 0)).reshape(n, d_pad).astype(np.uint8)
    bits = np.unpackbits(six[:, :, None], axis=2, bitorder="little")[:, :, :6]
    codes = np.packbits(bits.reshape(n, d_pad * 6), axis=1, bitorder="little")
    byte = (ef - 2).astype(np.uint8)
    scales = np.concatenate([byte[:, 0::2], byte[:, 1::2]], axis=1)
    S = ((8 * E2M3[idx]) ** 2).sum(axis=2)               # exact integers <= 115 200
    n2 = np.zeros(n, np.float64)
    for b in range(nb):                                  # block order
        n2 = n2 + S[:, b] * 2.0 ** (2 * (ef[:, b] - 129) - 6)
    inv = np.ones(n, np.float32)
    inv[n2 > 0] = (1.0 / np.sqrt(n2[n2 > 0])).astype(np.float32)
    vals = (np.sign(t) * E2M3[idx] * 2.0 ** (ef - 129)[..., None]).reshape(n, d_pad)
    return codes, scales, inv, vals
