"""The 4-bit storage restated in numpy (include/lmi_hip.h, "the MXFP4 format"):
quantise, distances in float64 and float32, independent of li/.

  block      32 consecutive columns of the row as float32, zeros past d
  scale      !(m >= 2^-100) (m the block's max |v|, NaN included): codes +0,
             byte 127; else e = floor(log2 m) - 2, byte e + 127
  code       t = v 2^-e; the E2M1 value of {0, .5, 1, 1.5, 2, 3, 4, 6} nearest
             |t|, ties to the even mantissa, saturating at 6; bit 3 the sign,
             never set on a zero code; column 2i the low nibble of byte i
  scales     byte of block b at (b & 1) * d_pad/64 + (b >> 1)
  norm       n^2 = sum_b S_b 2^(2e_b - 2) in float64 in block order, S_b the
             integer sum of (2c)^2; inv = 1 if n^2 == 0 else float32(1/sqrt(n^2))
  distance   d = fma(-acc, invq * invy, 1), acc = sum over blocks of the scaled
             code products
"""
import numpy as np

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
D_PAD = 768


def quantize(v, d_pad=D_PAD):
    """(codes uint8 [n, d_pad/2], scales uint8 [n, d_pad/32], inv float32 [n],
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
    a = np.abs(t)
    idx = ((a > 0.25).astype(np.int64) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    nib = (idx | np.where((t < 0) & (idx != 0), 8, 0)).reshape(n, d_pad).astype(np.uint8)
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    byte = (ef - 2).astype(np.uint8)
    scales = np.concatenate([byte[:, 0::2], byte[:, 1::2]], axis=1)
    S = ((2 * E2M1[idx]) ** 2).sum(axis=2)               # exact integers <= 4608
    n2 = np.zeros(n, np.float64)
    for b in range(nb):                                  # block order
        n2 = n2 + S[:, b] * 2.0 ** (2 * (ef[:, b] - 129) - 2)
    inv = np.ones(n, np.float32)
    inv[n2 > 0] = (1.0 / np.sqrt(n2[n2 > 0])).astype(np.float32)
    vals = (np.sign(t) * E2M1[idx] * 2.0 ** (ef - 129)[..., None]).reshape(n, d_pad)
    return codes, scales, inv, vals


def distances64(vq, invq, vy, invy):
    """float64 [nq, n]: 1 - <q^, y^> * float32(invq * invy), the products and the sum in float64."""
    p = invq.astype(np.float32)[:, None] * invy.astype(np.float32)[None, :]
    return 1.0 - (vq @ vy.T) * p.astype(np.float64)


def distances32(vq, invq, vy, invy):
    """float32 [nq, n] for sums that are exact in float32 (asserted): the fma's one rounding."""
    acc = vq @ vy.T
    assert np.array_equal(acc, acc.astype(np.float32).astype(np.float64))
    p = invq.astype(np.float32)[:, None] * invy.astype(np.float32)[None, :]
    x = acc * p.astype(np.float64)                       # exact: 24 x 24 bits
    s = 1.0 - x
    bb = s - 1.0
    err = (1.0 - (s - bb)) + (-x - bb)                   # TwoSum: 1 - x = s + err exactly
    out = s.astype(np.float32)
    from fractions import Fraction
    for i, j in zip(*np.nonzero(err)):                   # (s is inexact: round the exact value once)
        exact = 1 - Fraction(float(x[i, j]))
        lo = np.float32(float(exact))
        cands = [lo, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf))]
        out[i, j] = min(cands, key=lambda c: (abs(Fraction(float(c)) - exact), int(c.view(np.uint32)) & 1))
    return out
