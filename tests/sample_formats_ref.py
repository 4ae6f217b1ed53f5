"""NumPy restatement of the sample formats of include/avsep.h (s16 / s24 / s32 PCM and f32), written from the header's table:
what one sample, a frame's down-mix and an output sample are.  The reference of test_wavio_host.py and
test_gpu_sample_formats.py; every function is exact arithmetic followed by ONE stated rounding."""
import numpy as np

BYTES = {"s16": 2, "s24": 3, "s32": 4, "f32": 4}
BITS = {"s16": 16, "s24": 24, "s32": 32}


def pack(values, fmt):
    """values [L, C] (integers of the format's range, or floats for f32) -> the file's bytes, uint8 [L*C*bytes]."""
    v = np.asarray(values)
    if fmt == "f32":
        return np.ascontiguousarray(v.astype("<f4")).view(np.uint8).reshape(-1).copy()
    v = v.astype(np.int64).reshape(-1)
    assert v.min() >= -2 ** (BITS[fmt] - 1) and v.max() < 2 ** (BITS[fmt] - 1)
    out = np.empty((v.size, BYTES[fmt]), np.uint8)
    for b in range(BYTES[fmt]):
        out[:, b] = (v >> (8 * b)) & 0xFF
    return out.reshape(-1)


def integers(raw, fmt, C):
    """The sign-extended integers of a PCM format, int64 [L, C], from single bytes."""
    b = np.asarray(raw, np.uint8).reshape(-1, BYTES[fmt]).astype(np.int64)
    v = sum(b[:, k] << (8 * k) for k in range(BYTES[fmt]))
    top = 1 << (BITS[fmt] - 1)
    return ((v ^ top) - top).reshape(-1, C)


def channel(raw, fmt, C, c):
    """Channel c as the f32 samples the kernels stage."""
    if fmt == "f32":
        return np.asarray(raw, np.uint8).view("<f4").reshape(-1, C)[:, c].astype(np.float32)
    v = integers(raw, fmt, C)[:, c]
    return v.astype(np.float32) * np.float32(2.0 ** -(BITS[fmt] - 1))        # s32: rounded to f32 once, then an exact scaling


def down_mix(raw, fmt, C):
    """The mono f32 signal of the header: integer formats, the exact sum over C * 2^(bits-1) (both exact in float64, the
    quotient rounded to f32); f32, the channels added in float64 in channel order, over C, rounded to f32."""
    if C == 1:
        return channel(raw, fmt, 1, 0)
    if fmt == "f32":
        x = np.asarray(raw, np.uint8).view("<f4").reshape(-1, C)
        acc = np.zeros(x.shape[0], np.float64)
        for c in range(C):
            acc += x[:, c].astype(np.float64)
        return (acc / C).astype(np.float32)
    s = integers(raw, fmt, C).sum(1)
    assert np.abs(s).max() <= 2 ** 53
    return (s.astype(np.float64) / float(C * 2 ** (BITS[fmt] - 1))).astype(np.float32)


def encode(y32, fmt):
    """f32 values [L, C] (or [L]) -> the bytes a kernel writes for them: s16 / s24 clip(rint(v * 2^(bits-1))), ties to even;
    f32 the bits."""
    y32 = np.asarray(y32, np.float32)
    if fmt == "f32":
        return pack(y32, "f32")
    top = 2.0 ** (BITS[fmt] - 1)
    return pack(np.clip(np.rint(y32.astype(np.float64) * top), -top, top - 1), fmt)
