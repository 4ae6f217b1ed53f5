"""NumPy restatement (int64 throughout) of the baseline JPEG decoder of csrc/jpeg.hip: Huffman decode, libjpeg's "islow" integer
inverse DCT, libjpeg-turbo's "fancy" chroma upsampling and its YCbCr -> RGB conversion.  It is the oracle of the kernels, and
tests/test_jpeg_host.py pins it to Pillow byte for byte.  The markers are read by avsep_amd.jpeg.probe; everything from the
entropy-coded bytes onwards is restated here."""
import numpy as np

# natural (row-major) index of zig-zag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

CONST_BITS, PASS1_BITS = 13, 2


def idct_1d(d, shift):
    """One pass of the islow inverse DCT over d[0..7] -> the 8 outputs, each (x + 2^(shift-1)) >> shift.  ``d`` holds anything
    that adds, subtracts, multiplies by an int and shifts (NumPy int64 arrays here; the linear forms of ``arith_bound``).  The
    order of operations is the kernel's (csrc/jpeg_parts.h: jp_idct_1d)."""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (d[0] + d[4]) << CONST_BITS
    tmp1 = (d[0] - d[4]) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069, z4 * -3196
    z3 = z3 + z5
    z4 = z4 + z5
    tmp0 = tmp0 + (z1 + z3)
    tmp1 = tmp1 + (z2 + z4)
    tmp2 = tmp2 + (z2 + z3)
    tmp3 = tmp3 + (z1 + z4)
    half = 1 << (shift - 1)
    return [(v + half) >> shift for v in (tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0,
                                          tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3)]


class _Form:
    """A linear form over the 8 inputs of a pass plus a constant, for ``arith_bound``: every value ``idct_1d`` forms is one of
    these, and ``seen`` collects the largest sum of absolute coefficients (and constant) any of them reaches."""
    seen = [0, 0]

    def __init__(self, c, k=0):
        self.c, self.k = np.asarray(c, dtype=object), k
        _Form.seen[0] = max(_Form.seen[0], int(sum(abs(int(v)) for v in self.c)))
        _Form.seen[1] = max(_Form.seen[1], abs(int(k)))

    def __add__(self, o):
        return _Form(self.c + o.c, self.k + o.k) if isinstance(o, _Form) else _Form(self.c, self.k + o)

    def __sub__(self, o):
        return _Form(self.c - o.c, self.k - o.k)

    def __mul__(self, m):
        return _Form(self.c * m, self.k * m)

    def __lshift__(self, s):
        return _Form(self.c * (1 << s), self.k * (1 << s))

    def __rshift__(self, s):         # the final descale: the caller reads ``seen`` before it matters
        return self


def pass_gain():
    """(G, R): every value a pass forms from inputs |d| <= M is at most G * M + R in magnitude, and G is reached (all eight inputs
    at +-M with the signs of the form's coefficients)."""
    _Form.seen = [0, 0]
    idct_1d([_Form([int(i == j) for j in range(8)]) for i in range(8)], 1)
    return _Form.seen[0], _Form.seen[1]


def arith_bound():
    """The largest M = |coefficient * quantiser| for which no value of either pass can leave int32.
    Pass 1: every value is at most G*M + 2^10.  Its outputs are at most M1 = ((G*M + 2^10) >> 11) + 1.  Pass 2: G*M1 + 2^17
    must stay below 2^31."""
    G, _ = pass_gain()
    M = 0
    lim = (1 << 31) - 1
    while True:
        n = M + 1
        m1 = ((G * n + (1 << 10)) >> 11) + 1
        if G * n + (1 << 10) > lim or G * m1 + (1 << 17) > lim:
            return M
        M = n


def huffman_codes(counts, values):
    """{(length, code): value} of a table given as libjpeg's BITS counts [16] and HUFFVAL."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(int(counts[length - 1])):
            out[(length, code)] = int(values[k])
            code, k = code + 1, k + 1
        code <<= 1
    return out


class _Bits:
    def __init__(self, data):
        raw = bytes(data).replace(b"\xff\x00", b"\xff")
        self.bits = np.unpackbits(np.frombuffer(raw, dtype=np.uint8)).tolist()
        self.at = 0

    def take(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bits[self.at]
            self.at += 1
        return v

    def symbol(self, codes):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bits[self.at]
            self.at += 1
            if (length, code) in codes:
                return codes[(length, code)]
        raise ValueError("no Huffman code within 16 bits")


def _extend(v, s):
    return v - ((1 << s) - 1) if s and v < (1 << (s - 1)) else v


def split_segments(data, begin, end):
    """The entropy-coded segments of data[begin:end]: cut at every RSTn marker."""
    a = np.frombuffer(data, dtype=np.uint8)[begin:end]
    at = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7)) if len(a) > 1 else np.zeros(0, dtype=np.int64)
    cuts = [0] + [int(p) + 2 for p in at]
    ends = [int(p) for p in at] + [len(a)]
    return [(begin + b, begin + e) for b, e in zip(cuts, ends)]


def geometry(info):
    """(hs, vs, mcux, mcuy, per component (blocks wide, blocks high, h, v)) of a probed file."""
    n = len(info.components)
    hs, vs = (info.components[0][1], info.components[0][2]) if n == 3 else (1, 1)
    mcux, mcuy = -(-info.W // (8 * hs)), -(-info.H // (8 * vs))
    comps = [(mcux * hs, mcuy * vs, hs, vs)] + [(mcux, mcuy, 1, 1)] * (n - 1)
    return hs, vs, mcux, mcuy, comps


def coefficients(info, data):
    """The quantised coefficients of every block, natural order -> per component int64 [blocks high, blocks wide, 64]."""
    hs, vs, mcux, mcuy, comps = geometry(info)
    out = [np.zeros((bh, bw, 64), dtype=np.int64) for bw, bh, _, _ in comps]
    dc = [huffman_codes(*info.huffman[(0, info.scan[c][0])]) for c in range(len(comps))]
    ac = [huffman_codes(*info.huffman[(1, info.scan[c][1])]) for c in range(len(comps))]
    segments = split_segments(data, info.data_begin, info.data_end)
    per = info.restart if info.restart else mcux * mcuy
    for s, (b, e) in enumerate(segments):
        bits, pred = _Bits(data[b:e]), [0] * len(comps)
        for m in range(s * per, min((s + 1) * per, mcux * mcuy)):
            my, mx = divmod(m, mcux)
            for c, (_, _, h, v) in enumerate(comps):
                for by in range(v):
                    for bx in range(h):
                        blk = out[c][my * v + by, mx * h + bx]
                        size = bits.symbol(dc[c])
                        pred[c] += _extend(bits.take(size), size)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(ac[c])
                            r, size = rs >> 4, rs & 15
                            if size == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[ZIGZAG[k]] = _extend(bits.take(size), size)
                            k += 1
    return out


def planes(info, coefs):
    """Dequantise and inverse DCT -> per component a uint8 plane of the padded size [8 * blocks high, 8 * blocks wide]."""
    out = []
    for c, co in enumerate(coefs):
        q = np.zeros(64, dtype=np.int64)
        q[ZIGZAG] = np.asarray(info.qtables[info.components[c][3]], dtype=np.int64)
        d = (co * q).reshape(co.shape[0], co.shape[1], 8, 8)
        cols = idct_1d([d[:, :, i, :] for i in range(8)], CONST_BITS - PASS1_BITS)              # [row i][bh, bw, col]
        w = np.stack(cols, axis=2)                                                               # [bh, bw, row, col]
        rows = idct_1d([w[:, :, :, j] for j in range(8)], CONST_BITS + PASS1_BITS + 3)
        px = np.clip(np.stack(rows, axis=3) + 128, 0, 255)
        out.append(px.transpose(0, 2, 1, 3).reshape(co.shape[0] * 8, co.shape[1] * 8).astype(np.uint8))
    return out


def upsample(p, hs, vs, H, W):
    """libjpeg-turbo's fancy upsampling of one chroma plane (padded, uint8) to [H, W], int64."""
    ch, cw = -(-H // vs), -(-W // hs)
    s = p[:ch, :cw].astype(np.int64)
    if hs == 1 and vs == 1:
        return s
    if cw <= 2:                                      # replicated, not filtered
        return np.repeat(np.repeat(s, vs, axis=0), hs, axis=1)[:H, :W]
    if vs == 1:
        left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        even, odd = (3 * s + left + 1) >> 2, (3 * s + right + 2) >> 2
        even[:, 0], odd[:, -1] = s[:, 0], s[:, -1]
        out = np.empty((ch, 2 * cw), dtype=np.int64)
        out[:, 0::2], out[:, 1::2] = even, odd
        return out[:H, :W]
    above, below = np.concatenate([s[:1], s[:-1]], axis=0), np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    for parity, other in ((0, above), (1, below)):
        this = 3 * s + other
        last, nxt = np.concatenate([this[:, :1], this[:, :-1]], axis=1), np.concatenate([this[:, 1:], this[:, -1:]], axis=1)
        even, odd = (3 * this + last + 8) >> 4, (3 * this + nxt + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * this[:, 0] + 8) >> 4, (4 * this[:, -1] + 7) >> 4
        out[parity::2, 0::2], out[parity::2, 1::2] = even, odd
    return out[:H, :W]


def _fix(v):
    return int(v * 65536 + 0.5)


def colour(info, pl):
    """Component planes -> uint8 [H, W, 3]."""
    H, W = info.H, info.W
    y = pl[0][:H, :W].astype(np.int64)
    if len(pl) == 1:
        return np.stack([y, y, y], axis=2).astype(np.uint8)
    hs, vs = geometry(info)[:2]
    cb, cr = upsample(pl[1], hs, vs, H, W) - 128, upsample(pl[2], hs, vs, H, W) - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(info, data):
    """-> (uint8 [H, W, 3], the coefficients of ``coefficients``)."""
    co = coefficients(info, data)
    return colour(info, planes(info, co)), co


def workspace(info, coefs):
    """The coefficients in the order of the kernels' workspace: component after component, each [blocks high][blocks wide][64]
    -> int16 [blocks * 64]."""
    return np.concatenate([c.reshape(-1) for c in coefs]).astype(np.int16)
