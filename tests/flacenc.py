"""A small FLAC encoder for the tests (numpy only), written from RFC 9639.  Not part of the package: the package reads FLAC with
csrc/ww_flac_index.h (container, frame index, CRCs) and decodes it on the GPU (csrc/ww_flac.hip).

No independent FLAC implementation is available to the tests (no libFLAC, soundfile, ffmpeg or sox), so the oracle is exactness: every
file is built from known integer samples, and a decoder is right when it returns those integers (times 2^-(bps-1)) bit for bit.  The
encoder can be told which tool to use for every part of the format, so that the tests reach each case of the decoder:

* subframes: CONSTANT, VERBATIM, FIXED orders 0-4, LPC orders 1-32 with a chosen coefficient precision (and shift 0-15), wasted bits;
* residuals: Rice (4-bit parameter), Rice2 (5-bit), escape partitions (raw n-bit, n = 0 included), partition orders 0-8 (or the
  largest the block allows);
* channels: independent (1-8), left/side, side/right, mid/side (the side channel carries bps + 1 bits);
* frames: any block size (the coded sizes and explicit 8- / 16-bit sizes, a short last block), fixed or variable blocking, coded or
  explicit sample-rate and sample-size codes;
* stream: STREAMINFO with total_samples or 0, PADDING / APPLICATION / VORBIS_COMMENT / PICTURE-like blocks to skip, an ID3v2 tag in front.

`signal()` makes content for it: noise plus tones, with full-scale extremes so that side channels need all bps + 1 bits.
"""
from __future__ import annotations

import numpy as np

STEREO = {"independent": None, "left_side": 8, "side_right": 9, "mid_side": 10}


def _crc_tables():
    t8 = np.zeros(256, np.uint32)
    t16 = np.zeros(256, np.uint32)
    for b in range(256):
        c = b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) if c & 0x80 else (c << 1)
        t8[b] = c & 0xFF
        d = b << 8
        for _ in range(8):
            d = ((d << 1) ^ 0x8005) if d & 0x8000 else (d << 1)
        t16[b] = d & 0xFFFF
    return [int(x) for x in t8], [int(x) for x in t16]


_T8, _T16 = _crc_tables()


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data: bytes) -> int:
    c = 0
    t = _T16
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ t[(c >> 8) ^ b]
    return c


class BitWriter:
    """MSB-first: a list of (values, widths) chunks, packed with numpy."""

    def __init__(self):
        self.vals, self.widths = [], []

    def put(self, value: int, width: int):
        if width:
            self.vals.append(np.array([int(value) & ((1 << width) - 1)], np.uint64))
            self.widths.append(np.array([width], np.int64))

    def put_array(self, values, widths):
        values = np.asarray(values, np.int64)
        widths = np.broadcast_to(np.asarray(widths, np.int64), values.shape)
        keep = widths > 0
        mask = np.where(widths >= 64, -1, (np.int64(1) << np.minimum(widths, 63)) - 1)
        self.vals.append((values & mask)[keep].astype(np.uint64))
        self.widths.append(widths[keep].copy())

    def bits(self) -> int:
        return int(sum(int(w.sum()) for w in self.widths))

    def getbytes(self) -> bytes:
        if not self.vals:
            return b""
        v = np.concatenate(self.vals)
        w = np.concatenate(self.widths)
        total = int(w.sum())
        idx = np.repeat(np.arange(len(w)), w)
        starts = np.cumsum(w) - w
        pos = np.arange(total, dtype=np.int64) - starts[idx]
        shift = (w[idx] - 1 - pos).astype(np.uint64)
        bits = ((v[idx] >> shift) & np.uint64(1)).astype(np.uint8)
        pad = (-total) % 8
        if pad:
            bits = np.concatenate([bits, np.zeros(pad, np.uint8)])
        return np.packbits(bits).tobytes()


def _utf8(n: int) -> bytes:
    if n < 0x80:
        return bytes([n])
    for nbytes, lim in ((2, 1 << 11), (3, 1 << 16), (4, 1 << 21), (5, 1 << 26), (6, 1 << 31), (7, 1 << 36)):
        if n < lim:
            out = []
            for _ in range(nbytes - 1):
                out.append(0x80 | (n & 0x3F))
                n >>= 6
            lead = (0xFF00 >> nbytes) & 0xFF
            return bytes([lead | n] + out[::-1])
    raise ValueError("number too large")


def _signed_width(x) -> int:
    """Bits of the smallest two's complement field that holds every value of x."""
    x = np.asarray(x, np.int64)
    if x.size == 0:
        return 0
    hi, lo = int(x.max()), int(x.min())
    w = 1
    while not (-(1 << (w - 1)) <= lo and hi <= (1 << (w - 1)) - 1):
        w += 1
    return w if (hi or lo) else 0


def _fixed_residual(x, order):
    x = np.asarray(x, np.int64)
    if order == 0:
        return x.copy()
    r = x.copy()
    for _ in range(order):
        r = np.diff(r)
    return np.concatenate([x[:order], r])     # warm-up then the order-th difference (= the fixed predictor's residual)


def _lpc_coefs(x, order, precision):
    """Least-squares predictor, quantised to `precision` bits with a shift in 0..15."""
    x = np.asarray(x, np.float64)
    n = len(x)
    if n <= order:
        c = np.zeros(order)
    else:
        A = np.stack([x[order - 1 - j:n - 1 - j] for j in range(order)], axis=1)
        c, *_ = np.linalg.lstsq(A, x[order:], rcond=None)
    cmax = float(np.abs(c).max()) if c.size else 0.0
    lim = (1 << (precision - 1)) - 1
    shift = 15
    while shift > 0 and cmax * (1 << shift) > lim:
        shift -= 1
    q = np.clip(np.round(c * (1 << shift)), -lim - 1, lim).astype(np.int64)
    return q, shift


def _lpc_residual(x, q, shift):
    x = np.asarray(x, np.int64)
    order = len(q)
    n = len(x)
    pred = np.zeros(n - order, dtype=object)
    acc = np.zeros(n - order, np.int64)
    for j in range(order):
        acc = acc + q[j] * x[order - 1 - j:n - 1 - j]          # |acc| < 2^25 * 32 * 2^15 = 2^45: exact in int64
    pred = acc >> shift
    return np.concatenate([x[:order], x[order:] - pred])


def _rice_param(u, rice2):
    """Parameter for unsigned residuals u (Rice: 0..14, Rice2: 0..30) that keeps the unary part short."""
    kmax = 30 if rice2 else 14
    if u.size == 0:
        return 0
    m = float(u.mean())
    k = max(0, int(np.floor(np.log2(m + 1))) if m > 0 else 0)
    # the longest quotient must stay short (the encoder writes a quotient as one code of <= 64 bits)
    big = int(u.max())
    while k < kmax and (big >> k) > 40:
        k += 1
    if (big >> k) > 40:
        return None                                             # needs an escape partition
    return min(k, kmax)


def _residual(bw: BitWriter, res, bs, order, rice2, escape, porder):
    """res: the residual samples (bs - order of them)."""
    bw.put(1 if rice2 else 0, 2)
    if porder is None:
        porder = 0
        while porder < 8 and bs % (1 << (porder + 1)) == 0 and (bs >> (porder + 1)) >= order and (bs >> (porder + 1)) >= 16:
            porder += 1
    if porder and (bs % (1 << porder) or (bs >> porder) < order):
        raise ValueError(f"partition order {porder} does not fit a block of {bs} with predictor order {order}")
    bw.put(porder, 4)
    pbits, esc = (5, 31) if rice2 else (4, 15)
    per = bs >> porder
    pos = 0
    for p in range(1 << porder):
        cnt = per - order if p == 0 else per
        r = np.asarray(res[pos:pos + cnt], np.int64)
        pos += cnt
        u = np.where(r >= 0, r << 1, ((-r) << 1) - 1)
        k = None if escape else _rice_param(u, rice2)
        if k is None:
            nb = _signed_width(r)
            bw.put(esc, pbits)
            bw.put(nb, 5)
            if nb:
                bw.put_array(r, nb)
            continue
        bw.put(k, pbits)
        q = u >> k
        # q zeros and a one (one code of q + 1 bits), then the k low bits
        bw.put_array(np.stack([np.ones_like(u), u & ((1 << k) - 1)], axis=1).ravel(),
                     np.stack([q + 1, np.full_like(q, k)], axis=1).ravel())


def _subframe(bw: BitWriter, x, sbps, kind, order, precision, rice2, escape, porder, wasted_ok):
    x = np.asarray(x, np.int64)
    bs = len(x)
    wasted = 0
    if wasted_ok and np.any(x):
        while wasted < sbps - 1 and not np.any(x & ((1 << (wasted + 1)) - 1)):
            wasted += 1
    if kind == "auto":
        kind = "constant" if np.all(x == x[0]) else "fixed"
    if kind == "constant" and not np.all(x == x[0]):
        raise ValueError("constant subframe of a non-constant block")
    xs = x >> wasted
    w = sbps - wasted
    types = {"constant": 0, "verbatim": 1}
    if kind in types:
        t = types[kind]
    elif kind == "fixed":
        order = 2 if order is None else order
        order = min(order, bs)
        t = 8 + order
    elif kind == "lpc":
        order = 8 if order is None else order
        order = min(order, bs)
        t = 32 + order - 1
    else:
        raise ValueError(kind)
    bw.put(0, 1)
    bw.put(t, 6)
    if wasted:
        bw.put(1, 1)
        bw.put(1, wasted)          # wasted - 1 zeros, then a one
    else:
        bw.put(0, 1)
    if kind == "constant":
        bw.put(int(xs[0]), w)
    elif kind == "verbatim":
        bw.put_array(xs, w)
    elif kind == "fixed":
        r = _fixed_residual(xs, order)
        bw.put_array(xs[:order], w)
        _residual(bw, r[order:], bs, order, rice2, escape, porder)
    else:
        q, shift = _lpc_coefs(xs, order, precision)
        r = _lpc_residual(xs, q, shift)
        bw.put_array(xs[:order], w)
        bw.put(precision - 1, 4)
        bw.put(shift, 5)
        bw.put_array(q, precision)
        _residual(bw, r[order:], bs, order, rice2, escape, porder)


_BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
_SR_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
_SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


def _frame(x, rate, bps, number, blocking, chan, kind, order, precision, rice2, escape, porder, wasted, explicit_bs, explicit_rate,
           bps_from_streaminfo):
    bs, nch = x.shape
    hdr = bytearray([0xFF, 0xF8 | blocking])
    if explicit_bs or bs not in _BS_CODES:
        bcode, bextra = (6, bytes([bs - 1])) if bs <= 256 else (7, (bs - 1).to_bytes(2, "big"))
    else:
        bcode, bextra = _BS_CODES[bs], b""
    if explicit_rate:
        if rate % 1000 == 0 and rate // 1000 < 256:
            scode, sextra = 12, bytes([rate // 1000])
        elif rate < 65536:
            scode, sextra = 13, rate.to_bytes(2, "big")
        else:
            scode, sextra = 14, (rate // 10).to_bytes(2, "big")
    else:
        scode, sextra = _SR_CODES.get(rate, 0), b""
    cacode = STEREO[chan] if chan != "independent" else nch - 1
    sscode = 0 if bps_from_streaminfo else _SS_CODES.get(bps, 0)
    hdr += bytes([(bcode << 4) | scode, (cacode << 4) | (sscode << 1)])
    hdr += _utf8(number) + bextra + sextra
    hdr.append(crc8(bytes(hdr)))
    bw = BitWriter()
    L, R = (x[:, 0], x[:, 1]) if nch == 2 else (None, None)
    if chan == "left_side":
        chans = [(L, bps), (L - R, bps + 1)]
    elif chan == "side_right":
        chans = [(L - R, bps + 1), (R, bps)]
    elif chan == "mid_side":
        chans = [((L + R) >> 1, bps), (L - R, bps + 1)]
    else:
        chans = [(x[:, c], bps) for c in range(nch)]
    for c, (v, w) in enumerate(chans):
        k = kind[c % len(kind)] if isinstance(kind, (list, tuple)) else kind
        _subframe(bw, v, w, k, order, precision, rice2, escape, porder, wasted)
    body = bytes(hdr) + bw.getbytes()
    return body + crc16(body).to_bytes(2, "big")


def metadata_block(btype: int, payload: bytes, last: bool = False) -> bytes:
    return bytes([(0x80 if last else 0) | btype]) + len(payload).to_bytes(3, "big") + payload


def id3v2(size: int = 300, footer: bool = False) -> bytes:
    """An ID3v2.4 tag of `size` payload bytes (syncsafe size)."""
    ss = bytes([(size >> 21) & 0x7F, (size >> 14) & 0x7F, (size >> 7) & 0x7F, size & 0x7F])
    body = b"TIT2" + (size - 10).to_bytes(4, "big") + b"\x00\x00" + b"\x03" + b"x" * (size - 11)
    tag = b"ID3\x04\x00" + bytes([0x10 if footer else 0]) + ss + body
    if footer:
        tag += b"3DI\x04\x00\x10" + ss
    return tag


def encode(samples, rate: int, bps: int, blocksize=4096, stereo: str = "independent", subframe="auto", order=None,
           precision: int = 12, rice2: bool = False, escape: bool = False, partition_order=None, wasted: bool = True,
           explicit_blocksize: bool = False, explicit_rate: bool = False, bps_from_streaminfo: bool = False, variable=None,
           total_samples_zero: bool = False, metadata=(), id3: int = 0) -> bytes:
    """samples: int [n] or [n, ch] in the signed range of `bps` bits -> the bytes of a .flac file.

    blocksize: frame size (the last frame is shorter when n is not a multiple); variable: a list of block sizes (variable blocking,
    sample numbers in the headers) that must sum to n; subframe: "auto" | "constant" | "verbatim" | "fixed" | "lpc" (or a list per
    channel); order: the FIXED / LPC order; precision: LPC coefficient bits (1..15); partition_order: None = the largest that fits (<= 8);
    metadata: (type, payload) blocks written after STREAMINFO; id3: size of an ID3v2 tag in front (0 = none)."""
    x = np.asarray(samples, np.int64)
    if x.ndim == 1:
        x = x[:, None]
    n, nch = x.shape
    if not (4 <= bps <= 32) or not (1 <= nch <= 8):
        raise ValueError("bps 4..32, 1..8 channels")
    lim = 1 << (bps - 1)
    if x.size and (x.min() < -lim or x.max() >= lim):
        raise ValueError("samples outside the bit width")
    if stereo != "independent" and nch != 2:
        raise ValueError("stereo modes need two channels")
    sizes = list(variable) if variable is not None else [blocksize] * (n // blocksize) + ([n % blocksize] if n % blocksize else [])
    if sum(sizes) != n:
        raise ValueError("block sizes must sum to the sample count")
    frames = []
    pos = 0
    for i, bs in enumerate(sizes):
        number = pos if variable is not None else i
        frames.append(_frame(x[pos:pos + bs], rate, bps, number, 1 if variable is not None else 0, stereo, subframe, order, precision,
                             rice2, escape, partition_order, wasted, explicit_blocksize, explicit_rate, bps_from_streaminfo))
        pos += bs
    full = sizes[:-1] if len(sizes) > 1 else sizes
    if variable is not None:
        min_bs, max_bs = max(16, min(full)), max(sizes)
    else:
        min_bs = max_bs = max(16, blocksize)
    total = 0 if total_samples_zero else n
    si = bytearray()
    si += min_bs.to_bytes(2, "big") + max_bs.to_bytes(2, "big") + (0).to_bytes(3, "big") + (0).to_bytes(3, "big")
    packed = (rate << 44) | ((nch - 1) << 41) | ((bps - 1) << 36) | total
    si += packed.to_bytes(8, "big") + bytes(16)
    blocks = [(0, bytes(si))] + list(metadata)
    out = bytearray(id3v2(id3) if id3 else b"")
    out += b"fLaC"
    for k, (t, payload) in enumerate(blocks):
        out += metadata_block(t, payload, last=k == len(blocks) - 1)
    for f in frames:
        out += f
    return bytes(out)


def signal(n: int, channels: int, bps: int, seed: int = 0, extremes: bool = True, correlated: bool = True):
    """Noise plus tones at `bps` bits, [n, channels] int64; with extremes, a few samples sit at the two ends of the range (left at the
    top and right at the bottom in the same frame, so a side channel spans bps + 1 bits)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    hi = (1 << (bps - 1)) - 1
    lo = -(1 << (bps - 1))
    base = 0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + 0.3)
    out = np.empty((n, channels), np.int64)
    for c in range(channels):
        tone = base if correlated else np.sin(2 * np.pi * (300.0 + 170 * c) * t)
        v = tone * (0.7 if correlated else 0.5) + 0.05 * rng.standard_normal(n)
        out[:, c] = np.clip(np.round(v * hi), lo, hi)
    if extremes and n >= 8:
        k = rng.integers(0, n, size=4)
        out[k[0], :] = hi
        out[k[1], :] = lo
        if channels >= 2:
            out[k[2], 0], out[k[2], 1] = hi, lo
            out[k[3], 0], out[k[3], 1] = lo, hi
    return out


def wav_bytes(samples, rate: int, bps: int) -> bytes:
    """The PCM WAV of the same integers: u8 for 8 bits, s16 for 12 / 16 (12-bit samples shifted left by 4), s24 for 20 / 24 (20-bit
    shifted by 4) -- soundfile's float for both files is then x * 2^-(bps-1)."""
    import struct
    x = np.asarray(samples, np.int64)
    if x.ndim == 1:
        x = x[:, None]
    ch = x.shape[1]
    if bps == 8:
        raw, width = (x + 128).astype(np.uint8).tobytes(), 1
    elif bps <= 16:
        raw, width = (x << (16 - bps)).astype("<i2").tobytes(), 2
    else:
        v = (x << (24 - bps)).astype("<i4").reshape(-1)
        raw, width = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes(), 3
    fmt = struct.pack("<HHIIHH", 1, ch, rate, rate * ch * width, ch * width, 8 * width)
    return b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(raw)) + raw


def first_frame_offset(data: bytes) -> int:
    """Byte offset of the first frame of a FLAC file written by encode()."""
    pos = 0
    if data[:3] == b"ID3":
        pos = 10 + ((data[6] << 21) | (data[7] << 14) | (data[8] << 7) | data[9]) + (10 if data[5] & 0x10 else 0)
    pos += 4
    while True:
        last, n = data[pos] & 0x80, int.from_bytes(data[pos + 1:pos + 4], "big")
        pos += 4 + n
        if last:
            return pos
