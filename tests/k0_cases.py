"""Shared by tests/test_host_decode_stages.py, tests/test_gpu_decode_stages.py and scripts/decode_stage_errors.py: the rates, frame counts,
crops and signals of the K0 stage checks, K0's own float32 taps, and the descriptor packing.  No test lives here."""
import ctypes as C

import numpy as np

from oracle import decode_oracle as do
from wakeword_jupyterlab_amd import _native as nat

RATES = (1000, 6000, 7350, 8000, 11025, 12000, 15999, 22050, 37800, 44100, 48000, 88200, 96000, 192000, 384000)
ROW_LENS = (4000, 16000)
# csrc/ww_decode.hip's LDS budget: they choose the CASES (block seams, which kernel runs), never an expected value
K_RS_TAPS, K_RS_SPAN = 8960, 7168

_TAPS = {}


def taps(sr):
    """(float32 taps as K0 uploads them, up, down, half_len) from ww_resample_taps_host."""
    if sr not in _TAPS:
        up, dn, hl = C.c_int32(), C.c_int32(), C.c_int32()
        n = nat.lib.ww_resample_taps_host(sr, None, 0, C.byref(up), C.byref(dn), C.byref(hl))
        assert n == 2 * hl.value + 1 and n == 20 * max(up.value, dn.value) + 1
        t = np.zeros(n, np.float32)
        assert nat.lib.ww_resample_taps_host(sr, t.ctypes.data, n, None, None, None) == n
        t.setflags(write=False)
        _TAPS[sr] = (t, up.value, dn.value, hl.value)
    return _TAPS[sr]


def in_lds(sr):
    _, up, down, hl = taps(sr)
    lh = 2 * hl + 1
    return lh <= K_RS_TAPS and lh // up + 8 < K_RS_SPAN // 2


def blk(sr):
    """Outputs per block of resample_lds_kernel (2048 for the direct form, which has no blocks: the seam cases then are just more crops)."""
    _, up, down, hl = taps(sr)
    if not in_lds(sr):
        return 2048
    return int(min(2048, max(1, (K_RS_SPAN - (2 * hl + 1) // up - 8) * up // down)))


def n_out_of(n_in, sr):
    _, up, down, _ = taps(sr)
    return -(-n_in * up // down)


def frames_for(n_out, sr):
    """The smallest frame count with at least n_out outputs (exactly n_out wherever the rate can give it: up <= down)."""
    _, up, down, _ = taps(sr)
    n = (n_out - 1) * down // up + 1
    while n_out_of(n, sr) < n_out:
        n += 1
    while n > 1 and n_out_of(n - 1, sr) >= n_out:
        n -= 1
    return n


def frame_counts(sr):
    _, up, down, hl = taps(sr)
    lh = 2 * hl + 1
    counts = [1, 2, 3, lh // up - 1, lh // up + 1]
    if sr == 15999:                                              # 320,001 taps: 200 frames at most
        counts.append(200)
    else:
        for row_len in ROW_LENS:
            counts += [frames_for(row_len + k, sr) for k in (-1, 0, 1)]
        counts.append(frames_for(3 * blk(sr) + 17, sr))
    return sorted({c for c in counts if c >= 1})


def crops(n_out, sr, row_len):
    b = blk(sr)
    return sorted({c for c in (0, 1, b - 1, b, b + 1, n_out - row_len) if 0 <= c < max(n_out, 1)})


def noise_s16(n, seed):
    """Full-scale uniform noise, first frame +full-scale, last frame -full-scale (mono S16 codes)."""
    v = np.random.default_rng(seed).integers(-32768, 32768, size=n, dtype=np.int64)
    v[0] = 32767
    v[-1] = -32768
    return v


def to_bytes(codes, fmt):
    c = np.asarray(codes).reshape(-1)
    if fmt == do.FMT_S24:
        u = (c.astype(np.int64) & 0xFFFFFF)
        return np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255], 1).astype(np.uint8).reshape(-1)
    dt = {do.FMT_S16: "<i2", do.FMT_S32: "<i4", do.FMT_U8: "u1", do.FMT_F32: "<f4", do.FMT_F64: "<f8"}[fmt]
    return np.frombuffer(c.astype(dt).tobytes(), np.uint8)


class Pack:
    """Raw bytes of many in-memory files in one buffer (each at a 16-byte boundary plus `shift`) and the descriptors that point at them."""

    def __init__(self):
        self.chunks, self.size, self.descs = [], 0, []

    def add_bytes(self, b, shift=0):
        pad = (-self.size) % 16 + shift
        self.chunks.append(np.zeros(pad, np.uint8))
        off = self.size + pad
        self.chunks.append(np.asarray(b, np.uint8))
        self.size = off + len(b)
        return off

    def desc(self, off, n_frames, channels, sr, fmt, crop_start=0):
        if fmt != nat.FMT_FLAC:
            assert off + n_frames * channels * do.SAMPLE_BYTES[fmt] <= self.size      # K0 reads n_frames frames from byte_offset
        self.descs.append((off, n_frames, channels, sr, fmt, crop_start))
        return len(self.descs) - 1

    def raw(self):
        r = np.concatenate(self.chunks) if self.chunks else np.zeros(0, np.uint8)
        return np.concatenate([r, np.zeros(16, np.uint8)])
