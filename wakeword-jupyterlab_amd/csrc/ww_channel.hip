// Microphone-channel augmentation: a clip through up to 8 second-order sections (RBJ cookbook forms at 16 kHz:
// high-pass, low shelf, up to 4 peaks, high shelf, low-pass) and an optional peak-preserving tanh saturator.
//   channel_draw_kernel   one thread per (clip, slot): the clip's record drawn from SpecAugment's counter-based generator
//   channel_kernel        one workgroup of 256 threads per clip: the record (read, or drawn by the same functions), the clip in LDS,
//                         every section as a chunked scan over the 256 threads, the peak, the saturator, one store per sample
// An IIR is sequential in time, but its recurrence is linear: thread t owns the chunk [t L, (t + 1) L) of the clip, L = ceil(N / 256)
// (the clip is zero-padded to 256 L in LDS; the pad is never stored).  Per section that is not the identity:
//   1  every thread runs its chunk with the true x history and y history 0 and keeps z = (y[L-1], y[L-2]);
//   2  the true end states are s(t) = z(t) + M s(t-1), M = A^L, A = [[-a1, -a2], [1, 0]]: a Hillis-Steele scan over the 256 threads
//      with M, M^2, M^4 ... M^128 -- a thread only ever pulls from lower threads, so what a NaN at sample k reaches is k and later;
//   3  every thread reruns its chunk from s(t-1) and writes the section's output over its input in LDS, rounded to float32.
// The recurrences, M and the scan are float64 (5 fused multiply-adds per sample and pass); only a section's output is rounded, so the
// result is closer to the float64 recursion than a float32 recursion run sample by sample is.
// LDS: chunk t starts at float t (L | 1): an odd stride, so the 32 lanes of a ds_read_b32 group hit 32 banks.  256 x 65 floats at
// N = 16,383 (66,560 B) + 2 x 256 float64 pairs for the scan + the record and the peak partials: two workgroups per CU.
// Each sample is read from global memory once and written once; a clip whose record is "off" is left alone in place and copied out of place.
#include "ww_internal.h"

namespace ww {

// no contraction in this file: the record arithmetic is plain IEEE float64 operation by operation (what tests/channel_ref.py restates);
// the recurrences name their fused multiply-adds
#pragma clang fp contract(off)

constexpr int kChanThreads = 256;
constexpr int kChanWaves = kChanThreads / 64;
constexpr int kChanSlots = WW_CHANNEL_SECTIONS;         // 8 sections of 5 coefficients
constexpr int kChanRecord = WW_CHANNEL_RECORD_F32;      // 48 float32: 8 x [b0 b1 b2 a1 a2], d, 7 zeros
constexpr int kChanMaxChunk = 64;                       // ceil(16383 / 256)
constexpr int kChanMaxStride = kChanMaxChunk | 1;
constexpr double kChanFs = 16000.0;

__device__ __forceinline__ uint64_t chan_fmix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// Word j of clip c: SpecAugment's generator (ww_specaug.hip), so a clip's record does not depend on n.
__device__ __forceinline__ uint64_t chan_word(uint64_t seed, int64_t c, int j) {
    return chan_fmix64(seed + 0x9E3779B97F4A7C15ull * (32ull * uint64_t(c) + uint64_t(j) + 1ull));
}
__device__ __forceinline__ bool chan_on(uint64_t seed, int64_t c, int j, float p) {
    return float(uint32_t(chan_word(seed, c, j) >> 40)) * (1.0f / 16777216.0f) < p;
}
// 53 bits in [0, 1)
__device__ __forceinline__ double chan_u(uint64_t seed, int64_t c, int j) {
    return double(chan_word(seed, c, j) >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ double chan_uniform(uint64_t seed, int64_t c, int j, float lo, float hi) {
    return double(lo) + chan_u(seed, c, j) * (double(hi) - double(lo));
}
__device__ __forceinline__ double chan_log_uniform(uint64_t seed, int64_t c, int j, float lo, float hi) {
    return double(lo) * pow(double(hi) / double(lo), chan_u(seed, c, j));
}

// The generator's table: j = 0 the clip at all; then per slot [on, f, (gain dB, (Q))]
//   high-pass 1, 2    low shelf 3, 4, 5    peak i 6 + 4 i .. 9 + 4 i    high shelf 22, 23, 24    low-pass 25, 26    drive 27, 28
// Slot `slot` of clip c as 5 float32 [b0, b1, b2, a1, a2] / a0, computed in float64 and rounded once.
__device__ __forceinline__ void channel_section(const ww_channel_config& g, uint64_t seed, int64_t c, int slot, float (&out)[5]) {
    out[0] = 1.f; out[1] = 0.f; out[2] = 0.f; out[3] = 0.f; out[4] = 0.f;
    if (!chan_on(seed, c, 0, g.prob)) return;
    constexpr double kQ = 0.70710678118654752440;       // 1 / sqrt(2): both passes and the shelf slope
    int kind;                                           // 0 high-pass, 1 low-pass, 2 peak, 3 low shelf, 4 high shelf
    double f, db = 0.0, q = kQ;
    if (slot == 0) {
        if (!chan_on(seed, c, 1, g.highpass_prob)) return;
        kind = 0; f = chan_log_uniform(seed, c, 2, g.highpass_lo, g.highpass_hi);
    } else if (slot == 1) {
        if (!chan_on(seed, c, 3, g.low_shelf_prob)) return;
        kind = 3; f = chan_log_uniform(seed, c, 4, g.low_shelf_lo, g.low_shelf_hi);
        db = chan_uniform(seed, c, 5, -g.shelf_db, g.shelf_db);
    } else if (slot < 6) {
        const int i = slot - 2, j = 6 + 4 * i;
        if (i >= g.peaks || !chan_on(seed, c, j, g.peak_prob)) return;
        kind = 2; f = chan_log_uniform(seed, c, j + 1, g.peak_lo, g.peak_hi);
        db = chan_uniform(seed, c, j + 2, -g.peak_db, g.peak_db);
        q = chan_log_uniform(seed, c, j + 3, g.peak_q_lo, g.peak_q_hi);
    } else if (slot == 6) {
        if (!chan_on(seed, c, 22, g.high_shelf_prob)) return;
        kind = 4; f = chan_log_uniform(seed, c, 23, g.high_shelf_lo, g.high_shelf_hi);
        db = chan_uniform(seed, c, 24, -g.shelf_db, g.shelf_db);
    } else {
        if (!chan_on(seed, c, 25, g.lowpass_prob)) return;
        kind = 1; f = chan_log_uniform(seed, c, 26, g.lowpass_lo, g.lowpass_hi);
    }
    const double w0 = 2.0 * 3.14159265358979323846 * f / kChanFs;
    const double cs = cos(w0), alpha = sin(w0) / (2.0 * q);
    double b0, b1, b2, a0, a1, a2;
    if (kind == 0) {
        b0 = (1.0 + cs) / 2.0; b1 = -(1.0 + cs); b2 = b0;
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
    } else if (kind == 1) {
        b0 = (1.0 - cs) / 2.0; b1 = 1.0 - cs; b2 = b0;
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
    } else {
        const double A = pow(10.0, db / 40.0);
        if (kind == 2) {
            b0 = 1.0 + alpha * A; b1 = -2.0 * cs; b2 = 1.0 - alpha * A;
            a0 = 1.0 + alpha / A; a1 = -2.0 * cs; a2 = 1.0 - alpha / A;
        } else {
            const double t = 2.0 * sqrt(A) * alpha, ap = A + 1.0, am = A - 1.0;
            if (kind == 3) {
                b0 = A * (ap - am * cs + t); b1 = 2.0 * A * (am - ap * cs); b2 = A * (ap - am * cs - t);
                a0 = ap + am * cs + t; a1 = -2.0 * (am + ap * cs); a2 = ap + am * cs - t;
            } else {
                b0 = A * (ap + am * cs + t); b1 = -2.0 * A * (am + ap * cs); b2 = A * (ap + am * cs - t);
                a0 = ap - am * cs + t; a1 = 2.0 * (am - ap * cs); a2 = ap - am * cs - t;
            }
        }
    }
    out[0] = float(b0 / a0); out[1] = float(b1 / a0); out[2] = float(b2 / a0); out[3] = float(a1 / a0); out[4] = float(a2 / a0);
}

__device__ __forceinline__ float channel_drive(const ww_channel_config& g, uint64_t seed, int64_t c) {
    if (!chan_on(seed, c, 0, g.prob) || !chan_on(seed, c, 27, g.drive_prob)) return 0.f;
    return float(chan_uniform(seed, c, 28, g.drive_lo, g.drive_hi));
}

// Thread s of the first 8 (and thread 8 for d and the zeros) writes its part of clip c's record to rec[48].
__device__ __forceinline__ void channel_draw_part(const ww_channel_config& g, uint64_t seed, int64_t c, int part, float* rec) {
    if (part < kChanSlots) {
        float co[5];
        channel_section(g, seed, c, part, co);
#pragma unroll
        for (int k = 0; k < 5; ++k) rec[5 * part + k] = co[k];
    } else if (part == kChanSlots) {
        rec[5 * kChanSlots] = channel_drive(g, seed, c);
        for (int k = 5 * kChanSlots + 1; k < kChanRecord; ++k) rec[k] = 0.f;
    }
}

__global__ __launch_bounds__(kChanThreads) void channel_draw_kernel(float* __restrict__ records, int64_t n, uint64_t seed, ww_channel_config g) {
    const int64_t i = int64_t(blockIdx.x) * kChanThreads + threadIdx.x;       // 16 threads per clip, 9 of them at work
    const int64_t c = i >> 4;
    if (c >= n) return;
    channel_draw_part(g, seed, c, int(i & 15), records + c * kChanRecord);
}

__global__ __launch_bounds__(kChanThreads) void channel_kernel(const float* in, float* out, int N, int L, uint32_t l_recip, int64_t row_stride,
                                                               const float* __restrict__ records, uint64_t seed, ww_channel_config g) {
    __shared__ float clip[kChanThreads * kChanMaxStride];
    __shared__ double2 scan[2][kChanThreads];
    __shared__ float rec[kChanRecord];
    __shared__ float wave_peak[kChanWaves];
    const int t = threadIdx.x;
    const int64_t c = blockIdx.x;
    if (records) {
        if (t < kChanRecord) rec[t] = records[c * kChanRecord + t];
    } else {
        channel_draw_part(g, seed, c, t, rec);
    }
    __syncthreads();
    const float d = rec[5 * kChanSlots];
    unsigned active = 0;
#pragma unroll
    for (int s = 0; s < kChanSlots; ++s) {
        const float* co = rec + 5 * s;
        if (!(co[0] == 1.f && co[1] == 0.f && co[2] == 0.f && co[3] == 0.f && co[4] == 0.f)) active |= 1u << s;
    }
    const float* src = in + c * row_stride;
    float* dst = out + c * row_stride;
    if (active == 0 && d == 0.f) {                      // "off": in place neither read nor written, out of place the same bits
        if (in != out)
            for (int i = t; i < N; i += kChanThreads) dst[i] = src[i];
        return;
    }
    const int stride = L | 1;
    // sample i lives at (i / L) stride + i % L; i < 256 L <= 16384 and L <= 64, so the reciprocal multiply (floor(2^32 / L) + 1) is exact
    for (int k = 0; k < L; ++k) {
        const int i = t + kChanThreads * k;
        const int q = int(__umulhi(uint32_t(i), l_recip));
        clip[q * stride + (i - q * L)] = i < N ? src[i] : 0.f;
    }
    __syncthreads();
    float* mine = clip + t * stride;
    for (int s = 0; s < kChanSlots; ++s) {
        if (!((active >> s) & 1u)) continue;            // uniform over the workgroup
        const double b0 = double(rec[5 * s]), b1 = double(rec[5 * s + 1]), b2 = double(rec[5 * s + 2]);
        const double a1 = double(rec[5 * s + 3]), a2 = double(rec[5 * s + 4]);
        double x1 = 0.0, x2 = 0.0;                      // the two inputs before the chunk (L >= 16)
        if (t > 0) { x1 = double(mine[-stride + L - 1]); x2 = double(mine[-stride + L - 2]); }
        const double x1_0 = x1, x2_0 = x2;
        double y1 = 0.0, y2 = 0.0;
        for (int i = 0; i < L; ++i) {
            const double x = double(mine[i]);
            const double y = fma(-a1, y1, fma(-a2, y2, fma(b0, x, fma(b1, x1, b2 * x2))));
            x2 = x1; x1 = x; y2 = y1; y1 = y;
        }
        // M = A^L by binary powers, the same in every thread
        double m00 = 1.0, m01 = 0.0, m10 = 0.0, m11 = 1.0, p00 = -a1, p01 = -a2, p10 = 1.0, p11 = 0.0;
        for (int e = L; e > 0; e >>= 1) {
            if (e & 1) {
                const double r00 = p00 * m00 + p01 * m10, r01 = p00 * m01 + p01 * m11, r10 = p10 * m00 + p11 * m10, r11 = p10 * m01 + p11 * m11;
                m00 = r00; m01 = r01; m10 = r10; m11 = r11;
            }
            const double r00 = p00 * p00 + p01 * p10, r01 = p00 * p01 + p01 * p11, r10 = p10 * p00 + p11 * p10, r11 = p10 * p01 + p11 * p11;
            p00 = r00; p01 = r01; p10 = r10; p11 = r11;
        }
        double2 v = make_double2(y1, y2);
        scan[0][t] = v;
        __syncthreads();
        int cur = 0;
#pragma unroll
        for (int off = 1; off < kChanThreads; off <<= 1) {
            if (t >= off) {
                const double2 u = scan[cur][t - off];
                v.x += m00 * u.x + m01 * u.y;
                v.y += m10 * u.x + m11 * u.y;
            }
            scan[cur ^ 1][t] = v;
            __syncthreads();
            cur ^= 1;
            const double r00 = m00 * m00 + m01 * m10, r01 = m00 * m01 + m01 * m11, r10 = m10 * m00 + m11 * m10, r11 = m10 * m01 + m11 * m11;
            m00 = r00; m01 = r01; m10 = r10; m11 = r11;
        }
        y1 = 0.0; y2 = 0.0;
        if (t > 0) { const double2 u = scan[cur][t - 1]; y1 = u.x; y2 = u.y; }
        x1 = x1_0; x2 = x2_0;
        for (int i = 0; i < L; ++i) {
            const double x = double(mine[i]);
            const double y = fma(-a1, y1, fma(-a2, y2, fma(b0, x, fma(b1, x1, b2 * x2))));
            mine[i] = float(y);
            x2 = x1; x1 = x; y2 = y1; y1 = y;
        }
        __syncthreads();                                // the next section reads its neighbour's last two outputs, and scan[] again
    }
    double gain = 0.0, scale = 0.0;                     // out = gain tanh(scale y); d == 0: out = y
    if (d != 0.f) {
        float p = 0.f;                                  // fmaxf passes a NaN over; samples at or past N are 0 or, behind a NaN, not looked at
        for (int i = 0; i < L; ++i)
            if (t * L + i < N) p = fmaxf(p, fabsf(mine[i]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) p = fmaxf(p, __shfl_xor(p, off));
        if ((t & 63) == 0) wave_peak[t >> 6] = p;
        __syncthreads();
        p = fmaxf(fmaxf(wave_peak[0], wave_peak[1]), fmaxf(wave_peak[2], wave_peak[3]));
        if (p > 0.f) {
            gain = double(p) / tanh(double(d));
            scale = double(d) / double(p);
        }
    }
    for (int k = 0; k < L; ++k) {
        const int i = t + kChanThreads * k;
        if (i >= N) break;
        const int q = int(__umulhi(uint32_t(i), l_recip));
        float y = clip[q * stride + (i - q * L)];
        if (d != 0.f && scale != 0.0) y = float(gain * tanh(scale * double(y)));
        dst[i] = y;
    }
}

int launch_channel_draw(const ww_channel_config& g, uint64_t seed, int64_t n, float* records, hipStream_t stream) {
    const int64_t grid = (n * 16 + kChanThreads - 1) / kChanThreads;
    return launch<channel_draw_kernel>(dim3(unsigned(grid)), dim3(kChanThreads), 0, stream, records, n, seed, g);
}

int launch_channel(const float* in, float* out, int64_t n, int n_samples, int64_t row_stride, const float* records, uint64_t seed,
                   const ww_channel_config& g, hipStream_t stream) {
    const int L = (n_samples + kChanThreads - 1) / kChanThreads;
    if (L < 2 || L > kChanMaxChunk) return fail(WW_EUNSUPPORTED, "n_samples %d: chunks of 2..%d samples", n_samples, kChanMaxChunk);
    const uint32_t l_recip = uint32_t((uint64_t(1) << 32) / uint64_t(L)) + 1u;
    return launch<channel_kernel>(dim3(unsigned(n)), dim3(kChanThreads), 0, stream, in, out, n_samples, L, l_recip, row_stride, records, seed, g);
}

}  // namespace ww
