// SpecAugment on log-mel batches: blocks of mel bands and of frames of a clip replaced by one fill value.
//   spec_draw_kernel      one thread per clip: the clip's record drawn from the counter-based generator, for callers and tests to read
//   spec_augment_kernel   one wave per clip: the record (read from device memory or drawn by the same function), the clip's mean or
//                         minimum where the fill mode wants one, then the masked positions
// mel [n][80][T] float32, T = 1 .. 63: a clip is 320 T bytes, so every clip starts on a 16-byte boundary and is 20 T float4.  A wave keeps
// its clip in registers (at most 20 float4 per lane) between the loads, the reduction and the stores: each byte is read once.
// Memory-bound: out of place 2 x 320 T bytes per clip; in place the clip read (mean, min) plus the masked floats written.
#include "ww_internal.h"

namespace ww {

constexpr int kSpecThreads = 256;                       // four waves, one clip each
constexpr int kSpecWaves = kSpecThreads / 64;
constexpr int kSpecRecord = 16;                         // int16 per clip: [f_start, f_width] x 4, [t_start, t_width] x 4
constexpr int kSpecMasks = 4;                           // per axis

// The three xor-shift-multiply steps of splitmix64 (dropout_factor in ww_head.hip applies the same ones).
__device__ __forceinline__ uint64_t fmix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// Word j of clip c: the clip's index in the batch is the only thing besides the seed that enters, so a clip's record does not depend on n.
__device__ __forceinline__ uint64_t spec_word(uint64_t seed, int64_t c, int j) {
    return fmix64(seed + 0x9E3779B97F4A7C15ull * (32ull * uint64_t(c) + uint64_t(j) + 1ull));
}

// An integer in 0 .. m from the top 32 bits of r.
__device__ __forceinline__ int int_in(uint64_t r, int m) { return int(((r >> 32) * uint64_t(m + 1)) >> 32); }

// Clip c's record as 16 ints: read from `records` when the caller gave some, else drawn.  Both kernels go through here.
__device__ __forceinline__ void spec_record(const int16_t* __restrict__ records, const SpecDraw& d, int64_t c, int T, int (&rec)[kSpecRecord]) {
    if (records) {
        const int4* p = reinterpret_cast<const int4*>(records + c * kSpecRecord);
        const int4 a = p[0], b = p[1];
        const int w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            rec[2 * i] = int(int16_t(w[i] & 0xffff));
            rec[2 * i + 1] = w[i] >> 16;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < kSpecRecord; ++i) rec[i] = 0;
    const float u = float(uint32_t(spec_word(d.seed, c, 0) >> 40)) * (1.0f / 16777216.0f);      // 24 bits
    if (!(u < d.prob)) return;
#pragma unroll
    for (int i = 0; i < kSpecMasks; ++i) {
        if (i < d.n_freq) {
            const int w = int_in(spec_word(d.seed, c, 1 + 2 * i), d.freq_max);
            rec[2 * i] = int_in(spec_word(d.seed, c, 2 + 2 * i), kMels - w);
            rec[2 * i + 1] = w;
        }
        if (i < d.n_time) {
            const int w = int_in(spec_word(d.seed, c, 9 + 2 * i), d.time_max);
            rec[8 + 2 * i] = int_in(spec_word(d.seed, c, 10 + 2 * i), T - w);
            rec[8 + 2 * i + 1] = w;
        }
    }
}

__global__ __launch_bounds__(kSpecThreads) void spec_draw_kernel(int16_t* __restrict__ records, int64_t n, int T, SpecDraw d) {
    const int64_t c = int64_t(blockIdx.x) * kSpecThreads + threadIdx.x;
    if (c >= n) return;
    int rec[kSpecRecord];
    spec_record(nullptr, d, c, T, rec);
    int w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (rec[2 * i] & 0xffff) | (rec[2 * i + 1] << 16);
    int4* p = reinterpret_cast<int4*>(records + c * kSpecRecord);
    p[0] = make_int4(w[0], w[1], w[2], w[3]);
    p[1] = make_int4(w[4], w[5], w[6], w[7]);
}

// Bits 0 .. k-1 (none for k <= 0, all 64 for k >= 64), and the bits of [a, b) inside 0 .. 63: a record that reaches outside the clip
// masks what lies inside it, and one whose width is 0 or negative masks nothing.
__device__ __forceinline__ uint64_t bits_below(int k) { return k <= 0 ? 0ull : k >= 64 ? ~0ull : (1ull << k) - 1ull; }
__device__ __forceinline__ uint64_t bits_of(int a, int b) { return bits_below(b) & ~bits_below(a); }

// One wave per clip.  Lane l owns the float4 l + 64 k, k < kV (kV = 5, 10 or 20 by T; the ones at or past 20 T are skipped).
// The mean: every lane adds its floats in double in the order it holds them, then an xor butterfly over the 64 lanes -- an order that T
// alone fixes -- and one rounding of sum / (80 T) to float32.  The minimum is an fminf fold (a NaN is passed over).
// in == out is allowed (the host refuses every other overlap): a clip without masks is then left alone, unread; a float4 that is
// masked whole is stored as one, single masked floats one by one; WW_SPEC_FILL_VALUE does not read the clip at all.
template <int kV>
__global__ __launch_bounds__(kSpecThreads) void spec_augment_kernel(const float* in, float* out, int64_t n, int T, uint32_t t_recip,
                                                                    const int16_t* __restrict__ records, SpecDraw d, int mode, float fill_value) {
    const int lane = threadIdx.x & 63;
    const int64_t c = int64_t(blockIdx.x) * kSpecWaves + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    if (c >= n) return;
    int rec[kSpecRecord];
    spec_record(records, d, c, T, rec);
    uint64_t rows_lo = 0, rows_hi = 0, cols = 0;                       // mel bands 0 .. 63, 64 .. 79, frames
#pragma unroll
    for (int i = 0; i < kSpecMasks; ++i) {
        const int f0 = rec[2 * i], f1 = f0 + rec[2 * i + 1], t0 = rec[8 + 2 * i], t1 = t0 + rec[8 + 2 * i + 1];
        rows_lo |= bits_of(f0, f1);
        rows_hi |= bits_of(f0 - 64, f1 - 64);
        cols |= bits_of(t0, t1);
    }
    rows_hi &= bits_below(kMels - 64);
    cols &= bits_below(T);
    const bool any = (rows_lo | rows_hi | cols) != 0;
    const bool inplace = in == out;
    if (inplace && !any) return;

    const int nvec = 20 * T;
    const float* src = in + c * int64_t(kMels) * T;
    float* dst = out + c * int64_t(kMels) * T;
    const bool load = !inplace || mode != WW_SPEC_FILL_VALUE;
    float4 v[kV];
#pragma unroll
    for (int k = 0; k < kV; ++k) {
        const int idx = lane + 64 * k;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (load && idx < nvec) v[k] = *reinterpret_cast<const float4*>(src + 4 * idx);
    }
    float fill = fill_value;
    if (any && mode == WW_SPEC_FILL_MEAN) {
        double acc = 0.0;                                              // the skipped float4 hold +0.0f: adding them changes nothing
#pragma unroll
        for (int k = 0; k < kV; ++k) {
            acc += double(v[k].x); acc += double(v[k].y); acc += double(v[k].z); acc += double(v[k].w);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        fill = float(acc / double(kMels * T));
    } else if (any && mode == WW_SPEC_FILL_MIN) {
        float m = __builtin_inff();
#pragma unroll
        for (int k = 0; k < kV; ++k)
            if (lane + 64 * k < nvec) m = fminf(fminf(m, fminf(v[k].x, v[k].y)), fminf(v[k].z, v[k].w));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off));
        fill = m;
    }
#pragma unroll
    for (int k = 0; k < kV; ++k) {
        const int idx = lane + 64 * k;
        if (idx >= nvec) continue;
        float r[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        bool m[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t e = uint32_t(4 * idx + q);                  // e < 80 T <= 5040: e T < 2^32, so the reciprocal multiply is exact
            const uint32_t row = T == 1 ? e : __umulhi(e, t_recip);    // t_recip = floor(2^32 / T) + 1
            const uint32_t col = e - row * uint32_t(T);
            const uint64_t rb = row < 64u ? rows_lo >> row : rows_hi >> (row - 64u);
            m[q] = ((rb | (cols >> col)) & 1ull) != 0;
            if (m[q]) r[q] = fill;
        }
        if (!inplace || (m[0] && m[1] && m[2] && m[3])) {
            *reinterpret_cast<float4*>(dst + 4 * idx) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (m[q]) dst[4 * idx + q] = fill;
        }
    }
}

int launch_spec_draw(const SpecDraw& d, int64_t n, int T, int16_t* records, hipStream_t stream) {
    const int64_t grid = (n + kSpecThreads - 1) / kSpecThreads;
    return launch<spec_draw_kernel>(dim3(unsigned(grid)), dim3(kSpecThreads), 0, stream, records, n, T, d);
}

int launch_spec_augment(const float* in, float* out, int64_t n, int T, const int16_t* records, const SpecDraw& d, int mode, float fill_value,
                        hipStream_t stream) {
    const dim3 grid(unsigned((n + kSpecWaves - 1) / kSpecWaves)), block(kSpecThreads);
    const uint32_t t_recip = T == 1 ? 0u : uint32_t((uint64_t(1) << 32) / uint64_t(T)) + 1u;
    if (T <= 16)
        return launch<spec_augment_kernel<5>>(grid, block, 0, stream, in, out, n, T, t_recip, records, d, mode, fill_value);
    if (T <= 32)
        return launch<spec_augment_kernel<10>>(grid, block, 0, stream, in, out, n, T, t_recip, records, d, mode, fill_value);
    return launch<spec_augment_kernel<20>>(grid, block, 0, stream, in, out, n, T, t_recip, records, d, mode, fill_value);
}

}  // namespace ww
