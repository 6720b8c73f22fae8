// KA: AudioProcessor.augment_audio on the GPU (training-side, feeds K1).
//
// Replaces /root/reference/wakeword_training_script.py:103-123, one plan (the caller's random draws) per clip:
//     np.roll -> librosa.effects.pitch_shift -> librosa.effects.time_stretch + pad_or_truncate -> + N(0, sigma)
// librosa.effects.time_stretch = istft(phase_vocoder(stft(y), rate), length=round(len/rate)), n_fft 2048 / hop 512 / Hann;
// pitch_shift = resample(time_stretch(y, 2^(-n/12)), ratio) cut or zero-padded to the input length.
//
//   roll_kernel       out[i] = in[(i - shift) mod L]                        (also the copy into the work buffer)
//   stft_pv_kernel    one workgroup per clip: four frames per round (one per wave: window, 1024-point complex FFT of the packed
//                     real frame (ww_fft.h), real-input split in place) into a ring of eight LDS slabs, then the phase vocoder
//                     over the output steps whose two columns are there: thread = bin; librosa's arithmetic types are kept
//                     (float32 magnitudes and phase accumulator, float64 phase advance) so that the accumulator rounds the
//                     same way; angle / magnitude / phasor by short in-kernel forms instead of libm's atan2f / hypotf / sincosf.
//   istft_kernel      Hermitian spectrum -> conj(Z) -> the same forward FFT -> frame, four frames per round into a ring
//                     of eight LDS slabs; the hop segments a round completes are summed straight from the slabs in
//                     frame order with the window and its sum-square, centre-trimmed, cropped / zero-padded
//   resample_kernel   windowed-sinc interpolation at t = i / ratio (resampy 'kaiser_best' table in LDS, float32 MACs): the stand-in
//                     for librosa's soxr_hq (absent third-party library; parity unpinned)
//   noise_kernel      + sigma * normal(seed, i), the build's counter-based generator (splitmix64 -> Box-Muller)
//   reverb_kernel     (ww_reverb.hip) the clip convolved with a room impulse response, energy kept: one workgroup per clip; runs
//                     between the stretch and the mix in a batch where some clip has reverb on
//   mix_kernel        background noise at an SNR, then the same Gaussian noise: one workgroup per clip (whole-clip energies first);
//                     replaces noise_kernel in a batch where some clip has background on
// Clips whose plan switches a transform off skip its kernels (their blocks copy the data through).
//
// Clip length: every kernel is a template on kN, the samples per clip -- 16000 (the 1 s entry points, a compile-time constant as before)
// or 0 (run-time `n`, 4000 <= n <= 16383: the *_n entry points), T = 1 + n / 512 <= 32 STFT frames.  At run-time n the work-buffer
// rows (bufA / bufB) are padded to a multiple of four floats for the float4 accesses; the padding is never used as a sample (stft_pv
// loads it and zeroes it).
// Each kernel forms L (samples per clip) and row (floats per work-buffer row) as `kN ? kN : ...` in place, so the 1 s instance folds them
// to the constants it always had and compiles to the same code as before.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "ww_fft.h"

namespace ww {

constexpr int kAugFrames = kFrames;                 // STFT frames of a 16000-sample clip (1 + 16000/512 = 32), the most any length has
constexpr int kAugMaxOut = 46;                      // phase-vocoder output steps: ceil(32 / rate), rate >= 32/46 (for every clip length)
constexpr int kAugYStride = 25600;                  // stretched-clip scratch row
constexpr int kSpec = kBins;                        // 1025 complex bins per spectrum row

struct AugDev {            // one per clip, derived on the host from ww_augment_plan
    int32_t shift;         // np.roll shift reduced to [0, L)
    int32_t crop;          // crop start after time_stretch
    int32_t p_out, p_len, p_res;   // pitch: PV steps, istft length, resampled length (0 = pitch off)
    int32_t s_out, s_len;          // stretch: PV steps, istft length (0 = stretch off)
    uint32_t seed;
    double p_rate, p_ratio, s_rate;
    float sigma;
    float pad_;
};

// ------------------------------------------------------------------------------------------------
template <int kN>
__global__ __launch_bounds__(256) void roll_kernel(const float* __restrict__ in, int64_t stride, const AugDev* __restrict__ plan,
                                                   float* __restrict__ out, int n) {
    const int L = kN ? kN : n, row = kN ? kN : (n + 3) & ~3;
    const int clip = blockIdx.y;
    const int i = 4 * (blockIdx.x * 256 + threadIdx.x);          // four outputs per thread: one 16-byte store (row % 4 == 0)
    if (i >= L) return;
    const float* __restrict__ x = in + int64_t(clip) * stride;
    float4 v;
    if constexpr (kN != 0) {
        int src = i - plan[clip].shift;
        src += src < 0 ? kN : 0;
        if (src + 3 < kN) { v.x = x[src]; v.y = x[src + 1]; v.z = x[src + 2]; v.w = x[src + 3]; }
        else {                                                   // the wrap falls inside this group of four
            v.x = x[src]; v.y = x[src + 1 < kN ? src + 1 : src + 1 - kN];
            v.z = x[src + 2 < kN ? src + 2 : src + 2 - kN]; v.w = x[src + 3 - kN];
        }
    } else {
        // the shift is reduced again against this n (records prepared for another length stay inside the row); the row's last group
        // of four may pass its end: those outputs are the padding (zero), nothing past the row is read
        int src = i - plan[clip].shift % L;
        src += src < 0 ? L : 0;
        float* pv = &v.x;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int s = src + q;
            s -= s >= L ? L : 0;
            pv[q] = i + q < L ? x[s] : 0.f;
        }
    }
    *reinterpret_cast<float4*>(out + int64_t(clip) * row + i) = v;
}

// atan2 for the vocoder: a = min/max in [0, 1], atan(a) = a P(a^2) (degree 8 in a^2, |err| <= 1.2e-7 in float32 evaluation -- the size of
// libm's own last-place error at these magnitudes), octant and quadrant folded back; signed zeros and (0, 0) as atan2f has them.
__device__ __forceinline__ float pv_atan2(float y, float x) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    // min / max by v_rcp_f32 (1 ulp; the polynomial's own error is of that size).  The hardware reciprocal takes denormals for zero, so
    // tiny pairs are scaled up first (exact, the ratio is unchanged)
    const float sc = mx < 5.4210109e-20f ? 1.8446744e19f : 1.0f;                      // 2^-64, 2^64
    mx *= sc; mn *= sc;
    const float a = mx > 0.f ? mn * __builtin_amdgcn_rcpf(mx) : 0.f;
    const float q = a * a;
    float p = 2.399661113e-03f;
    p = fmaf(p, q, -1.415910292e-02f);
    p = fmaf(p, q, 3.935785964e-02f);
    p = fmaf(p, q, -7.195615768e-02f);
    p = fmaf(p, q, 1.047824398e-01f);
    p = fmaf(p, q, -1.415504068e-01f);
    p = fmaf(p, q, 1.998492777e-01f);
    p = fmaf(p, q, -3.333252668e-01f);
    p = fmaf(p, q, 9.999998808e-01f);
    float r = a * p;
    r = ay > ax ? 1.57079632679489662f - r : r;
    r = __builtin_signbitf(x) ? 3.14159265358979324f - r : r;
    return __builtin_copysignf(r, y);
}

// cos / sin of the float32 phase accumulator.  The accumulator reaches 10^4 .. 10^5 radians (phi = pi k / 2 per step): libm's sincosf takes
// its large-argument reduction path there (round 2: the bulk of this kernel's time).  Here the turn count acc / 2 pi is formed in double, its
// fraction goes to the hardware's v_sin_f32 / v_cos_f32 (arguments in revolutions; absolute error ~1e-6, five hundred times under the tests' bound
// on the output samples).
// |c| by v_sqrt_f32 (1 ulp) instead of the correctly rounded expansion
__device__ __forceinline__ float pv_abs(float2 c) {
    return __builtin_amdgcn_sqrtf(fmaf(c.x, c.x, c.y * c.y));
}

// round(dphase / 2 pi) with the quotient formed by the reciprocal: differs from the division only when the quotient is within an ulp of a
// half-integer, where either neighbour wraps the phase to the same angle (the accumulator then differs by its own rounding of +-2 pi)
__device__ __forceinline__ double pv_wrap(double dphase) {
    const double two_pi = 6.283185307179586476925286766559;
    return dphase - two_pi * __builtin_rint(dphase * 0.15915494309189533576888);
}

__device__ __forceinline__ void pv_sincos(float acc, float& sn, float& cs) {
    const double turns = double(acc) * 0.15915494309189533576888;       // 1 / (2 pi)
    const float fr = float(turns - __builtin_rint(turns));                // [-0.5, 0.5]
    sn = __builtin_amdgcn_sinf(fr);
    cs = __builtin_amdgcn_cosf(fr);
}

// ------------------------------------------------------------------------------------------------
// The STFT and the phase vocoder in one pass over the clip: the STFT columns never leave the CU.  Four frames per round (one per wave) are
// transformed into a ring of eight LDS slabs and split IN PLACE into their spectrum column (a lane reads Z[k], Z[1024-k] and writes
// D[k], D[1024-k] back to the same two slots; D[1024] takes the slab's spare slot), then every thread advances its bins' vocoder state
// over the output steps whose two columns are there.  A step reads columns i0, i0 + 1 with i0 non-decreasing, so round r + 1 may
// overwrite the columns of round r - 1 (two barriers per round).  ceil(T / 4) rounds: a last round that is only partly inside the clip
// transforms frames >= T too, but no step reads them -- the vocoder sees zero columns past T - 1, as librosa's padded D.
constexpr int kStftPvLds = 8 * fft::kSlabFloats * int(sizeof(float));                    // 65,664 B: two workgroups per CU

template <int kN>
__global__ __launch_bounds__(256) void stft_pv_kernel(const float* __restrict__ x, const AugDev* __restrict__ plan, int which,
                                                      const LogmelTables* __restrict__ tb, float2* __restrict__ S, int n) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int clip = blockIdx.x, tid = threadIdx.x;
    const int n_out = which == 0 ? plan[clip].p_out : plan[clip].s_out;
    if (n_out == 0) return;
    const double rate = which == 0 ? plan[clip].p_rate : plan[clip].s_rate;
    const int lane = tid & 63, wave = tid >> 6;
    const int L = kN ? kN : n, row = kN ? kN : (n + 3) & ~3, T = 1 + L / kHop;      // T = kAugFrames at 1 s
    const float* xc = x + int64_t(clip) * row;
    const float4* win4 = reinterpret_cast<const float4*>(&tb->window[0]);
    float2* Sc = S + int64_t(clip) * kAugMaxOut * kSpec;
    constexpr int kB = 5;                                        // bins tid + 256 b; b = 4 is bin 1024 (thread 0 only)
    float acc[kB], m0[kB], a0[kB], m1[kB], a1[kB];
#pragma unroll
    for (int b = 0; b < kB; ++b) { acc[b] = 0.f; m0[b] = 0.f; a0[b] = 0.f; m1[b] = 0.f; a1[b] = 0.f; }
    int have = -2, t = 0;
    for (int r = 0; r < (T + 3) / 4; ++r) {
        {
            const int frame = 4 * r + wave;
            float* slab = lds + (frame & 7) * fft::kSlabFloats;
            float2* slab2 = reinterpret_cast<float2*>(slab);
            float2 za[8], zb[8];
            const int base = frame * kHop - kNfft / 2 + 4 * lane;
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) {
                const int idx = base + 256 * n1;                 // a multiple of 4
                float4 s;
                if constexpr (kN != 0) {
                    s = (idx >= 0 && idx < kN) ? *reinterpret_cast<const float4*>(xc + idx) : make_float4(0.f, 0.f, 0.f, 0.f);
                } else {
                    // the rows are padded to a multiple of 4, so a group that starts inside the row is one 16-byte load within it; its
                    // lanes past L (the padding) are replaced by zeros -- selected, never used as samples (a branchy partial load here
                    // took 1.43 instead of 1.11 ms per 4096 clips at T = 32)
                    s = (idx >= 0 && idx < L) ? *reinterpret_cast<const float4*>(xc + idx) : make_float4(0.f, 0.f, 0.f, 0.f);
                    s.y = idx + 1 < L ? s.y : 0.f;
                    s.z = idx + 2 < L ? s.z : 0.f;
                    s.w = idx + 3 < L ? s.w : 0.f;
                }
                const float4 w = win4[64 * n1 + lane];
                za[n1] = make_float2(s.x * w.x, s.y * w.y);
                zb[n1] = make_float2(s.z * w.z, s.w * w.w);
            }
            fft::wave_fft1024(za, zb, slab, tb, lane);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = lane + 64 * j;                     // 0..511
                const int pa = fft::zpos(k), pb = fft::zpos((1024 - k) & 1023);
                const float2 a = slab2[pa], b = slab2[pb];
                const float2 tw = tb->twr[k];
                const float2 e = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
                const float2 o = make_float2(0.5f * (a.y + b.y), 0.5f * (b.x - a.x));
                const float2 tt = fft::cmul(o, tw);
                slab2[pa] = make_float2(e.x + tt.x, e.y + tt.y);
                slab2[k == 0 ? 1024 : pb] = make_float2(e.x - tt.x, -(e.y - tt.y));
            }
            if (lane == 0) { const int pz = fft::zpos(512); const float2 z = slab2[pz]; slab2[pz] = make_float2(z.x, -z.y); }
        }
        __syncthreads();                                         // columns <= 4r + 3 are in their slabs
        {
#pragma clang fp contract(off)
            const double two_pi = 6.283185307179586476925286766559;
            if (r == 0) {
                const float2* c = reinterpret_cast<const float2*>(lds);
#pragma unroll
                for (int b = 0; b < kB; ++b) {
                    const int k = tid + 256 * b;
                    if (k < kSpec) { const float2 d0 = c[fft::zpos(k)]; acc[b] = pv_atan2(d0.y, d0.x); }
                }
            }
            const int last = 4 * r + 3;
            for (; t < n_out; ++t) {
                const double step = double(t) * rate;
                const int i0 = int(step);
                if ((i0 + 1 < T ? i0 + 1 : T - 1) > last) break;                  // this step's columns come with a later round
                const double alpha = step - double(i0);
                const bool fresh0 = i0 != have && i0 != have + 1, fresh1 = i0 != have;
                const float2* c0 = reinterpret_cast<const float2*>(lds + (i0 & 7) * fft::kSlabFloats);
                const float2* c1 = reinterpret_cast<const float2*>(lds + ((i0 + 1) & 7) * fft::kSlabFloats);
#pragma unroll
                for (int b = 0; b < kB; ++b) {
                    const int k = tid + 256 * b;
                    if (k < kSpec) {
                        const double phi = double(k) * two_pi * 0.25;
                        if (fresh1) {
                            if (!fresh0) { m0[b] = m1[b]; a0[b] = a1[b]; }
                            else {
                                const float2 v = i0 < T ? c0[fft::zpos(k)] : make_float2(0.f, 0.f);
                                m0[b] = pv_abs(v);
                                a0[b] = pv_atan2(v.y, v.x);
                            }
                            const float2 v = i0 + 1 < T ? c1[fft::zpos(k)] : make_float2(0.f, 0.f);
                            m1[b] = pv_abs(v);
                            a1[b] = pv_atan2(v.y, v.x);
                        }
                        const float mag = float(1.0 - alpha) * m0[b] + float(alpha) * m1[b];
                        float sn, cs;
                        pv_sincos(acc[b], sn, cs);
                        Sc[int64_t(t) * kSpec + k] = make_float2(cs * mag, sn * mag);
                        const float da = a1[b] - a0[b];
                        double dphase = double(da) - phi;
                        dphase = pv_wrap(dphase);
                        acc[b] = float(double(acc[b]) + (phi + dphase));
                    }
                }
                have = i0;
            }
        }
        __syncthreads();                                         // the next round overwrites the columns of round r - 1
    }
}

// ------------------------------------------------------------------------------------------------
constexpr int kIstftSlabs = 8;                                   // two rounds of four frames stay resident
constexpr int kIstftLds = kIstftSlabs * fft::kSlabFloats * int(sizeof(float));          // 65,664 B: two workgroups per CU

// dst[i], i < dst_len, = y[i + crop] (0 past the stretched length); clips with the stage off copy `passthru` instead.
// Four frames per round (one per wave) into a ring of eight slabs.  A sample of the padded signal in hop segment s is
// covered by frames s-3..s, so after round r the segments 4r..4r+3 are complete: they are summed straight from the
// slabs in frame order (librosa's order), normalised and stored -- no overlap-add buffer, two barriers per round.
template <int kN>
__global__ __launch_bounds__(256) void istft_kernel(const float2* __restrict__ S, const AugDev* __restrict__ plan, int which,
                                                    const LogmelTables* __restrict__ tb, const float* __restrict__ passthru,
                                                    float* __restrict__ dst, int64_t dst_stride, int n_rt) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int clip = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int n_out = which == 0 ? plan[clip].p_out : plan[clip].s_out;
    const int L = kN ? kN : n_rt, row = kN ? kN : (n_rt + 3) & ~3;
    float* out = dst + int64_t(clip) * dst_stride;
    if (n_out == 0) {
        if (passthru)
            for (int i = tid; i < L; i += 256) out[i] = passthru[int64_t(clip) * row + i];
        return;
    }
    const int length = which == 0 ? plan[clip].p_len : plan[clip].s_len;
    const int crop = which == 0 ? 0 : plan[clip].crop;
    const int dst_len = which == 0 ? length : L;
    int n_frames = (length + kNfft + kHop - 1) / kHop;           // ceil((length + n_fft) / hop)
    n_frames = n_frames < n_out ? n_frames : n_out;
    const float2* Sc = S + int64_t(clip) * kAugMaxOut * kSpec;
    const int rounds = (n_frames + 3) / 4 + 1;                   // + a flush round for the tails of the last frames
    for (int r = 0; r < rounds; ++r) {
        const int frame = 4 * r + wave;
        if (frame < n_frames) {
            float* slab = lds + (frame % kIstftSlabs) * fft::kSlabFloats;
            const float2* X = Sc + int64_t(frame) * kSpec;
            float2 za[8], zb[8];
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int m = 128 * n1 + 2 * lane + q;       // 0..1023
                    float2 xm = X[m], xp = X[1024 - m];
                    if (m == 0) { xm.y = 0.f; xp.y = 0.f; }      // irfft ignores the imaginary parts of DC and Nyquist
                    // E = (X[m] + conj X[M-m])/2, O = (X[m] - conj X[M-m])/2 * conj(W^m), Z = E + iO; FFT input conj(Z)
                    const float2 e = make_float2(0.5f * (xm.x + xp.x), 0.5f * (xm.y - xp.y));
                    const float2 d = make_float2(0.5f * (xm.x - xp.x), 0.5f * (xm.y + xp.y));
                    const float2 w = tb->twr[m];
                    const float2 o = fft::cmul(d, make_float2(w.x, -w.y));
                    const float2 zc = make_float2(e.x - o.y, -(e.y + o.x));
                    if (q == 0) za[n1] = zc; else zb[n1] = zc;
                }
            fft::wave_fft1024(za, zb, slab, tb, lane);          // F = FFT(conj Z); z[n] = conj(F[n]) / 1024
        }
        __syncthreads();                                         // frames <= 4r + 3 are in their slabs
        // segments 4r .. 4r+3 of the padded signal: 1024 sample PAIRS (2p, 2p+1), four per thread
        for (int pp = tid; pp < 4 * kHop / 2; pp += 256) {
            const int n = 4 * r * kHop + 2 * pp;                 // even sample of the pair
            const int seg = n / kHop;
            int f0 = seg - 3;
            f0 = f0 < 0 ? 0 : f0;
            const int f1 = seg < n_frames - 1 ? seg : n_frames - 1;
            float vx = 0.f, vy = 0.f, wsx = 0.f, wsy = 0.f;      // window sum-square in float32, frame order, as librosa
            for (int f = f0; f <= f1; ++f) {
                const int j = n - f * kHop;                      // even, 0..2046
                const float2 F = reinterpret_cast<const float2*>(lds + (f % kIstftSlabs) * fft::kSlabFloats)[fft::zpos(j >> 1)];
                const float2 w = *reinterpret_cast<const float2*>(&tb->window[j]);
                vx += w.x * (F.x * (1.0f / 1024.0f));
                vy += w.y * (-F.y * (1.0f / 1024.0f));
                wsx += w.x * w.x;
                wsy += w.y * w.y;
            }
            if (wsx > 1.17549435e-38f) vx = vx / wsx;
            if (wsy > 1.17549435e-38f) vy = vy / wsy;
            const int src = n - kNfft / 2;                       // centre trim; n even, so src and src + 1 share their fate below
            const int i = src - crop;
            if (i >= 0 && i < dst_len) out[i] = src < length ? vx : 0.f;
            if (i + 1 >= 0 && i + 1 < dst_len) out[i + 1] = src + 1 < length ? vy : 0.f;
        }
        __syncthreads();                                         // the next round overwrites the slabs of round r - 1
    }
    // samples past the reach of the last frame (only when the spectrogram is shorter than `length` asks for)
    for (int i = 4 * rounds * kHop - kNfft / 2 - crop + tid; i < dst_len; i += 256)
        if (i >= 0) out[i] = 0.f;
}

// ------------------------------------------------------------------------------------------------
constexpr int kKbZeros = 64, kKbTable = 512;
constexpr int kKbLen = kKbZeros * kKbTable + 1;                  // 32,769 table entries
// transposed table of resample_kernel: (step + 2) rows of R floats; step <= 512 -> R = 68; the pitch range's smallest step (scale 32/46) is 356 -> R = 96
constexpr int kResampleLds = 150 * 1024;

// One workgroup of 1024 threads per clip.  Pitch-off clips copy through.
// The taps of one output are the table entries offset + i * step, i = 0, 1, ... -- `step` = int(scale * 512) is the same for every
// output of a clip, `offset` is a pseudo-random phase.  Round 2 kept the half-window in LDS in its natural order: one ds_read2_b32 per
// tap at a random address per lane (3.5-way bank conflicts on average, 3.3 ms per 4096 clips, half of the augmentation).  Round 3 loads
// it TRANSPOSED by phase, P[ph][i] = tab[ph + i * step] (rows of R floats, step + 2 rows: 137-145 KB): a lane's taps are consecutive in
// its row, so four taps are one ds_read_b128 (two rows: the entry and its upper neighbour for the interpolation), and the four samples
// one 16-byte global load.  Same weights, same fused multiply-adds in the same order: the results are bit-identical to the round-2 kernel.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));       // four consecutive samples at a 4-byte aligned address

template <int kN>
__global__ __launch_bounds__(1024) void resample_kernel(const float* __restrict__ Y, const AugDev* __restrict__ plan,
                                                        const LogmelTables* __restrict__ tb, const float* __restrict__ passthru,
                                                        float* __restrict__ out, int n_rt) {
    extern __shared__ __attribute__((aligned(16))) float P[];   // [step + 2][R]
    const int clip = blockIdx.x, tid = threadIdx.x;
    const int L = kN ? kN : n_rt, row = kN ? kN : (n_rt + 3) & ~3;
    float* o = out + int64_t(clip) * row;
    if (plan[clip].p_out == 0) {
        for (int i = tid; i < L; i += 1024) o[i] = passthru[int64_t(clip) * row + i];
        return;
    }
    const double ratio = plan[clip].p_ratio;
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const int index_step = int(scale * kKbTable);
    const int cnt = kKbLen / index_step + 1;                      // entries of row 0: i * step <= kKbLen
    int R = (cnt + 3) & ~3;
    if (((R >> 2) & 1) == 0) R += 4;                              // an odd number of 16-byte slots per row spreads the rows over the banks
    // index kKbLen is the pad np.diff(win) gets (the last value again): tab[kKbLen] = tab[kKbLen - 1]
    {   // every thread takes (step + 2) * R / 1024 entries, phase-fastest (coalesced table reads), four loads in flight
        const int rows = index_step + 2, total = rows * R;
#pragma unroll 4
        for (int e = tid; e < total; e += 1024) {
            const int i = e / rows, ph = e - i * rows;
            const int j = ph + i * index_step;
            P[ph * R + i] = (i < cnt && j <= kKbLen) ? tb->kaiser_best[j < kKbLen ? j : kKbLen - 1] : 0.f;
        }
    }
    __syncthreads();
    const int n_orig = plan[clip].p_len, n_res = plan[clip].p_res;
    const float* y = Y + int64_t(clip) * kAugYStride;
    const double inv = 1.0 / ratio;
    for (int t = tid; t < L; t += 1024) {
        // positions and table fractions in float64 (t / ratio needs ~15 integer + 9 fraction bits); the ~140 products per
        // output are float32 FMAs in two independent chains (left wing, right wing), each in tap order.  The two wings advance in
        // lock-step while both have taps left (round 3: twice the loads in flight per wave -- the kernel waits on its table and sample
        // reads, four waves per SIMD being all the LDS-resident table leaves room for)
        float accl = 0.f, accr = 0.f;
        const double time_register = double(t) * inv;
        const int n = int(time_register);
        if (t < n_res && n < n_orig) {
            const double frac_l = scale * (time_register - double(n));
            const double if_l = frac_l * kKbTable;
            const int off_l = int(if_l);
            const float eta_l = float(if_l - double(off_l));
            int i_max = (kKbLen - off_l) / index_step;
            i_max = i_max < n + 1 ? i_max : n + 1;
            const double frac_r = scale - frac_l;
            const double if_r = frac_r * kKbTable;
            const int off_r = int(if_r);
            const float eta_r = float(if_r - double(off_r));
            int k_max = (kKbLen - off_r) / index_step;
            k_max = k_max < n_orig - n - 1 ? k_max : n_orig - n - 1;
            const float* l0 = P + off_l * R;
            const float* r0 = P + off_r * R;
            const float* l1 = l0 + R;
            const float* r1 = r0 + R;
            auto left4 = [&](int i) {
                const float4 t0 = *reinterpret_cast<const float4*>(l0 + i), t1 = *reinterpret_cast<const float4*>(l1 + i);
                const f4u yy = *reinterpret_cast<const f4u*>(y + n - i - 3);              // y[n-i-3 .. n-i]
                accl = fmaf(fmaf(eta_l, t1.x - t0.x, t0.x), yy.w, accl);
                accl = fmaf(fmaf(eta_l, t1.y - t0.y, t0.y), yy.z, accl);
                accl = fmaf(fmaf(eta_l, t1.z - t0.z, t0.z), yy.y, accl);
                accl = fmaf(fmaf(eta_l, t1.w - t0.w, t0.w), yy.x, accl);
            };
            auto right4 = [&](int k) {
                const float4 t0 = *reinterpret_cast<const float4*>(r0 + k), t1 = *reinterpret_cast<const float4*>(r1 + k);
                const f4u yy = *reinterpret_cast<const f4u*>(y + n + 1 + k);              // y[n+1+k .. n+4+k]
                accr = fmaf(fmaf(eta_r, t1.x - t0.x, t0.x), yy.x, accr);
                accr = fmaf(fmaf(eta_r, t1.y - t0.y, t0.y), yy.y, accr);
                accr = fmaf(fmaf(eta_r, t1.z - t0.z, t0.z), yy.z, accr);
                accr = fmaf(fmaf(eta_r, t1.w - t0.w, t0.w), yy.w, accr);
            };
            const int both = (i_max < k_max ? i_max : k_max) & ~3;
            int i = 0;
            for (; i < both; i += 4) { left4(i); right4(i); }
            int k = i;
            for (; i + 4 <= i_max; i += 4) left4(i);
            for (; k + 4 <= k_max; k += 4) right4(k);
            // the last one to three taps of a wing: one more block of four with the weights past the end set to zero (fma(0, y, acc) = acc:
            // the same sum) when its four samples are inside the signal, tap by tap at the signal's edges -- a tap-by-tap tail is a
            // dependent load round trip per tap
            if (i < i_max && n - i - 3 >= 0) {
                const float4 t0 = *reinterpret_cast<const float4*>(l0 + i), t1 = *reinterpret_cast<const float4*>(l1 + i);
                const f4u yy = *reinterpret_cast<const f4u*>(y + n - i - 3);
                accl = fmaf(fmaf(eta_l, t1.x - t0.x, t0.x), yy.w, accl);
                accl = fmaf(i + 1 < i_max ? fmaf(eta_l, t1.y - t0.y, t0.y) : 0.f, yy.z, accl);
                accl = fmaf(i + 2 < i_max ? fmaf(eta_l, t1.z - t0.z, t0.z) : 0.f, yy.y, accl);
                i = i_max;
            }
            if (k < k_max && n + 4 + k < n_orig) {
                const float4 t0 = *reinterpret_cast<const float4*>(r0 + k), t1 = *reinterpret_cast<const float4*>(r1 + k);
                const f4u yy = *reinterpret_cast<const f4u*>(y + n + 1 + k);
                accr = fmaf(fmaf(eta_r, t1.x - t0.x, t0.x), yy.x, accr);
                accr = fmaf(k + 1 < k_max ? fmaf(eta_r, t1.y - t0.y, t0.y) : 0.f, yy.y, accr);
                accr = fmaf(k + 2 < k_max ? fmaf(eta_r, t1.z - t0.z, t0.z) : 0.f, yy.z, accr);
                k = k_max;
            }
            for (; i < i_max; ++i) {
                const float w0 = l0[i], w1 = l1[i];
                accl = fmaf(fmaf(eta_l, w1 - w0, w0), y[n - i], accl);
            }
            for (; k < k_max; ++k) {
                const float w0 = r0[k], w1 = r1[k];
                accr = fmaf(fmaf(eta_r, w1 - w0, w0), y[n + k + 1], accr);
            }
        }
        float acc = accl + accr;
        if (ratio < 1.0) acc *= float(ratio);
        o[t] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The Gaussian noise generator, shared by noise_kernel and mix_kernel: the per-clip keys of the hash generator, and the normal deviate of
// sample i (j = i + 1 in the counter).  The uniforms are the hash generator's exact 32-bit words; Box-Muller runs in float32
// (round 2: float64 log / sqrt / cos, 0.35 ms per 4096 clips for a 0.5 GB stream; the float32 form is bound by that stream).  Against the
// float64 evaluation the normal deviate moves by <= 3e-7 of sigma, four orders under the augmentation tests' tolerance.
__device__ __forceinline__ void noise_keys(uint64_t seed, uint64_t& k1, uint64_t& k2) {
    k1 = mix64(seed * 0x9E3779B97F4A7C15ull + 1ull * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull);
    k2 = mix64(seed * 0x9E3779B97F4A7C15ull + 2ull * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull);
}

__device__ __forceinline__ float noise_normal(uint64_t k1, uint64_t k2, int i) {
    const uint64_t j = uint64_t(i) + 1ull;
    const uint32_t w1 = uint32_t(mix64(k1 + j * 0x9E3779B97F4A7C15ull) >> 32), w2 = uint32_t(mix64(k2 + j * 0x9E3779B97F4A7C15ull) >> 32);
    const float u1 = (float(w1 >> 8) + (float(w1 & 0xffu) + 0.5f) * (1.0f / 256.0f)) * (1.0f / 16777216.0f);   // (w1 + 0.5) / 2^32 to float32
    const float u2 = (float(w2 >> 8) + float(w2 & 0xffu) * (1.0f / 256.0f)) * (1.0f / 16777216.0f) + (0.5f / 4294967296.0f);
    return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// Four samples per thread (float4 in, float4 out).
template <int kN>
__global__ __launch_bounds__(256) void noise_kernel(const float* __restrict__ in, const AugDev* __restrict__ plan,
                                                    float* __restrict__ out, int64_t out_stride, int n) {
    const int L = kN ? kN : n, row = kN ? kN : (n + 3) & ~3;
    const int clip = blockIdx.y;
    const int i = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (i >= L) return;
    float4 v = *reinterpret_cast<const float4*>(in + int64_t(clip) * row + i);          // (padding lanes are not stored)
    const float sigma = plan[clip].sigma;
    if (sigma != 0.f) {
        uint64_t k1, k2;
        noise_keys(plan[clip].seed, k1, k2);
        float* pv = &v.x;
#pragma unroll
        for (int q = 0; q < 4; ++q) pv[q] = fmaf(sigma, noise_normal(k1, k2, i + q), pv[q]);
    }
    float* o = out + int64_t(clip) * out_stride + i;
    if constexpr (kN != 0) {
        if ((out_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) *reinterpret_cast<float4*>(o) = v;
        else { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
    } else {
        if (i + 3 < L && (out_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) *reinterpret_cast<float4*>(o) = v;
        else {
            o[0] = v.x;
            if (i + 1 < L) o[1] = v.y;
            if (i + 2 < L) o[2] = v.z;
            if (i + 3 < L) o[3] = v.w;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Background noise at a random SNR (MS-SNSD's snr_mixer with the SNR as named): one workgroup of 1024 threads per clip, one pass.
//   seg[j] = bank[off + (start + j) mod len], j < L            (a file shorter than the clip repeats)
//   Ex = sum x^2, En = sum seg^2                                (float64: per thread in index order, wave-64 butterfly, then the 16 wave
//                                                                sums in wave order -- a fixed order that depends on L alone)
//   g = sqrt(Ex / (En * 10^(snr/10))), out = fma(g, seg, x)    (nothing is added when Ex or En is 0)
// then (kNoise) + sigma * normal(seed, i) through noise_kernel's generator; the standalone mix has no Gaussian noise.  Sample i of the clip is
// i = tid + 1024 k, k < kPer: the clip and its segment stay in registers between the reduction and the store.
struct BgDev {             // one per clip, derived on the host from ww_augment_bg
    int64_t off;           // the file's first sample in the bank
    int64_t len;           // the file's samples; 0 = no background for this clip
    int64_t start;         // segment start, [0, len)
    double snr_lin;        // 10^(snr_db / 10)
};
constexpr int kMixThreads = 1024;

template <int kN, int kPer, bool kNoise>
__global__ __launch_bounds__(kMixThreads) void mix_kernel(const float* __restrict__ in, int64_t in_stride, const AugDev* __restrict__ plan,
                                                          const BgDev* __restrict__ bg, const float* __restrict__ bank, int64_t bank_len,
                                                          float* __restrict__ out, int64_t out_stride, int n) {
    __shared__ double red[2][kMixThreads / 64];
    __shared__ float gain;
    const int L = kN ? kN : n;
    const int clip = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ x = in + int64_t(clip) * in_stride;
    float xv[kPer], sv[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = tid + kMixThreads * k;
        xv[k] = i < L ? x[i] : 0.f;
        sv[k] = 0.f;
    }
    const BgDev b = bg[clip];
    // a record that does not lie inside the bank (prepared against another one) mixes nothing
    const bool on = b.len > 0 && b.off >= 0 && b.off <= bank_len - b.len && b.start >= 0 && b.start < b.len;
    if (on) {
        const float* __restrict__ f = bank + b.off;
        int64_t p = (b.start + tid) % b.len;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (tid + kMixThreads * k < L) sv[k] = f[p];
            p += kMixThreads;
            if (p >= b.len) p = b.len >= kMixThreads ? p - b.len : p % b.len;
        }
        double ex = 0.0, en = 0.0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            ex = fma(double(xv[k]), double(xv[k]), ex);
            en = fma(double(sv[k]), double(sv[k]), en);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            ex += __shfl_xor(ex, m, 64);
            en += __shfl_xor(en, m, 64);
        }
        if ((tid & 63) == 0) { red[0][tid >> 6] = ex; red[1][tid >> 6] = en; }
        __syncthreads();
        if (tid == 0) {
            double sx = 0.0, sn = 0.0;
            for (int w = 0; w < kMixThreads / 64; ++w) { sx += red[0][w]; sn += red[1][w]; }
            gain = (sx > 0.0 && sn > 0.0) ? float(sqrt(sx / (sn * b.snr_lin))) : 0.f;
        }
        __syncthreads();
    }
    const float g = on ? gain : 0.f;
    const float sigma = kNoise ? plan[clip].sigma : 0.f;
    uint64_t k1 = 0, k2 = 0;
    if (kNoise && sigma != 0.f) noise_keys(plan[clip].seed, k1, k2);
    float* __restrict__ o = out + int64_t(clip) * out_stride;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = tid + kMixThreads * k;
        if (i < L) {
            float v = g != 0.f ? fmaf(g, sv[k], xv[k]) : xv[k];
            if (kNoise && sigma != 0.f) v = fmaf(sigma, noise_normal(k1, k2, i), v);
            o[i] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
static int64_t aug_row_host(int64_t n_samples) { return (n_samples + 3) & ~int64_t(3); }

// The workspace's regions, in bytes -- the one definition: the size below, launch_records and the diagnostic ww_augment_workspace_layout
// all read it.  The spectrogram and stretched-clip scratch keep their 1 s strides at every length: both are sized by the rate bounds,
// which do not change with the length (round(16383 / (32 / 46)) = 23551 <= kAugYStride)
ww_augment_layout augment_workspace_layout(int64_t n, int64_t n_samples) {
    ww_augment_layout l = {};
    l.row_bytes = aug_row_host(n_samples) * 4;
    l.spec_step_bytes = int64_t(kSpec) * 8;
    l.spec_clip_bytes = int64_t(kAugMaxOut) * l.spec_step_bytes;
    l.y_clip_bytes = int64_t(kAugYStride) * 4;
    l.record_bytes = int64_t(sizeof(AugDev));
    l.records = 0;                                                  // (the slot the direct calls copy their AugDev records into)
    l.buf_a = l.records + up256(n * l.record_bytes);
    l.buf_b = l.buf_a + up256(n * l.row_bytes);
    l.spec = l.buf_b + up256(n * l.row_bytes);
    l.y = l.spec + up256(n * l.spec_clip_bytes);
    l.total_bytes = l.y + up256(n * l.y_clip_bytes);
    return l;
}

// Where the BgDev and RirDev arrays of `parts` lie behind `first` bytes: packed behind the [n] AugDev of a records buffer, or in
// 256-byte-rounded slots behind the plain workspace.  The one definition of both orders: the sizes, the prepare and the launchers read it.
struct PartOffsets { int64_t bg, rir, end; };
static PartOffsets part_offsets(int64_t first, int64_t n, unsigned parts, bool slots) {
    const int64_t b = n * int64_t(sizeof(BgDev)), r = n * int64_t(sizeof(RirDev));
    PartOffsets o;
    o.bg = first;
    o.rir = o.bg + (parts & kAugBg ? (slots ? up256(b) : b) : 0);
    o.end = o.rir + (parts & kAugRir ? (slots ? up256(r) : r) : 0);
    return o;
}
static PartOffsets record_offsets(int64_t n, unsigned parts) { return part_offsets(n * int64_t(sizeof(AugDev)), n, parts, false); }
static PartOffsets slot_offsets(int64_t n, int64_t n_samples, unsigned parts) {
    return part_offsets(augment_workspace_layout(n, n_samples).total_bytes, n, parts, true);
}

int64_t augment_record_bytes(unsigned parts) { return record_offsets(1, parts).end; }
int64_t augment_workspace_bytes(int64_t n, int64_t n_samples, unsigned parts) { return slot_offsets(n, n_samples, parts).end; }

// ww_augment_bg -> BgDev, refusing a segment outside the bank, an empty file and a non-finite SNR (clips with enabled = 0: a zero record)
int background_prepare(const ww_augment_bg* bg_host, int64_t n, int64_t bank_len, void* records_host, bool* any_out) {
    BgDev* host = static_cast<BgDev*>(records_host);
    bool any = false;
    for (int64_t c = 0; c < n; ++c) {
        const ww_augment_bg& b = bg_host[c];
        BgDev d = {};
        if (b.enabled) {
            if (b.file_len <= 0) return fail(WW_EINVAL, "bg %lld: file_len %lld must be > 0", (long long)c, (long long)b.file_len);
            if (b.file_offset < 0 || bank_len < 0 || b.file_offset > bank_len - b.file_len)
                return fail(WW_EINVAL, "bg %lld: file [%lld, +%lld) outside the bank of %lld samples", (long long)c, (long long)b.file_offset,
                            (long long)b.file_len, (long long)bank_len);
            if (b.start < 0 || b.start >= b.file_len)
                return fail(WW_EINVAL, "bg %lld: start %lld outside [0, %lld)", (long long)c, (long long)b.start, (long long)b.file_len);
            if (!std::isfinite(b.snr_db)) return fail(WW_EINVAL, "bg %lld: snr_db must be finite", (long long)c);
            d.off = b.file_offset;
            d.len = b.file_len;
            d.start = b.start;
            d.snr_lin = std::pow(10.0, double(b.snr_db) / 10.0);
            any = true;
        }
        host[c] = d;
    }
    if (any_out) *any_out = any;
    return WW_OK;
}

// The records of `parts`, in the order rir, bg, plans (the first refusal of a batch with several faults is the first of that order).
// plans -> the per-clip records the kernels read (librosa's lengths are host arithmetic: len(np.arange), round, ceil), for clips of
// n_samples = N samples, T = 1 + N / 512 frames.  The rate bounds are the 1 s ones at every N (ceil(32 / rate) <= kAugMaxOut: the scratch
// strides and the resampler's LDS table are sized by them); the upper bound is ceil(T / rate) >= 2.
int augment_prepare(const ww_augment_plan* plans_host, const ww_augment_bg* bg_host, const ww_augment_rir* rir_host, int64_t n,
                    int64_t n_samples, int64_t bank_len, int64_t n_rirs, unsigned parts, void* records_host, AugStages* stages_out) {
    char* rec = static_cast<char*>(records_host);
    const PartOffsets at = record_offsets(n, parts);
    AugStages st = {};
    if (parts & kAugRir)
        if (int rc = rir_prepare(rir_host, n, n_rirs, rec + at.rir, &st.rir)) return rc;
    if ((parts & kAugBg) && bg_host) {
        if (int rc = background_prepare(bg_host, n, bank_len, rec + at.bg, &st.bg)) return rc;
    } else if (parts & kAugBg) {
        std::memset(rec + at.bg, 0, size_t(n) * sizeof(BgDev));
    }
    AugDev* host = reinterpret_cast<AugDev*>(rec);
    const int N = int(n_samples), T = 1 + N / kHop;
    for (int64_t c = 0; c < n; ++c) {
        const ww_augment_plan& p = plans_host[c];
        AugDev d = {};
        int64_t sh = int64_t(p.shift) % N;
        d.shift = int32_t(sh < 0 ? sh + N : sh);
        d.sigma = p.noise_sigma;
        d.seed = p.noise_seed;
        if (!(p.noise_sigma >= 0.f)) return fail(WW_EINVAL, "plan %lld: noise_sigma must be >= 0", (long long)c);
        auto steps = [T](double rate) { return int(std::ceil(double(T) / rate)); };
        auto check = [&](double rate, const char* what) {
            if (!(rate > 0.0) || int(std::ceil(double(kAugFrames) / rate)) > kAugMaxOut || steps(rate) < 2)
                return fail(WW_EUNSUPPORTED, "plan %lld: %s rate %g outside [%g, %d) for clips of %d samples", (long long)c, what, rate,
                            double(kAugFrames) / kAugMaxOut, T, N);
            return int(WW_OK);
        };
        if (p.pitch_rate != 0.0) {
            if (int rc = check(p.pitch_rate, "pitch")) return rc;
            d.p_rate = p.pitch_rate;
            d.p_out = steps(p.pitch_rate);
            d.p_len = int32_t(std::nearbyint(double(N) / p.pitch_rate));          // Python round(): half to even
            d.p_ratio = double(WW_SAMPLE_RATE) / (double(WW_SAMPLE_RATE) / p.pitch_rate);
            d.p_res = int32_t(std::ceil(double(d.p_len) * d.p_ratio));
            st.pitch = true;
        }
        if (p.stretch_rate != 0.0) {
            if (int rc = check(p.stretch_rate, "stretch")) return rc;
            d.s_rate = p.stretch_rate;
            d.s_out = steps(p.stretch_rate);
            d.s_len = int32_t(std::nearbyint(double(N) / p.stretch_rate));
            const int over = d.s_len > N ? d.s_len - N : 0;
            if (p.crop_start < 0 || p.crop_start > over)
                return fail(WW_EINVAL, "plan %lld: crop_start %d outside [0, %d] for clips of %d samples", (long long)c, p.crop_start, over, N);
            d.crop = p.crop_start;
            st.stretch = true;
        }
        host[c] = d;
    }
    if (stages_out) *stages_out = st;
    return WW_OK;
}

// The kernels alone, on records already in device memory: nothing but launches on the call's stream (capturable into a hipGraph).  A
// stage whose flag is off for a clip copies that clip through, so both vocoder stages may always be launched (what a captured graph must
// do).  With `rir` (reverb records) reverb_kernel (ww_reverb.hip) runs after the stretch; with `bg` (background records) the last launch
// is mix_kernel, which adds the background and then the same Gaussian noise, otherwise noise_kernel.
template <int kN>
static int launch_records(const AugCall& c, const AugDev* plan, const BgDev* bg, const RirDev* rir, bool any_pitch, bool any_stretch) {
    const LogmelTables* tb = device_tables();
    if (!tb) return WW_EHIP;
    const int64_t n = c.n;
    const hipStream_t stream = c.stream;
    const ww_augment_layout lay = augment_workspace_layout(n, c.n_samples);
    const int64_t row = lay.row_bytes / 4;
    char* w = static_cast<char*>(c.workspace);
    float* bufA = reinterpret_cast<float*>(w + lay.buf_a);
    float* bufB = reinterpret_cast<float*>(w + lay.buf_b);
    float2* S = reinterpret_cast<float2*>(w + lay.spec);
    float* Y = reinterpret_cast<float*>(w + lay.y);
    const int nn = int(c.n_samples);
    const dim3 egrid(unsigned((row / 4 + 255) / 256), unsigned(n));
    if (int rc = launch<roll_kernel<kN>>(egrid, dim3(256), 0, stream, c.pcm, c.stride, plan, bufA, nn)) return rc;
    float* cur = bufA;
    float* other = bufB;
    if (any_pitch) {
        if (int rc = launch<stft_pv_kernel<kN>>(dim3(unsigned(n)), dim3(256), kStftPvLds, stream, cur, plan, 0, tb, S, nn)) return rc;
        if (int rc = launch<istft_kernel<kN>>(dim3(unsigned(n)), dim3(256), kIstftLds, stream, S, plan, 0, tb, nullptr, Y, int64_t(kAugYStride), nn))
            return rc;
        if (int rc = launch<resample_kernel<kN>>(dim3(unsigned(n)), dim3(1024), kResampleLds, stream, Y, plan, tb, cur, other, nn)) return rc;
        float* t = cur; cur = other; other = t;
    }
    if (any_stretch) {
        if (int rc = launch<stft_pv_kernel<kN>>(dim3(unsigned(n)), dim3(256), kStftPvLds, stream, cur, plan, 1, tb, S, nn)) return rc;
        if (int rc = launch<istft_kernel<kN>>(dim3(unsigned(n)), dim3(256), kIstftLds, stream, S, plan, 1, tb, cur, other, row, nn)) return rc;
        float* t = cur; cur = other; other = t;
    }
    if (rir) {
        if (int rc = launch_reverb_records(cur, row, n, nn, rir, reinterpret_cast<const float2*>(c.spectra), c.n_rirs, other, row, stream))
            return rc;
        float* t = cur; cur = other; other = t;
    }
    if (bg)
        return launch<mix_kernel<kN, 16, true>>(dim3(unsigned(n)), dim3(kMixThreads), 0, stream, cur, row, plan, bg, c.bank, c.bank_len, c.out,
                                                c.out_stride, nn);
    return launch<noise_kernel<kN>>(egrid, dim3(256), 0, stream, cur, plan, c.out, c.out_stride, nn);
}

// 16000 samples run the compile-time 1 s instance (the kernels the 1 s entry points always ran), every other length the run-time one.
// bg / rir NULL: that stage is not launched
static int launch_arrays(const AugCall& c, const void* plan, const void* bg, const void* rir, bool any_pitch, bool any_stretch) {
    if (c.n == 0) return WW_OK;
    const AugDev* p = static_cast<const AugDev*>(plan);
    const BgDev* b = static_cast<const BgDev*>(bg);
    const RirDev* r = static_cast<const RirDev*>(rir);
    return c.n_samples == kClip ? launch_records<kClip>(c, p, b, r, any_pitch, any_stretch) : launch_records<0>(c, p, b, r, any_pitch, any_stretch);
}

int launch_augment_records(const AugCall& c, const void* records_dev, unsigned parts) {
    const char* rec = static_cast<const char*>(records_dev);
    const PartOffsets at = record_offsets(c.n, parts);
    return launch_arrays(c, rec, parts & kAugBg ? rec + at.bg : nullptr, parts & kAugRir ? rec + at.rir : nullptr, true, true);
}

// Pinned staging for host records: two slots per device, each guarded by an event, so a call can return as soon as its copies and
// kernels are enqueued.  Every call family shares the slots.
struct ByteStage {
    void* host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool in_use = false;
};
static std::mutex g_bstage_mu;
static ByteStage g_bstage[16][2];
static int g_bstage_next[16] = {};

int stage_to_device(const void* const* src, const size_t* sizes, void* const* dst, int pieces, hipStream_t stream) {
    size_t total = 0;
    for (int i = 0; i < pieces; ++i) total += sizes[i];
    int dev = 0;
    WW_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16) return fail(WW_EUNSUPPORTED, "device ordinal %d out of range", dev);
    std::lock_guard<std::mutex> lock(g_bstage_mu);
    ByteStage& st = g_bstage[dev][g_bstage_next[dev]];
    g_bstage_next[dev] ^= 1;
    if (st.in_use) WW_HIP(hipEventSynchronize(st.ev));             // the copies that last read this slot (two calls ago) must be done
    if (st.cap < total) {
        if (st.host) WW_HIP(hipHostFree(st.host));
        st.host = nullptr;
        st.cap = 0;
        WW_HIP(hipHostMalloc(&st.host, total, hipHostMallocDefault));
        st.cap = total;
    }
    if (!st.ev) WW_HIP(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    size_t at = 0;
    for (int i = 0; i < pieces; ++i) {
        std::memcpy(static_cast<char*>(st.host) + at, src[i], sizes[i]);
        WW_HIP(hipMemcpyAsync(dst[i], static_cast<char*>(st.host) + at, sizes[i], hipMemcpyHostToDevice, stream));
        at += sizes[i];
    }
    WW_HIP(hipEventRecord(st.ev, stream));
    st.in_use = true;
    return WW_OK;
}

// The direct calls: a stage no clip uses is neither staged nor launched, so a batch without background or reverb is one copy and the
// plain launches (noise_kernel last) through every entry point
int launch_augment(const AugCall& c, const void* records_host, unsigned parts, AugStages st) {
    if (c.n == 0) return WW_OK;
    const char* h = static_cast<const char*>(records_host);
    char* w = static_cast<char*>(c.workspace);
    const PartOffsets from = record_offsets(c.n, parts), to = slot_offsets(c.n, c.n_samples, parts);
    const size_t n = size_t(c.n);
    const void* src[3] = {h};
    size_t sizes[3] = {n * sizeof(AugDev)};
    void* dst[3] = {w};
    int pieces = 1;
    if (st.bg) { src[pieces] = h + from.bg; sizes[pieces] = n * sizeof(BgDev); dst[pieces++] = w + to.bg; }
    if (st.rir) { src[pieces] = h + from.rir; sizes[pieces] = n * sizeof(RirDev); dst[pieces++] = w + to.rir; }
    if (int rc = stage_to_device(src, sizes, dst, pieces, c.stream)) return rc;
    return launch_arrays(c, w, st.bg ? w + to.bg : nullptr, st.rir ? w + to.rir : nullptr, st.pitch, st.stretch);
}

int64_t mix_background_workspace_bytes(int64_t n) { return up256(n * int64_t(sizeof(BgDev))); }

// The mix alone (no Gaussian noise) on clips of 4000 .. 32000 samples: 16000 runs the 1 s instance, up to 16384 the run-time one with 16
// samples per thread, longer clips 32 per thread
int launch_mix_background(const AugCall& c, const void* records_host) {
    if (c.n == 0) return WW_OK;
    BgDev* bg = static_cast<BgDev*>(c.workspace);
    const size_t bytes = size_t(c.n) * sizeof(BgDev);
    void* const dst = bg;
    if (int rc = stage_to_device(&records_host, &bytes, &dst, 1, c.stream)) return rc;
    const int nn = int(c.n_samples);
    const AugDev* no_plan = nullptr;
    const dim3 grid = dim3(unsigned(c.n)), block = dim3(kMixThreads);
    if (c.n_samples == kClip)
        return launch<mix_kernel<kClip, 16, false>>(grid, block, 0, c.stream, c.pcm, c.stride, no_plan, bg, c.bank, c.bank_len, c.out, c.out_stride,
                                                    nn);
    if (c.n_samples <= 16 * kMixThreads)
        return launch<mix_kernel<0, 16, false>>(grid, block, 0, c.stream, c.pcm, c.stride, no_plan, bg, c.bank, c.bank_len, c.out, c.out_stride, nn);
    return launch<mix_kernel<0, 32, false>>(grid, block, 0, c.stream, c.pcm, c.stride, no_plan, bg, c.bank, c.bank_len, c.out, c.out_stride, nn);
}

}  // namespace ww
