// Reverberation: a clip convolved with a room impulse response (RIR), advanced by the RIR's direct-path delay and rescaled to the
// clip's energy.  The KA stage between time_stretch + crop and the background mix, and the standalone ww_reverb_f32.
//
//   y[i] = sum_k h[k] x[i + dpos - k], i in [0, N)      (x zero outside [0, N); h = the kept taps, at most WW_RIR_MAX_TAPS = 16384)
//   out  = g y, g = sqrt(Ex / Ey)                       (float64 energies in a fixed order; g = 1 when Ex or Ey is 0)
//
// Overlap-save with M = 32768-point real FFTs, one block of 16384 outputs at a time:
//   rir_spectrum_kernel  at bank build: h zero-padded to M -> its real FFT, scaled by 1/M -> 16385 bins per RIR, stored in the order
//                        reverb_kernel reads them (kernel order, below)
//   reverb_kernel        one workgroup of 1024 threads per clip: for the block [i0, i0 + 16384) the segment
//                        seg[m] = x[i0 + dpos - 16384 + m], m < M -> real FFT -> * H -> inverse real FFT; circular outputs
//                        16384 .. 32767 are y[i0 .. i0 + 16383] (exact for j >= taps - 1 = 16383: the wrap touches none of them).
//                        (The segment starts at dpos - 16384 rather than dpos - 16383 so that the kept outputs are whole complex pairs.)
//                        A clip whose RIR is off is copied through unchanged.
// A real FFT of M points is one complex FFT of N = 16384 points of z[n] = seg[2n] + i seg[2n+1], then the split
//   E[k] = (Z[k] + conj Z[N-k]) / 2, O[k] = (Z[k] - conj Z[N-k]) / 2i, X[k] = E[k] + W^k O[k], X[N-k] = conj(E[k] - W^k O[k])
// (W = e^{-2 pi i / M}); the inverse runs the same forward FFT on conj(Y[k] + conj Y[N-k] + i (Y[k] - conj Y[N-k]) conj W^k).
// The 16384-point complex FFT is four-step 16 x 1024 in LDS: a 16-point DFT per thread over n1 (stride 1024) with twiddle
// W_16384^{n2 k1}, then one wave per row k1 runs ww_fft.h's wave_fft1024 on its own row (the row is the wave's slab).
// LDS: 16 rows of 1024 complex, each padded to fft::kSlabFloats (rows start 4 banks apart): 131,328 B, one workgroup per CU.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "ww_fft.h"

namespace ww {

constexpr int kRvThreads = 1024;
constexpr int kRvN = WW_RIR_MAX_TAPS;                 // 16384: complex FFT points, outputs per block, taps kept at most
constexpr int kRvRow2 = fft::kSlabFloats / 2;         // float2 per LDS row (1026)
constexpr int kRvLdsFloats = 16 * fft::kSlabFloats;   // 32832 floats = 131,328 B
static_assert(WW_RIR_FFT_SIZE == 2 * kRvN && WW_RIR_SPECTRUM_BINS == kRvN + 1, "reverb sizes");

struct RirSrc {            // one RIR for rir_spectrum_kernel
    int64_t off;           // its first tap in the taps buffer
    int64_t len;           // taps, 1 .. 16384
};

// LDS float2 index of Z[k] after fft16384 (row k & 15, position zpos(k >> 4) within the row)
__device__ __forceinline__ int rv_fpos(int k) { return (k & 15) * kRvRow2 + fft::zpos(k >> 4); }

// The 16384-point forward FFT.  In: thread t holds v[n1] = z[1024 n1 + t].  Out (after the final barrier): Z[k] at rv_fpos(k).
__device__ __forceinline__ void fft16384(float2 (&v)[16], float* lds, const LogmelTables* tb, int tid) {
    float2* lds2 = reinterpret_cast<float2*>(lds);
    fft::dft16(v);
    lds2[tid] = v[0];
#pragma unroll
    for (int k1 = 1; k1 < 16; ++k1) {
        float s, c;
        sincospif(-float(tid * k1) * (1.0f / 8192.0f), &s, &c);      // W_16384^{t k1}: the argument is exact
        lds2[k1 * kRvRow2 + tid] = fft::cmul(v[k1], make_float2(c, s));
    }
    __syncthreads();
    const int w = tid >> 6, lane = tid & 63;
    float* slab = lds + w * fft::kSlabFloats;
    const float4* s4 = reinterpret_cast<const float4*>(slab);
    float2 za[8], zb[8];
#pragma unroll
    for (int n1 = 0; n1 < 8; ++n1) {
        const float4 q = s4[64 * n1 + lane];
        za[n1] = make_float2(q.x, q.y);
        zb[n1] = make_float2(q.z, q.w);
    }
    fft::lds_order();
    fft::wave_fft1024(za, zb, slab, tb, lane);
    __syncthreads();
}

// Pair j (0..7) of thread t: the bins k and kb = N - k that one split step handles together.  Rows 1..7 pair with 15..9; row 0 with
// itself (t = 0: k = 0 with the Nyquist bin N, whose Z is Z[0]) and row 8 with itself; thread 0 also takes the self pair k = kb = 8192.
__device__ __forceinline__ void rv_pair(int j, int t, int& k, int& kb) {
    if (j < 7) k = (j + 1) + 16 * t;
    else if (t < 512) k = 16 * t;
    else k = 8 + 16 * (t - 512);
    kb = kRvN - k;
}

// Spectrum slots (kernel order): bin k of pair (j, t) at j * 1024 + t, bin kb at 8192 + j * 1024 + t, bin 8192 at 16384
__device__ __forceinline__ void rv_split(float2 a, float2 b, int k, float2& xa, float2& xb, float2& w) {
    const float2 e = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
    const float2 o = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
    float s, c;
    sincospif(-float(k) * (1.0f / 16384.0f), &s, &c);
    w = make_float2(c, s);
    const float2 wo = fft::cmul(w, o);
    xa = fft::add(e, wo);
    const float2 d = fft::sub(e, wo);
    xb = make_float2(d.x, -d.y);
}

// Build the RIR spectra: one workgroup per RIR, taps zero-padded to M, real FFT, * 1/M, kernel order.
__global__ __launch_bounds__(kRvThreads) void rir_spectrum_kernel(const float* __restrict__ taps, const RirSrc* __restrict__ src,
                                                                  const LogmelTables* __restrict__ tb, float2* __restrict__ spectra) {
    __shared__ __attribute__((aligned(16))) float lds[kRvLdsFloats];
    const int r = blockIdx.x, tid = threadIdx.x;
    const RirSrc s = src[r];
    const float* __restrict__ h = taps + s.off;
    float2 v[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
        const int m = 2 * (1024 * n1 + tid);
        v[n1] = make_float2(m < s.len ? h[m] : 0.f, m + 1 < s.len ? h[m + 1] : 0.f);
    }
    fft16384(v, lds, tb, tid);
    const float2* lds2 = reinterpret_cast<const float2*>(lds);
    float2* __restrict__ out = spectra + int64_t(r) * WW_RIR_SPECTRUM_BINS;
    constexpr float sc = 1.0f / float(WW_RIR_FFT_SIZE);
    for (int j = 0; j < 8 + (tid == 0); ++j) {
        int k, kb;
        if (j < 8) rv_pair(j, tid, k, kb);
        else k = kb = kRvN / 2;
        float2 xa, xb, w;
        rv_split(lds2[rv_fpos(k)], lds2[rv_fpos(kb & (kRvN - 1))], k, xa, xb, w);
        if (j < 8) {
            out[j * 1024 + tid] = make_float2(sc * xa.x, sc * xa.y);
            out[8192 + j * 1024 + tid] = make_float2(sc * xb.x, sc * xb.y);
        } else {
            out[kRvN] = make_float2(sc * xa.x, sc * xa.y);
        }
    }
}

// Sum of one double per thread over the workgroup: per wave by butterfly, then the 16 wave sums in wave order (every thread forms the
// same sum, in the same order).  `red` is 16 doubles of LDS that no thread reads or writes around the call.
__device__ __forceinline__ double rv_block_sum(double v, double* red, int tid) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kRvThreads / 64; ++w) s += red[w];
    return s;
}

// One clip per workgroup, kBlocks blocks of 16384 outputs (1: N <= 16384, 2: N <= 32768).  Every read of the clip precedes the first
// store (the outputs wait in registers for the gain), so `out` may alias `in` row for row.
template <int kBlocks>
__global__ __launch_bounds__(kRvThreads) void reverb_kernel(const float* in, int64_t in_stride, const RirDev* __restrict__ rir,
                                                            const float2* __restrict__ spectra, int64_t n_rirs,
                                                            const LogmelTables* __restrict__ tb, float* out, int64_t out_stride, int n) {
    __shared__ __attribute__((aligned(16))) float lds[kRvLdsFloats];
    __shared__ double red[2][kRvThreads / 64];
    const int clip = blockIdx.x, tid = threadIdx.x;
    const float* x = in + int64_t(clip) * in_stride;
    float* o = out + int64_t(clip) * out_stride;
    const RirDev rd = rir[clip];
    // a record that does not lie inside the bank (prepared against another one) reverberates nothing
    if (!(rd.index >= 0 && rd.index < n_rirs && rd.dpos >= 0 && rd.dpos < kRvN)) {
        for (int i = tid; i < n; i += kRvThreads) o[i] = x[i];
        return;
    }
    const float2* __restrict__ H = spectra + rd.index * WW_RIR_SPECTRUM_BINS;
    double ex = 0.0;
    for (int i = tid; i < n; i += kRvThreads) ex = fma(double(x[i]), double(x[i]), ex);
    float y[kBlocks][16];
    float2* lds2 = reinterpret_cast<float2*>(lds);
#pragma unroll
    for (int b = 0; b < kBlocks; ++b) {
        const int base = b * kRvN + rd.dpos - kRvN;                   // seg[m] = x[base + m]
        float2 v[16];
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) {
            const int m = base + 2 * (1024 * n1 + tid);
            v[n1] = make_float2(m >= 0 && m < n ? x[m] : 0.f, m + 1 >= 0 && m + 1 < n ? x[m + 1] : 0.f);
        }
        fft16384(v, lds, tb, tid);
        // split, * H, merge for the inverse, pair by pair in place: conj Z''[k] where Z[k] was
#pragma unroll 1
        for (int j = 0; j < 9; ++j) {
            if (j == 8 && tid != 0) break;
            int k, kb;
            if (j < 8) rv_pair(j, tid, k, kb);
            else k = kb = kRvN / 2;
            float2 xa, xb, w;
            rv_split(lds2[rv_fpos(k)], lds2[rv_fpos(kb & (kRvN - 1))], k, xa, xb, w);
            const float2 ha = j < 8 ? H[j * 1024 + tid] : H[kRvN];
            const float2 hb = j < 8 ? H[8192 + j * 1024 + tid] : ha;
            const float2 ya = fft::cmul(xa, ha), yb = fft::cmul(xb, hb);
            const float2 cw = make_float2(w.x, -w.y);
            // Z''[k] = (Ya + conj Yb) + i (Ya - conj Yb) conj W^k
            const float2 da = fft::cmul(make_float2(ya.x - yb.x, ya.y + yb.y), cw);
            const float2 zk = make_float2(ya.x + yb.x - da.y, ya.y - yb.y + da.x);
            lds2[rv_fpos(k)] = make_float2(zk.x, -zk.y);
            if (kb != k && kb < kRvN) {
                // Z''[N - k] = (Yb + conj Ya) + i (Yb - conj Ya) (-W^k)
                const float2 db = fft::cmul(make_float2(yb.x - ya.x, yb.y + ya.y), make_float2(-w.x, -w.y));
                const float2 zkb = make_float2(yb.x + ya.x - db.y, yb.y - ya.y + db.x);
                lds2[rv_fpos(kb)] = make_float2(zkb.x, -zkb.y);
            }
        }
        __syncthreads();
#pragma unroll
        for (int n1 = 0; n1 < 16; ++n1) v[n1] = lds2[rv_fpos(1024 * n1 + tid)];
        __syncthreads();                                               // fft16384 writes where other threads read
        fft16384(v, lds, tb, tid);
        // y[2n] = Re, y[2n+1] = -Im of the forward transform of the conjugate (1/M is in H); kept: n in [8192, 16384)
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const float2 z = lds2[rv_fpos(8192 + 1024 * m + tid)];
            y[b][2 * m] = z.x;
            y[b][2 * m + 1] = -z.y;
        }
        if (b + 1 < kBlocks) __syncthreads();                          // the next block's first FFT rewrites the LDS
    }
    double ey = 0.0;
#pragma unroll
    for (int b = 0; b < kBlocks; ++b)
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = b * kRvN + 2 * (1024 * m + tid) + q;
                if (i < n) ey = fma(double(y[b][2 * m + q]), double(y[b][2 * m + q]), ey);
            }
    const double sx = rv_block_sum(ex, red[0], tid);
    const double sy = rv_block_sum(ey, red[1], tid);
    const float g = (sx > 0.0 && sy > 0.0) ? float(sqrt(sx / sy)) : 1.0f;
#pragma unroll
    for (int b = 0; b < kBlocks; ++b)
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = b * kRvN + 2 * (1024 * m + tid) + q;
                if (i < n) o[i] = g * y[b][2 * m + q];
            }
}

// ------------------------------------------------------------------------------------------------
// ww_augment_rir -> RirDev, refusing an index outside the bank and a direct path outside the kept taps (enabled = 0: index -1)
int rir_prepare(const ww_augment_rir* rir_host, int64_t n, int64_t n_rirs, void* records_host, bool* any_out) {
    RirDev* host = static_cast<RirDev*>(records_host);
    bool any = false;
    for (int64_t c = 0; c < n; ++c) {
        const ww_augment_rir& r = rir_host[c];
        RirDev d = {-1, 0, 0};
        if (r.enabled) {
            if (r.index < 0 || r.index >= n_rirs)
                return fail(WW_EINVAL, "rir %lld: index %lld outside the bank of %lld", (long long)c, (long long)r.index, (long long)n_rirs);
            if (r.taps < 1 || r.taps > WW_RIR_MAX_TAPS)
                return fail(WW_EINVAL, "rir %lld: taps %d outside [1, %d]", (long long)c, r.taps, WW_RIR_MAX_TAPS);
            if (r.dpos < 0 || r.dpos >= r.taps)
                return fail(WW_EINVAL, "rir %lld: dpos %d outside the kept taps [0, %d)", (long long)c, r.dpos, r.taps);
            d.index = r.index;
            d.dpos = r.dpos;
            any = true;
        }
        host[c] = d;
    }
    if (any_out) *any_out = any;
    return WW_OK;
}

// The reverb stage on records already in device memory (launches only; capturable)
int launch_reverb_records(const float* in, int64_t in_stride, int64_t n, int n_samples, const RirDev* rir, const float2* spectra,
                          int64_t n_rirs, float* out, int64_t out_stride, hipStream_t stream) {
    if (n == 0) return WW_OK;
    const LogmelTables* tb = device_tables();
    if (!tb) return WW_EHIP;
    if (n_samples <= kRvN)
        return launch<reverb_kernel<1>>(dim3(unsigned(n)), dim3(kRvThreads), 0, stream, in, in_stride, rir, spectra, n_rirs, tb, out, out_stride,
                                        n_samples);
    return launch<reverb_kernel<2>>(dim3(unsigned(n)), dim3(kRvThreads), 0, stream, in, in_stride, rir, spectra, n_rirs, tb, out, out_stride,
                                    n_samples);
}

int64_t reverb_workspace_bytes(int64_t n) { return up256(n * int64_t(sizeof(RirDev))); }

int launch_reverb(const AugCall& c, const void* records_host) {
    if (c.n == 0) return WW_OK;
    RirDev* rec = static_cast<RirDev*>(c.workspace);
    const size_t bytes = size_t(c.n) * sizeof(RirDev);
    void* const dst = rec;
    if (int rc = stage_to_device(&records_host, &bytes, &dst, 1, c.stream)) return rc;
    return launch_reverb_records(c.pcm, c.stride, c.n, int(c.n_samples), rec, reinterpret_cast<const float2*>(c.spectra), c.n_rirs, c.out,
                                 c.out_stride, c.stream);
}

int64_t rir_spectra_workspace_bytes(int64_t n_rirs) { return up256(n_rirs * int64_t(sizeof(RirSrc))); }

int launch_rir_spectra(const float* taps, int64_t taps_len, const int64_t* offsets_host, const int32_t* lengths_host, int64_t n_rirs,
                       float* spectra, void* workspace, hipStream_t stream) {
    if (n_rirs == 0) return WW_OK;
    std::vector<RirSrc> host(static_cast<size_t>(n_rirs));
    for (int64_t r = 0; r < n_rirs; ++r) {
        const int64_t off = offsets_host[r], len = lengths_host[r];
        if (len < 1 || len > WW_RIR_MAX_TAPS)
            return fail(WW_EINVAL, "rir %lld: %lld taps outside [1, %d]", (long long)r, (long long)len, WW_RIR_MAX_TAPS);
        if (off < 0 || off > taps_len - len)
            return fail(WW_EINVAL, "rir %lld: taps [%lld, +%lld) outside the buffer of %lld", (long long)r, (long long)off, (long long)len,
                        (long long)taps_len);
        host[size_t(r)] = {off, len};
    }
    const LogmelTables* tb = device_tables();
    if (!tb) return WW_EHIP;
    RirSrc* src = static_cast<RirSrc*>(workspace);
    const void* const from = host.data();
    const size_t bytes = size_t(n_rirs) * sizeof(RirSrc);
    void* const dst = src;
    if (int rc = stage_to_device(&from, &bytes, &dst, 1, stream)) return rc;
    return launch<rir_spectrum_kernel>(dim3(unsigned(n_rirs)), dim3(kRvThreads), 0, stream, taps, src, tb, reinterpret_cast<float2*>(spectra));
}

}  // namespace ww
