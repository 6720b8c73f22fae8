// Training clips kept in device memory: a bank is one float32 buffer with its entries back to back.
//   bank_peaks_kernel    peaks[e] = fmaxf-fold of |x| over entry e (what K0 takes over a file), linear in the buffer's length
//                        however it is split into entries
//   bank_gather_kernel   windows of N samples cut from entries into the rows of a batch, zero outside the entry, as they are, divided
//                        by the entry's peak (K0's normalise-then-crop) or by the window's own peak (what the detector does per window)
// Both are memory-bound: the gather reads 4 B N bytes and writes 4 B N.
#include <cstring>

#include "ww_internal.h"

namespace ww {

// ---------------------------------------------------------------------------------------------
// peaks
// ---------------------------------------------------------------------------------------------
constexpr int kPeakThreads = 256;
constexpr int kPeakVecs = 4;                                    // 16-byte vectors per thread and chunk
constexpr int kPeakChunk = kPeakThreads * kPeakVecs * 4;        // 4096 samples per chunk
constexpr int kPeakTable = 1024;                                // entries of one chunk that are folded in LDS first

// The largest e in [lo, n) with offsets[e] <= p, galloping up from lo (offsets[lo] <= p is the caller's): the empty entries that share
// an offset are skipped, so e is the entry that holds sample p when p < offsets[n].
__device__ __forceinline__ int entry_of(const int64_t* __restrict__ offsets, int n, int lo, int64_t p) {
    int step = 1, hi = lo + 1;
    while (hi < n && offsets[hi] <= p) {
        lo = hi;
        step <<= 1;
        hi = lo + step < n ? lo + step : n;
    }
    // offsets[lo] <= p, and hi == n or offsets[hi] > p
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// The order of non-negative floats (Inf included) is the order of their bit patterns, so an unsigned atomicMax folds them exactly and in
// any arrival order.
__device__ __forceinline__ void put_peak(uint32_t* table, uint32_t* __restrict__ peaks, int e_first, int e, float m) {
    const uint32_t bits = __float_as_uint(m);
    if (bits == 0u) return;
    if (table) atomicMax(&table[e - e_first], bits);
    else atomicMax(&peaks[e], bits);
}

// Each workgroup takes a contiguous range of chunks of the buffer.  A chunk inside one entry (every chunk of a long recording but two)
// is one register / LDS reduction and one atomicMax; a chunk that holds entry boundaries folds per wave where the wave's samples share
// an entry, else per thread, into an LDS table over the chunk's entries, and then issues one atomicMax per (chunk, entry).  peaks is
// zeroed by the caller on the same stream.  Nothing outside [0, min(total, offsets[n])) is read, whatever the table says.
__global__ __launch_bounds__(kPeakThreads) void bank_peaks_kernel(const float* __restrict__ audio, int64_t total, const int64_t* __restrict__ offsets,
                                                                  int n, uint32_t* __restrict__ peaks, int64_t chunks_per_block) {
    __shared__ uint32_t table[kPeakTable];
    __shared__ float red[kPeakThreads / 64];
    __shared__ int span[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t end = offsets[n] < total ? offsets[n] : total;
    if (end <= 0) return;
    // 16-byte loads need the address aligned, not the index: vector i holds the samples 4 i - a .. 4 i - a + 3
    const int a = int((reinterpret_cast<uintptr_t>(audio) >> 2) & 3);
    const int64_t n_chunks = (end + a + kPeakChunk - 1) / kPeakChunk;
    const int64_t c0 = int64_t(blockIdx.x) * chunks_per_block;
    const int64_t c1 = c0 + chunks_per_block < n_chunks ? c0 + chunks_per_block : n_chunks;
    int hint = 0;
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t s0 = c * kPeakChunk - a > 0 ? c * kPeakChunk - a : 0;                     // the chunk's samples [s0, s1)
        const int64_t s1 = (c + 1) * kPeakChunk - a < end ? (c + 1) * kPeakChunk - a : end;
        if (tid == 0) {
            span[0] = entry_of(offsets, n, hint, s0);
            span[1] = entry_of(offsets, n, span[0], s1 - 1);
        }
        __syncthreads();
        const int e_first = span[0], e_last = span[1];
        hint = e_first;
        const bool one = e_first == e_last;
        const bool use_table = !one && e_last - e_first < kPeakTable;
        if (use_table)
            for (int i = tid; i <= e_last - e_first; i += kPeakThreads) table[i] = 0u;
        __syncthreads();
        float block_max = 0.f;
        for (int k = 0; k < kPeakVecs; ++k) {
            const int64_t p = c * kPeakChunk + 4 * int64_t((k * (kPeakThreads / 64) + wave) * 64 + lane) - a;   // first sample of this vector
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if (p >= 0 && p + 4 <= end) {
                const float4 v = *reinterpret_cast<const float4*>(audio + p);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (p + q >= 0 && p + q < end) x[q] = audio[p + q];
            }
            if (one) {
#pragma unroll
                for (int q = 0; q < 4; ++q) block_max = fmaxf(block_max, fabsf(x[q]));         // samples outside [0, end) are 0
                continue;
            }
            // the entries of this vector's first and last sample inside [s0, s1)
            const int64_t pa = p > s0 ? p : s0, pb = p + 3 < s1 - 1 ? p + 3 : s1 - 1;
            const bool any = pa <= pb;
            const int n_lim = e_last + 1;                                    // no sample of the chunk lies in an entry past e_last
            int ea = e_first, eb = e_first;
            if (any) {
                ea = entry_of(offsets, n_lim, e_first, pa);
                eb = pb == pa ? ea : entry_of(offsets, n_lim, ea, pb);
            }
            uint32_t* const tb = use_table ? table : nullptr;
            const int e_wave = __builtin_amdgcn_readfirstlane(ea);
            // (a lane without samples holds zeros and e_first; with lane 0 such a lane the others are compared with e_first)
            if (__all(!any || (ea == e_wave && eb == e_wave))) {
                float m = fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3])));
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
                if (lane == 0) put_peak(tb, peaks, e_first, e_wave, m);
            } else if (any) {
                int e = ea;
                int64_t next = offsets[e + 1];
                float m = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t s = p + q;
                    if (s < pa || s > pb) continue;
                    if (s >= next) {
                        put_peak(tb, peaks, e_first, e, m);
                        m = 0.f;
                        e = entry_of(offsets, n_lim, e, s);
                        next = offsets[e + 1];
                    }
                    m = fmaxf(m, fabsf(x[q]));
                }
                put_peak(tb, peaks, e_first, e, m);
            }
        }
        if (one) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) block_max = fmaxf(block_max, __shfl_xor(block_max, off));
            if (lane == 0) red[wave] = block_max;
            __syncthreads();
            if (tid == 0) put_peak(nullptr, peaks, e_first, e_first, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
        } else if (use_table) {
            __syncthreads();
            for (int i = tid; i <= e_last - e_first; i += kPeakThreads)
                if (table[i]) atomicMax(&peaks[e_first + i], table[i]);
        }
        __syncthreads();                                   // span, red and table are rewritten by the next chunk
    }
}

int launch_bank_peaks(const float* audio, int64_t total, const int64_t* offsets, int n, float* peaks, hipStream_t stream) {
    WW_HIP(hipMemsetAsync(peaks, 0, size_t(n) * sizeof(float), stream));
    if (total == 0) return WW_OK;
    const int64_t n_chunks = (total + 3 + kPeakChunk - 1) / kPeakChunk;
    const int64_t cap = int64_t(device_cu_count()) * 8;                       // memory-bound: a capped grid, contiguous chunks per workgroup
    const int64_t per = (n_chunks + cap - 1) / cap;
    const int64_t grid = (n_chunks + per - 1) / per;
    return launch<bank_peaks_kernel>(dim3(unsigned(grid)), dim3(kPeakThreads), 0, stream, audio, total, offsets, n,
                                     reinterpret_cast<uint32_t*>(peaks), per);
}

// ---------------------------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------------------------
constexpr int kGatherThreads = 256;

// Four source samples at entry coordinates e0 .. e0 + 3, zero outside [0, length).  `g` = audio + offset + e0 is 16-byte aligned by the
// caller's choice of e0, and the one 16-byte load is taken only where all four lie inside the entry (so inside the buffer).
__device__ __forceinline__ float4 load4(const float* __restrict__ g, int64_t e0, int64_t length) {
    if (e0 >= 0 && e0 + 4 <= length) return *reinterpret_cast<const float4*>(g);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e0 + 0 >= 0 && e0 + 0 < length) r.x = g[0];
    if (e0 + 1 >= 0 && e0 + 1 < length) r.y = g[1];
    if (e0 + 2 >= 0 && e0 + 2 < length) r.z = g[2];
    if (e0 + 3 >= 0 && e0 + 3 < length) r.w = g[3];
    return r;
}

// One workgroup per output row, a capped grid striding over the items.  Thread t owns the output columns 4 q .. 4 q + 3, q = t + 256 k,
// kV vectors in registers from the loads through the window-peak reduction to the stores (one pass over the row).  A source row is only
// 4-byte aligned: with m = its address's phase in floats, the output vector is cut from the two 16-byte-aligned source vectors around
// it (the second one is the neighbour's first: a hit in the CU's cache).  Stores are 16 bytes wide where the output row is aligned.
template <int kV>
__global__ __launch_bounds__(kGatherThreads) void bank_gather_kernel(const float* __restrict__ audio, const ww_bank_item* __restrict__ items,
                                                                     int n_items, int N, float* __restrict__ out, int64_t out_stride) {
    __shared__ float red[kGatherThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const ww_bank_item d = items[it];
        float* __restrict__ o = out + int64_t(d.row) * out_stride;
        const float* __restrict__ src = audio + d.offset + d.start;            // column 0 (never dereferenced outside the entry)
        const int m = int((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
        const int64_t lo = d.start < 0 ? -d.start : 0;                         // columns [lo, hi) lie inside the entry
        const int64_t hi = d.length - d.start < N ? d.length - d.start : N;
        float4 v[kV];
#pragma unroll
        for (int k = 0; k < kV; ++k) {
            const int col = 4 * (tid + kGatherThreads * k);
            v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (col < N && col + 4 > lo && col < hi) {
                const float4 a = load4(src + col - m, d.start + col - m, d.length);
                if (m == 0) {
                    v[k] = a;
                } else {
                    const float4 b = load4(src + col - m + 4, d.start + col - m + 4, d.length);
                    v[k] = m == 1 ? make_float4(a.y, a.z, a.w, b.x) : m == 2 ? make_float4(a.z, a.w, b.x, b.y) : make_float4(a.w, b.x, b.y, b.z);
                }
                if (col + 4 > N) {                                             // the row's last vector when N is no multiple of 4
                    if (col + 1 >= N) v[k].y = 0.f;
                    if (col + 2 >= N) v[k].z = 0.f;
                    if (col + 3 >= N) v[k].w = 0.f;
                }
            }
        }
        float div = 1.f;
        bool zero_row = false;
        if (d.norm == WW_BANK_NORM_ENTRY) {
            div = d.peak;
        } else if (d.norm == WW_BANK_NORM_WINDOW) {
            float p = 0.f;
#pragma unroll
            for (int k = 0; k < kV; ++k) p = fmaxf(fmaxf(p, fmaxf(fabsf(v[k].x), fabsf(v[k].y))), fmaxf(fabsf(v[k].z), fabsf(v[k].w)));
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) p = fmaxf(p, __shfl_xor(p, off));
            __syncthreads();                                                   // red: the previous row's readers are done
            if (lane == 0) red[wave] = p;
            __syncthreads();
            div = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
            zero_row = div == 0.f;
        }
        const bool scale = d.norm != WW_BANK_NORM_NONE && !zero_row;
        const bool wide = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
#pragma unroll
        for (int k = 0; k < kV; ++k) {
            const int col = 4 * (tid + kGatherThreads * k);
            if (col >= N) continue;
            float r[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool inside = col + q >= lo && col + q < hi;             // the pad is +0.0f and is never divided
                r[q] = !inside || zero_row ? 0.f : scale ? r[q] / div : r[q];
            }
            if (wide && col + 4 <= N) {
                *reinterpret_cast<float4*>(o + col) = make_float4(r[0], r[1], r[2], r[3]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (col + q < N) o[col + q] = r[q];
            }
        }
    }
}

int64_t bank_gather_workspace_bytes(int64_t n) { return up256(n * int64_t(sizeof(ww_bank_item))); }

int launch_bank_gather(const float* audio, const ww_bank_item* items_host, int64_t n, int N, float* out, int64_t out_stride, void* workspace,
                       hipStream_t stream) {
    if (n == 0) return WW_OK;
    const void* src = items_host;
    const size_t bytes = size_t(n) * sizeof(ww_bank_item);
    void* const dst = workspace;
    if (int rc = stage_to_device(&src, &bytes, &dst, 1, stream)) return rc;
    const ww_bank_item* items = static_cast<const ww_bank_item*>(workspace);
    const int64_t cap = int64_t(device_cu_count()) * 8;
    const dim3 grid(unsigned(n < cap ? n : cap)), block(kGatherThreads);
    if (N <= 4 * kGatherThreads * 16)
        return launch<bank_gather_kernel<16>>(grid, block, 0, stream, audio, items, int(n), N, out, out_stride);
    return launch<bank_gather_kernel<32>>(grid, block, 0, stream, audio, items, int(n), N, out, out_stride);
}

}  // namespace ww

using namespace ww;

extern "C" {

int ww_bank_peaks_f32(const float* audio_dev, int64_t total_samples, const int64_t* offsets_dev, int64_t n_entries, float* peaks_dev,
                      ww_stream_t stream) {
    if (total_samples < 0) return fail(WW_EINVAL, "total_samples %lld < 0", (long long)total_samples);
    if (n_entries < 0 || n_entries > (int64_t(1) << 30)) return fail(WW_EINVAL, "n_entries %lld out of range", (long long)n_entries);
    if (n_entries == 0) return WW_OK;
    if (!offsets_dev || !peaks_dev || (total_samples > 0 && !audio_dev)) return fail(WW_EINVAL, "null audio / offsets / peaks pointer");
    if ((reinterpret_cast<uintptr_t>(audio_dev) & 3) || (reinterpret_cast<uintptr_t>(peaks_dev) & 3) || (reinterpret_cast<uintptr_t>(offsets_dev) & 7))
        return fail(WW_EINVAL, "audio_dev / peaks_dev must be 4-byte and offsets_dev 8-byte aligned");
    if (int rc = require_gfx950()) return rc;
    return launch_bank_peaks(audio_dev, total_samples, offsets_dev, int(n_entries), peaks_dev, static_cast<hipStream_t>(stream));
}

int64_t ww_bank_gather_workspace_bytes(int64_t n_items) {
    if (n_items < 0 || n_items > (int64_t(1) << 24)) return fail(WW_EINVAL, "n_items %lld out of range", (long long)n_items);
    return bank_gather_workspace_bytes(n_items);
}

int ww_bank_gather_f32(const float* audio_dev, int64_t total_samples, const ww_bank_item* items_host, int64_t n_items, int64_t n_samples,
                       float* out_dev, int64_t n_rows, int64_t out_stride, void* workspace_dev, ww_stream_t stream) {
    const int64_t N = n_samples;
    if (N < WW_MIN_CLIP_SAMPLES || N > WW_MAX_CLIP_SAMPLES)
        return fail(WW_EINVAL, "n_samples %lld: expected %d..%d", (long long)N, WW_MIN_CLIP_SAMPLES, WW_MAX_CLIP_SAMPLES);
    if (out_stride < N) return fail(WW_EINVAL, "out_stride %lld < n_samples %lld", (long long)out_stride, (long long)N);
    if (total_samples < 0) return fail(WW_EINVAL, "total_samples %lld < 0", (long long)total_samples);
    if (n_items < 0 || n_items > (int64_t(1) << 24)) return fail(WW_EINVAL, "n_items %lld out of range", (long long)n_items);
    if (n_rows < 0 || n_rows > (int64_t(1) << 24)) return fail(WW_EINVAL, "n_rows %lld out of range", (long long)n_rows);
    if (n_items == 0) return WW_OK;
    if (!items_host) return fail(WW_EINVAL, "null items pointer");
    std::vector<bool> named(size_t(n_rows), false);
    for (int64_t i = 0; i < n_items; ++i) {
        const ww_bank_item& d = items_host[i];
        if (d.offset < 0 || d.length < 0 || d.offset > total_samples || d.length > total_samples - d.offset)
            return fail(WW_EINVAL, "item %lld: offset %lld + length %lld outside the buffer of total_samples %lld", (long long)i, (long long)d.offset,
                        (long long)d.length, (long long)total_samples);
        if (d.start < -N || d.start > d.length)
            return fail(WW_EINVAL, "item %lld: start %lld outside [-n_samples, length] = [%lld, %lld]", (long long)i, (long long)d.start,
                        (long long)-N, (long long)d.length);
        if (d.norm != WW_BANK_NORM_NONE && d.norm != WW_BANK_NORM_ENTRY && d.norm != WW_BANK_NORM_WINDOW)
            return fail(WW_EINVAL, "item %lld: unknown norm %d", (long long)i, d.norm);
        if (d.peak < 0.f) return fail(WW_EINVAL, "item %lld: peak %g < 0", (long long)i, double(d.peak));
        if (d.row < 0 || d.row >= n_rows) return fail(WW_EINVAL, "item %lld: row %d outside [0, n_rows = %lld)", (long long)i, d.row, (long long)n_rows);
        if (named[size_t(d.row)]) return fail(WW_EINVAL, "item %lld: row %d is named twice", (long long)i, d.row);
        named[size_t(d.row)] = true;
    }
    if (!audio_dev || !out_dev || !workspace_dev) return fail(WW_EINVAL, "null audio / output / workspace pointer");
    if ((reinterpret_cast<uintptr_t>(audio_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3) || (reinterpret_cast<uintptr_t>(workspace_dev) & 255))
        return fail(WW_EINVAL, "audio_dev / out_dev must be 4-byte and workspace_dev 256-byte aligned");
    if (int rc = require_gfx950()) return rc;
    return launch_bank_gather(audio_dev, items_host, n_items, int(N), out_dev, out_stride, workspace_dev, static_cast<hipStream_t>(stream));
}

}  // extern "C"
