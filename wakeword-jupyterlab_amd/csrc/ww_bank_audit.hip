// Audit of a bank of training clips (the definitions are in include/wakeword_amd.h): one pass over a
// segment's samples, then one fold per entry.
//   bank_hops_kernel     one record per hop block (512 samples of one entry): float64 sum and sum of squares, peak, clipped and non-finite
//                        counts and the block's share of the content hash.  One wave per block, a fixed shuffle tree; reads 4 B per sample
//                        once and writes 40 B per 2 KiB read.
//   bank_entry_kernel    one wave per entry: folds the entry's records in index order and finds the active extent from the frame energies
//                        (four neighbouring blocks each).  Reads the records only: 2 % of the first pass's bytes.
// No float atomics and no order that depends on arrival: every field is the same bits from run to run, and -- a lane always owns the same
// eight samples of its block whatever the block's address -- the same bits wherever the entry lies in memory.
#include "ww_internal.h"

namespace ww {

constexpr int kAuditHop = 512;                    // WW_AUDIT_HOP
constexpr int kAuditThreads = 256;
constexpr int kAuditWaves = kAuditThreads / 64;
static_assert(WW_AUDIT_HOP == kAuditHop && kAuditHop == 64 * 8, "a lane owns eight samples of a hop block");

struct HopRec {
    double sum, sumsq;
    uint64_t hash;
    float peak;
    uint32_t clipped, nonfinite, pad_;
};
static_assert(sizeof(HopRec) == 40, "HopRec is the workspace's record");

// The largest e in [lo, n) with table[e] <= p (table[lo] <= p is the caller's): entry_of of ww_bank.hip over the prefix table of hop
// counts, so the entries without a hop block, which share a prefix, are skipped.
__device__ __forceinline__ int entry_of_hop(const int64_t* __restrict__ table, int n, int lo, int64_t p) {
    int step = 1, hi = lo + 1;
    while (hi < n && table[hi] <= p) {
        lo = hi;
        step <<= 1;
        hi = lo + step < n ? lo + step : n;
    }
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (table[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// The header's mix(bits, i): two 32-bit finalisers over two different combinations of the sample's bits and its index (the kernel
// below computes the same value with the index's words taken apart).
__host__ __device__ __forceinline__ uint64_t audit_mix(uint32_t bits, uint64_t i) {
    const uint32_t lo = uint32_t(i), hi = uint32_t(i >> 32);
    const uint32_t m = lo * 0x9E3779B1u;
    const uint32_t k1 = bits ^ m ^ (hi * 0x85EBCA77u);
    const uint32_t k2 = bits + ((m << 15) | (m >> 17)) + hi * 0xC2B2AE3Du + 0x27D4EB2Fu;
    return uint64_t(fmix32(k1)) | (uint64_t(fmix32(k2)) << 32);
}

// The entry's first sample and its length as the kernels use them: whatever the device table says, nothing outside [0, total) is named.
__device__ __forceinline__ void entry_span(const int64_t* __restrict__ offsets, int e, int64_t total, int64_t* base, int64_t* len) {
    const int64_t b = offsets[e];
    int64_t l = offsets[e + 1] - b;
    if (b < 0 || b > total || l < 0) l = 0;
    else if (l > total - b) l = total - b;
    *base = b;
    *len = l;
}

// A workgroup takes the hop blocks [hops_per_group * blockIdx.x, + hops_per_group) of the segment, its waves one block each in turn.  Lane l
// owns the block's samples 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3, so a wave's loads are contiguous: with m the phase of their address
// in floats, each four are cut from the two 16-byte-aligned vectors around them (the second one is the neighbour's first: a hit in the
// CU's cache), as bank_gather_kernel cuts its rows; a block whose vectors would reach outside the entry is read sample by sample.
__global__ __launch_bounds__(kAuditThreads) void bank_hops_kernel(const float* __restrict__ audio, int64_t total, const int64_t* __restrict__ offsets,
                                                                  const int64_t* __restrict__ hop_prefix, int n, float clip_level,
                                                                  HopRec* __restrict__ recs, int64_t hops_per_group) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const int64_t n_hops = hop_prefix[n];
    const int64_t g0 = int64_t(blockIdx.x) * hops_per_group;
    const int64_t g1 = g0 + hops_per_group < n_hops ? g0 + hops_per_group : n_hops;
    int e = 0;
    int64_t e_first = 0, e_end = 0, base = 0, len = 0;                  // the entry of the last block: its hop blocks [e_first, e_end)
    for (int64_t g = g0 + wave; g < g1; g += kAuditWaves) {
        if (g >= e_end) {                                               // most blocks follow one of the same entry: no lookup
            e = entry_of_hop(hop_prefix, n, e, g);
            e_first = hop_prefix[e];
            e_end = hop_prefix[e + 1];
            entry_span(offsets, e, total, &base, &len);
        }
        const int64_t h0 = (g - e_first) * kAuditHop;                   // the block's first sample in entry coordinates
        const bool full = h0 + kAuditHop <= len;
        float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (h0 < len) {
            const float* __restrict__ blk = audio + base + h0;
            const int m = __builtin_amdgcn_readfirstlane(int((reinterpret_cast<uintptr_t>(blk) >> 2) & 3));
            // every 16-byte vector that a full block at phase m touches lies inside the entry: [h0 - m, h0 + 512 + (4 - m) % 4)
            if (h0 - m >= 0 && h0 + kAuditHop + ((4 - m) & 3) <= len) {
                const float4* __restrict__ p = reinterpret_cast<const float4*>(blk - m) + lane;
                const float4 a0 = p[0], a1 = p[64];
                float4 v0 = a0, v1 = a1;
                if (m != 0) {
                    const float4 b0 = p[1], b1 = p[65];
                    if (m == 1) {
                        v0 = make_float4(a0.y, a0.z, a0.w, b0.x);
                        v1 = make_float4(a1.y, a1.z, a1.w, b1.x);
                    } else if (m == 2) {
                        v0 = make_float4(a0.z, a0.w, b0.x, b0.y);
                        v1 = make_float4(a1.z, a1.w, b1.x, b1.y);
                    } else {
                        v0 = make_float4(a0.w, b0.x, b0.y, b0.z);
                        v1 = make_float4(a1.w, b1.x, b1.y, b1.z);
                    }
                }
                x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w;
                x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
            } else {                                                    // an entry's first or last block: sample by sample, inside the entry
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int64_t i = 256 * (q >> 2) + 4 * lane + (q & 3);
                    if (h0 + i < len) x[q] = blk[i];
                }
            }
        }
        double sum = 0.0, sumsq = 0.0;
        uint64_t hash = 0;
        float peak = 0.f;
        uint32_t clipped = 0, nonfinite = 0;
        // The block's samples have the indices h0 + li, li < 512, and h0 is a multiple of 512: the index's high word is the block's, its
        // low word uint32(h0) + li without a carry, so the header's mix needs one multiplication per lane and block for its m.
        const int cnt = full ? kAuditHop : int(len - h0);               // the block's samples inside the entry
        const uint32_t hi = uint32_t(uint64_t(h0) >> 32);
        const uint32_t hk1 = hi * 0x85EBCA77u, hk2 = hi * 0xC2B2AE3Du + 0x27D4EB2Fu;
        const uint32_t m0 = (uint32_t(h0) + 4u * uint32_t(lane)) * 0x9E3779B1u;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int li = 256 * (q >> 2) + 4 * lane + (q & 3);
            const uint32_t bits = __float_as_uint(x[q]);                // a sample outside the entry is +0.0f here: it adds to the hash alone
            const bool finite = (bits & 0x7F800000u) != 0x7F800000u;
            const uint32_t m = m0 + 0x9E3779B1u * uint32_t(256 * (q >> 2) + (q & 3));
            const uint64_t mixed = uint64_t(fmix32(bits ^ m ^ hk1)) | (uint64_t(fmix32(bits + ((m << 15) | (m >> 17)) + hk2)) << 32);
            hash += li < cnt ? mixed : 0;
            peak = fmaxf(peak, fabsf(x[q]));                            // ww_bank_peaks_f32's fold: a NaN is passed over, an Inf stays
            const float xf = finite ? x[q] : 0.f;
            nonfinite += finite ? 0u : 1u;
            clipped += finite && fabsf(xf) >= clip_level ? 1u : 0u;
            const double d = double(xf);
            sum += d;
            sumsq = fma(d, d, sumsq);                                   // d * d is exact in float64
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sum += __shfl_xor(sum, off);
            sumsq += __shfl_xor(sumsq, off);
            hash += (unsigned long long)__shfl_xor((unsigned long long)hash, off);
            peak = fmaxf(peak, __shfl_xor(peak, off));
            clipped += __shfl_xor(clipped, off);
            nonfinite += __shfl_xor(nonfinite, off);
        }
        if (lane == 0) {
            HopRec r;
            r.sum = sum;
            r.sumsq = sumsq;
            r.hash = hash;
            r.peak = peak;
            r.clipped = clipped;
            r.nonfinite = nonfinite;
            r.pad_ = 0;
            recs[g] = r;
        }
    }
}

// Waves stride over the entries.  The float64 totals are added record by record in index order (every lane holds the same running
// total); the integer fields and the peak, whose folds are exact in any order, go lane-strided and through a tree.  Frame t's energy is
// recomputed from the four records around it in both passes, by the same additions, so the threshold test sees the bits the maximum saw.
__global__ __launch_bounds__(kAuditThreads) void bank_entry_kernel(const int64_t* __restrict__ offsets, int64_t total,
                                                                   const int64_t* __restrict__ hop_prefix, int n,
                                                                   const HopRec* __restrict__ recs, double ratio,
                                                                   ww_bank_entry_stats* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const int64_t stride = int64_t(gridDim.x) * kAuditWaves;
    for (int64_t e64 = int64_t(blockIdx.x) * kAuditWaves + wave; e64 < n; e64 += stride) {
        const int e = int(e64);
        int64_t base, len;
        entry_span(offsets, e, total, &base, &len);
        const int64_t r0 = hop_prefix[e], nh = hop_prefix[e + 1] - r0;
        const HopRec* __restrict__ rec = recs + r0;
        double sum = 0.0, sumsq = 0.0;
        uint64_t hash = 0;
        float peak = 0.f;
        int64_t clipped = 0, nonfinite = 0;
        for (int64_t c = 0; c < nh; c += 64) {
            double s = 0.0, ss = 0.0;
            if (c + lane < nh) {
                const HopRec r = rec[c + lane];
                s = r.sum;
                ss = r.sumsq;
                hash += r.hash;
                peak = fmaxf(peak, r.peak);
                clipped += r.clipped;
                nonfinite += r.nonfinite;
            }
            const int cnt = nh - c < 64 ? int(nh - c) : 64;
            for (int k = 0; k < cnt; ++k) {
                sum += __shfl(s, k);
                sumsq += __shfl(ss, k);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            hash += (unsigned long long)__shfl_xor((unsigned long long)hash, off);
            peak = fmaxf(peak, __shfl_xor(peak, off));
            clipped += (long long)__shfl_xor((long long)clipped, off);
            nonfinite += (long long)__shfl_xor((long long)nonfinite, off);
        }
        const int64_t frames = len / kAuditHop + 1;
        auto energy = [&](int64_t t) {
            const double a = t - 2 >= 0 && t - 2 < nh ? rec[t - 2].sumsq : 0.0;
            const double b = t - 1 >= 0 && t - 1 < nh ? rec[t - 1].sumsq : 0.0;
            const double c = t < nh ? rec[t].sumsq : 0.0;
            const double d = t + 1 < nh ? rec[t + 1].sumsq : 0.0;
            return ((a + b) + c) + d;
        };
        double emax = 0.0;
        for (int64_t t = lane; t < frames; t += 64) emax = fmax(emax, energy(t));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) emax = fmax(emax, __shfl_xor(emax, off));
        const double thr = emax * ratio;
        int64_t t_first = INT64_MAX, t_last = -1;
        if (emax > 0.0) {
            for (int64_t t = lane; t < frames; t += 64) {
                if (energy(t) > thr) {
                    t_first = t < t_first ? t : t_first;
                    t_last = t;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int64_t f = (long long)__shfl_xor((long long)t_first, off), l = (long long)__shfl_xor((long long)t_last, off);
            t_first = f < t_first ? f : t_first;
            t_last = l > t_last ? l : t_last;
        }
        if (lane == 0) {
            int64_t a = 0, b = 0;
            if (t_last >= 0) {
                a = kAuditHop * t_first;
                b = kAuditHop * (t_last + 1) < len ? kAuditHop * (t_last + 1) : len;
            }
            if (nonfinite > 0) {
                a = 0;
                b = len;
            }
            ww_bank_entry_stats o;
            o.sum = sum;
            o.sumsq = sumsq;
            o.max_frame_energy = emax;
            o.active_start = a;
            o.active_end = b;
            o.hash = hash;
            o.clipped = clipped;
            o.nonfinite = nonfinite;
            o.peak = peak;
            o.reserved = 0;
            stats[e] = o;
        }
    }
}

static int64_t prefix_bytes(int64_t n) { return up256((n + 1) * int64_t(sizeof(int64_t))); }

int64_t bank_audit_workspace_bytes(int64_t total, int64_t n) {
    return prefix_bytes(n) + up256((total / kAuditHop + n + 1) * int64_t(sizeof(HopRec)));     // ceil(len / 512) <= len / 512 + 1 per entry
}

int launch_bank_audit(const float* audio, int64_t total, const int64_t* offsets, const int64_t* offsets_host, int n, float clip_level,
                      double ratio, ww_bank_entry_stats* stats, void* workspace, hipStream_t stream) {
    std::vector<int64_t> prefix(size_t(n) + 1);
    prefix[0] = 0;
    for (int e = 0; e < n; ++e) prefix[size_t(e) + 1] = prefix[size_t(e)] + (offsets_host[e + 1] - offsets_host[e] + kAuditHop - 1) / kAuditHop;
    const int64_t n_hops = prefix[size_t(n)];
    const void* src = prefix.data();
    const size_t bytes = prefix.size() * sizeof(int64_t);
    void* const dst = workspace;
    if (int rc = stage_to_device(&src, &bytes, &dst, 1, stream)) return rc;
    const int64_t* hop_prefix = static_cast<const int64_t*>(workspace);
    HopRec* recs = reinterpret_cast<HopRec*>(static_cast<char*>(workspace) + prefix_bytes(n));
    const int64_t cap = int64_t(device_cu_count()) * 8;                       // memory-bound: a capped grid, contiguous blocks per workgroup
    if (n_hops > 0) {
        int64_t per = (n_hops + cap - 1) / cap;
        per = (per + kAuditWaves - 1) / kAuditWaves * kAuditWaves;
        const int64_t grid = (n_hops + per - 1) / per;
        if (int rc = launch<bank_hops_kernel>(dim3(unsigned(grid)), dim3(kAuditThreads), 0, stream, audio, total, offsets, hop_prefix, n, clip_level,
                                              recs, per)) return rc;
    }
    const int64_t groups = (int64_t(n) + kAuditWaves - 1) / kAuditWaves, ecap = cap / 2;     // the fold is light: waves stride over the entries
    return launch<bank_entry_kernel>(dim3(unsigned(groups < ecap ? groups : ecap)), dim3(kAuditThreads), 0, stream, offsets, total, hop_prefix, n,
                                     recs, ratio, stats);
}

}  // namespace ww

using namespace ww;

extern "C" {

int64_t ww_bank_audit_workspace_bytes(int64_t total_samples, int64_t n_entries) {
    if (total_samples < 0) return fail(WW_EINVAL, "total_samples %lld < 0", (long long)total_samples);
    if (n_entries < 0 || n_entries > (int64_t(1) << 30)) return fail(WW_EINVAL, "n_entries %lld out of range", (long long)n_entries);
    return bank_audit_workspace_bytes(total_samples, n_entries);
}

int ww_bank_audit_f32(const float* audio_dev, int64_t total_samples, const int64_t* offsets_dev, const int64_t* offsets_host, int64_t n_entries,
                      float clip_level, double ratio, ww_bank_entry_stats* stats_dev, void* workspace_dev, ww_stream_t stream) {
    if (total_samples < 0) return fail(WW_EINVAL, "total_samples %lld < 0", (long long)total_samples);
    if (n_entries < 0 || n_entries > (int64_t(1) << 30)) return fail(WW_EINVAL, "n_entries %lld out of range", (long long)n_entries);
    if (!(clip_level > 0.f)) return fail(WW_EINVAL, "clip_level %g: expected > 0", double(clip_level));
    if (!(ratio > 0.0 && ratio <= 1.0)) return fail(WW_EINVAL, "ratio %g: expected 0 < ratio <= 1", ratio);
    if (n_entries == 0) return WW_OK;
    if (!offsets_host) return fail(WW_EINVAL, "null offsets_host pointer");
    if (offsets_host[0] < 0) return fail(WW_EINVAL, "offsets[0] = %lld < 0", (long long)offsets_host[0]);
    for (int64_t e = 0; e < n_entries; ++e)
        if (offsets_host[e + 1] < offsets_host[e])
            return fail(WW_EINVAL, "offsets[%lld] = %lld < offsets[%lld] = %lld: not non-decreasing", (long long)(e + 1),
                        (long long)offsets_host[e + 1], (long long)e, (long long)offsets_host[e]);
    if (offsets_host[n_entries] > total_samples)
        return fail(WW_EINVAL, "offsets[%lld] = %lld passes total_samples %lld", (long long)n_entries, (long long)offsets_host[n_entries],
                    (long long)total_samples);
    if (!offsets_dev || !stats_dev || !workspace_dev || (total_samples > 0 && !audio_dev))
        return fail(WW_EINVAL, "null audio / offsets / stats / workspace pointer");
    if ((reinterpret_cast<uintptr_t>(audio_dev) & 3) || (reinterpret_cast<uintptr_t>(offsets_dev) & 7) || (reinterpret_cast<uintptr_t>(stats_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(workspace_dev) & 255))
        return fail(WW_EINVAL, "audio_dev must be 4-byte, offsets_dev / stats_dev 8-byte and workspace_dev 256-byte aligned");
    if (int rc = require_gfx950()) return rc;
    return launch_bank_audit(audio_dev, total_samples, offsets_dev, offsets_host, int(n_entries), clip_level, ratio, stats_dev, workspace_dev,
                             static_cast<hipStream_t>(stream));
}

}  // extern "C"
