// Events on continuous audio: per-window scores p -> smoothed scores s -> events at a threshold with a
// refractory period.  Three kernels, each bit for bit the sequential definition:
//   smooth_kernel       q_j = p_j if finite else 0;  s_k = (sum of q over the last <= w windows of the segment, float64, ascending j) / n
//   event_sweep_kernel  counts[segment][threshold]: one workgroup per (segment, block of 256 thresholds), one thread per threshold
//   event_step_kernel   the per-hop form for the streamer, one thread per microphone, its state in device memory
// Window k of a segment fires iff s_k >= (double)theta and k >= next, where next = k_last + R + 1 after an event (0 before the first).
#include "ww_internal.h"

namespace ww {

constexpr int kSweepThreads = 256;     // thresholds per workgroup
constexpr int kSweepChunk = 2048;      // s values staged in LDS per pass (16 KiB of float64)

__device__ __forceinline__ double finite_or_zero(float p) { return __builtin_isfinite(p) ? double(p) : 0.0; }

// one thread per window; the segment of window i is found by binary search in offsets[0..n_segs].  Nothing at or past n_windows
// (the buffers' size) is read or written, whatever the table says.
__global__ __launch_bounds__(256) void smooth_kernel(const float* __restrict__ prob, const int64_t* __restrict__ offsets, int n_segs,
                                                     int64_t n_windows, int smooth, double* __restrict__ out) {
    const int64_t total = offsets[n_segs] < n_windows ? offsets[n_segs] : n_windows;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
        int lo = 0, hi = n_segs;                       // offsets[lo] <= i < offsets[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= i) lo = mid; else hi = mid;
        }
        const int64_t first = i - int64_t(smooth) + 1 > offsets[lo] ? i - int64_t(smooth) + 1 : offsets[lo];
        double acc = 0.0;
        for (int64_t j = first; j <= i; ++j) acc += finite_or_zero(prob[j]);
        out[i] = acc / double(i - first + 1);
    }
}

// grid (threshold blocks, segment lanes): a workgroup walks segments blockIdx.y, blockIdx.y + gridDim.y, ...  All lanes read the same
// s value from LDS at a time (a broadcast); the per-threshold state (next allowed window, count) stays in registers across chunks, so a
// segment of any length gives the sequential result.  fired: only with n_thr == 1, one byte per window, staged in LDS and written out
// by the whole workgroup.
__global__ __launch_bounds__(kSweepThreads) void event_sweep_kernel(const double* __restrict__ s, const int64_t* __restrict__ offsets,
                                                                    int n_segs, int64_t n_windows, const float* __restrict__ thresholds, int n_thr,
                                                                    int64_t refractory, int64_t* __restrict__ counts,
                                                                    uint8_t* __restrict__ fired) {
    __shared__ __attribute__((aligned(16))) double chunk[kSweepChunk];
    __shared__ uint8_t flags[kSweepChunk];
    const int t = blockIdx.x * kSweepThreads + threadIdx.x;
    const bool active = t < n_thr;
    const double theta = active ? double(thresholds[t]) : 2.0;
    for (int seg = blockIdx.y; seg < n_segs; seg += gridDim.y) {
        const int64_t begin = offsets[seg], end = offsets[seg + 1] < n_windows ? offsets[seg + 1] : n_windows;
        const int64_t len = begin < end ? end - begin : 0;
        int64_t next = 0, count = 0;
        for (int64_t c0 = 0; c0 < len; c0 += kSweepChunk) {
            const int n = int(len - c0 < kSweepChunk ? len - c0 : kSweepChunk);
            const double* src = s + begin + c0;
            // 16-byte loads from the first 16-byte aligned element on (segments start at any window), the odd head and tail one by one
            const int head = (reinterpret_cast<uintptr_t>(src) & 15) ? 1 : 0;
            const int pairs = (n - head) >> 1;
            if (head && threadIdx.x == 0) chunk[0] = src[0];
            for (int i = threadIdx.x; i < pairs; i += kSweepThreads) {
                const double2 v = reinterpret_cast<const double2*>(src + head)[i];
                chunk[head + 2 * i] = v.x;
                chunk[head + 2 * i + 1] = v.y;
            }
            if (head + 2 * pairs < n && threadIdx.x == 0) chunk[n - 1] = src[n - 1];
            __syncthreads();
            if (active) {
                for (int k = 0; k < n; ++k) {
                    const int64_t kk = c0 + k;
                    const bool fire = chunk[k] >= theta && kk >= next;
                    if (fire) {
                        next = kk + refractory + 1;
                        ++count;
                    }
                    if (fired) flags[k] = fire ? 1 : 0;
                }
            }
            __syncthreads();
            if (fired) {
                for (int i = threadIdx.x; i < n; i += kSweepThreads) fired[begin + c0 + i] = flags[i];
                __syncthreads();
            }
        }
        if (active) counts[int64_t(seg) * n_thr + t] = count;
    }
}

// one thread per microphone.  State per microphone (zeroed by the caller before the first hop): int64 hops seen, int64 next allowed
// window; then the ring of the last `smooth` q values as float, [n_mics][smooth].
__global__ __launch_bounds__(256) void event_step_kernel(const float* __restrict__ prob, int n_mics, int smooth, float threshold,
                                                         int64_t refractory, int64_t* __restrict__ head, float* __restrict__ ring,
                                                         uint8_t* __restrict__ fired) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_mics) return;
    const int64_t k = head[2 * m], next = head[2 * m + 1];
    const float p = prob[m];
    float* r = ring + int64_t(m) * smooth;
    r[k % smooth] = __builtin_isfinite(p) ? p : 0.f;
    const int64_t n = k + 1 < smooth ? k + 1 : smooth;
    double acc = 0.0;
    for (int64_t j = k - n + 1; j <= k; ++j) acc += double(r[j % smooth]);
    const double sk = acc / double(n);
    const bool fire = sk >= double(threshold) && k >= next;
    head[2 * m] = k + 1;
    if (fire) head[2 * m + 1] = k + refractory + 1;
    fired[m] = fire ? 1 : 0;
}

int launch_events_sweep(const float* prob, const int64_t* offsets, int n_segs, int64_t n_windows, int smooth, int64_t refractory,
                        const float* thresholds, int n_thr, int64_t* counts, uint8_t* fired, double* s_work, hipStream_t stream) {
    if (n_segs == 0) return WW_OK;
    if (n_windows > 0) {
        const int64_t blocks = (n_windows + 255) / 256;
        if (int rc = launch<smooth_kernel>(dim3(unsigned(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, prob, offsets, n_segs, n_windows,
                                           smooth, s_work)) return rc;
    }
    if (n_thr == 0) return WW_OK;
    const dim3 grid(unsigned((n_thr + kSweepThreads - 1) / kSweepThreads), unsigned(n_segs < 65535 ? n_segs : 65535));
    return launch<event_sweep_kernel>(grid, dim3(kSweepThreads), 0, stream, s_work, offsets, n_segs, n_windows, thresholds, n_thr, refractory, counts,
                                      fired);
}

int launch_events_step(const float* prob, int n_mics, int smooth, float threshold, int64_t refractory, void* state, uint8_t* fired,
                       hipStream_t stream) {
    int64_t* head = static_cast<int64_t*>(state);
    float* ring = reinterpret_cast<float*>(static_cast<char*>(state) + 16 * int64_t(n_mics));
    return launch<event_step_kernel>(dim3(unsigned((n_mics + 255) / 256)), dim3(256), 0, stream, prob, n_mics, smooth, threshold, refractory, head,
                                     ring, fired);
}

}  // namespace ww
