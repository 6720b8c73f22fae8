// Clip evaluation as device counters: what notebook cell 17 gathers clip by clip on the host -- predictions
// and labels for a confusion matrix and sklearn's report -- kept as integers in a ww_clip_metrics record in device memory.
//   clip_metrics_kernel  one workgroup of 1024 lanes per batch.  The small counters (argmax confusion, the operating points, bad labels,
//                        non-finite margins) are wave ballots counted by lane-uniform code; the margin histogram of the batch is built
//                        in LDS with integer LDS adds and the touched bins are added to the record by a plain read-modify-write.
//                        Stream order serialises the calls, as for ww_loss_stats: no global atomics, no float atomics.
//   clip_metrics_clear_kernel  zeroes the counters; with `write_margins` it also stores the margins, which travel in the kernel arguments.
// Every sum is an integer sum, so the record does not depend on batch size, geometry or clip order.
#include <cmath>

#include "ww_internal.h"

namespace ww {

constexpr int kMetThreads = 1024;
constexpr int kMetWaves = kMetThreads / 64;
constexpr int kMetBins = WW_METRICS_BINS;
constexpr int kMetMaxThr = WW_METRICS_MAX_THRESHOLDS;
constexpr int kMetSmall = 4 + 2 + 4 * kMetMaxThr;          // argmax[4], bad, nonfinite, at[8][4]
constexpr int kMetCounterWords = 8 + 4 * kMetMaxThr + 2 * kMetBins;   // the int64 words in front of the margins

static_assert(sizeof(ww_clip_metrics) == size_t(kMetCounterWords) * 8 + kMetMaxThr * 4 + 8, "ww_clip_metrics layout");
static_assert(offsetof(ww_clip_metrics, margin) == size_t(kMetCounterWords) * 8, "the counters come first");

struct MetMargins { float m[kMetMaxThr]; };

__device__ __forceinline__ int wave_count(bool c) { return __popcll(__ballot(c)); }

// The bin of a FINITE margin: 1/64 wide over [-32, 32), the end bins take the rest.  d + 32 rounds once, the product with 64 is exact
// (or overflows to +inf, which the clamp takes); the clamp runs in float so that the conversion never sees a value outside int's range.
__device__ __forceinline__ int margin_bin(float d) {
    const float t = floorf((d + 32.0f) * 64.0f);
    return int(fminf(fmaxf(t, 0.0f), float(kMetBins - 1)));
}

__global__ __launch_bounds__(kMetThreads) void clip_metrics_kernel(const float2* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                   int64_t n, ww_clip_metrics* __restrict__ st) {
    __shared__ int hist[2 * kMetBins];                     // 32 KB; a call has at most 2^30 clips
    __shared__ int small[kMetWaves][kMetSmall];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = tid; b < 2 * kMetBins; b += kMetThreads) hist[b] = 0;
    const int n_thr = st->n_thresholds;
    float margin[kMetMaxThr];
#pragma unroll
    for (int k = 0; k < kMetMaxThr; ++k) margin[k] = st->margin[k];
    int cnt[kMetSmall];                                    // lane-uniform: every lane of a wave holds the wave's counts
#pragma unroll
    for (int j = 0; j < kMetSmall; ++j) cnt[j] = 0;
    __syncthreads();

    const int64_t rounds = (n + kMetThreads - 1) / kMetThreads;    // every lane of a wave runs the same rounds: the ballots need it
    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t i = r * kMetThreads + tid;
        const bool live = i < n;
        float2 z = make_float2(0.0f, 0.0f);
        int64_t y = 0;
        if (live) { z = logits[i]; y = labels[i]; }
        const bool valid = live && (y == 0 || y == 1);
        const float d = z.y - z.x;
        const bool fin = isfinite(d);
        const int cls = 2 * int(y == 1) + int(z.y > z.x);  // [label][prediction]; a tie or a NaN predicts 0
#pragma unroll
        for (int c = 0; c < 4; ++c) cnt[c] += wave_count(valid && cls == c);
        cnt[4] += wave_count(live && !valid);
        cnt[5] += wave_count(valid && !fin);
        const bool scored = valid && fin;
#pragma unroll
        for (int k = 0; k < kMetMaxThr; ++k) {
            if (k < n_thr) {
                const int c_at = 2 * int(y == 1) + int(d >= margin[k]);
#pragma unroll
                for (int c = 0; c < 4; ++c) cnt[6 + 4 * k + c] += wave_count(scored && c_at == c);
            }
        }
        if (scored) atomicAdd(&hist[int(y) * kMetBins + margin_bin(d)], 1);    // an integer add in LDS
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kMetSmall; ++j) small[wave][j] = cnt[j];
    }
    __syncthreads();

    // the record: one lane per word, a plain read-modify-write (the calls of a stream run one after another)
    if (tid < kMetSmall) {
        int64_t s = 0;
#pragma unroll
        for (int w = 0; w < kMetWaves; ++w) s += small[w][tid];
        int64_t* word = tid < 4 ? &st->argmax[0][0] + tid : tid == 4 ? &st->bad_labels : tid == 5 ? &st->nonfinite : &st->at[0][0][0] + (tid - 6);
        if (s) *word += s;
    } else if (tid == 64) {
        st->total += n;
        st->batches += 1;
    }
    int64_t* __restrict__ gh = &st->hist[0][0];
    for (int b = tid; b < 2 * kMetBins; b += kMetThreads) {
        const int h = hist[b];
        if (h) gh[b] += h;
    }
}

__global__ __launch_bounds__(256) void clip_metrics_clear_kernel(ww_clip_metrics* __restrict__ st, MetMargins margins, int n_thr, int write_margins) {
    int64_t* __restrict__ words = reinterpret_cast<int64_t*>(st);
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < kMetCounterWords; w += gridDim.x * blockDim.x) words[w] = 0;
    if (write_margins && blockIdx.x == 0 && threadIdx.x < kMetMaxThr) st->margin[threadIdx.x] = margins.m[threadIdx.x];
    if (write_margins && blockIdx.x == 0 && threadIdx.x == kMetMaxThr) { st->n_thresholds = n_thr; st->reserved = 0; }
}

static int launch_clear(ww_clip_metrics* st, const MetMargins& margins, int n_thr, int write_margins, hipStream_t stream) {
    return launch<clip_metrics_clear_kernel>(dim3((kMetCounterWords + 255) / 256), dim3(256), 0, stream, st, margins, n_thr, write_margins);
}

static bool threshold_ok(float p) { return p > 0.0f && p < 1.0f; }             // false for a NaN

static float margin_of(float p) {
    const double q = double(p);
    return float(std::log(q / (1.0 - q)));
}

static int check_state(const ww_clip_metrics* st) {
    if (!st) return fail(WW_EINVAL, "null state_dev pointer");
    if (reinterpret_cast<uintptr_t>(st) & 7) return fail(WW_EINVAL, "state_dev must be 8-byte aligned");
    return WW_OK;
}

}  // namespace ww

using namespace ww;

extern "C" {

int64_t ww_clip_metrics_bytes(void) { return int64_t(sizeof(ww_clip_metrics)); }

float ww_clip_metrics_margin_host(float p) {
    if (!threshold_ok(p)) {
        fail(WW_EINVAL, "p %g: a probability threshold lies in (0, 1)", double(p));
        return std::nanf("");
    }
    return margin_of(p);
}

int ww_clip_metrics_init(ww_clip_metrics* state_dev, const float* thresholds_host, int32_t n_thresholds, ww_stream_t stream) {
    if (int rc = check_state(state_dev)) return rc;
    if (n_thresholds < 0 || n_thresholds > kMetMaxThr) return fail(WW_EINVAL, "n_thresholds %d: expected 0..%d", int(n_thresholds), kMetMaxThr);
    if (n_thresholds > 0 && !thresholds_host) return fail(WW_EINVAL, "null thresholds_host pointer");
    MetMargins margins;
    for (int k = 0; k < kMetMaxThr; ++k) margins.m[k] = 0.0f;
    for (int k = 0; k < n_thresholds; ++k) {
        if (!threshold_ok(thresholds_host[k])) return fail(WW_EINVAL, "thresholds_host[%d] %g: expected a probability in (0, 1)", k, double(thresholds_host[k]));
        margins.m[k] = margin_of(thresholds_host[k]);
    }
    if (int rc = require_gfx950()) return rc;
    return launch_clear(state_dev, margins, n_thresholds, 1, static_cast<hipStream_t>(stream));
}

int ww_clip_metrics_reset(ww_clip_metrics* state_dev, ww_stream_t stream) {
    if (int rc = check_state(state_dev)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_clear(state_dev, MetMargins{}, 0, 0, static_cast<hipStream_t>(stream));
}

int ww_clip_metrics_update_f32(const float* logits_dev, const int64_t* labels_dev, int64_t n, ww_clip_metrics* state_dev, ww_stream_t stream) {
    if (n < 0 || n > (int64_t(1) << 30)) return fail(WW_EINVAL, "n %lld: expected 0..2^30", (long long)n);
    if (!logits_dev || !labels_dev) return fail(WW_EINVAL, "null logits_dev / labels_dev pointer");
    if (reinterpret_cast<uintptr_t>(logits_dev) & 7) return fail(WW_EINVAL, "logits_dev must be 8-byte aligned (a row of two float32)");
    if (reinterpret_cast<uintptr_t>(labels_dev) & 7) return fail(WW_EINVAL, "labels_dev must be 8-byte aligned");
    if (int rc = check_state(state_dev)) return rc;
    if (n == 0) return WW_OK;
    if (int rc = require_gfx950()) return rc;
    return launch<clip_metrics_kernel>(dim3(1), dim3(kMetThreads), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const float2*>(logits_dev),
                                       labels_dev, n, state_dev);
}

}  // extern "C"
