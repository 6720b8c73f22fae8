// ClipLedger: a per-clip training record in device memory.  What the notebook would gather with a per-batch
// `.cpu().numpy()` loop -- which clip was seen when, whether it was classified right, how large the margin of its assigned class was -- is a
// scatter of a few integers per row, added to the ledger in stream order by one launch per batch.
//   clip_ledger_kernel       one lane per row, workgroups of 256.  A batch may name an entry more than once (positive_fraction oversamples,
//                            stream entries yield several windows) and its rows are spread over workgroups, so a record is updated with
//                            INTEGER global atomics at device scope: add, min, max and or.  Every one of them is commutative and
//                            associative, so the ledger after a set of rows does not depend on row order, batch split, geometry or run.
//                            No float atomics, no compare-and-swap loops.  The header counters are wave ballots: one atomic per wave and
//                            counter that is not zero.
//   clip_ledger_init_kernel  writes the header and clears every record, whatever the buffer held.
// Where a row may write is decided by the `n_entries` ARGUMENT alone, compared as int64: the kernels never read a device value for it.
#include <climits>

#include "ww_internal.h"

namespace ww {

constexpr int kLedThreads = 256;
constexpr int64_t kLedMaxEntries = int64_t(1) << 28;
constexpr int64_t kLedMaxRows = int64_t(1) << 30;
constexpr int kLedHeaderWords = int(sizeof(ww_ledger_header) / 8);
constexpr int kLedEntryWords = int(sizeof(ww_ledger_entry) / 8);

static_assert(sizeof(ww_ledger_header) == 64 && sizeof(ww_ledger_entry) == 56, "ledger layout");
static_assert(offsetof(ww_ledger_entry, seen) == 32 && offsetof(ww_ledger_entry, nonfinite) == 40 && offsetof(ww_ledger_entry, min_q) == 44 &&
              offsetof(ww_ledger_entry, max_q) == 48, "clip_ledger_init_kernel writes the records as 8-byte words");

typedef unsigned long long u64;

__device__ __forceinline__ void add_u64(void* p, u64 v) { __hip_atomic_fetch_add(static_cast<u64*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void or_u64(void* p, u64 v) { __hip_atomic_fetch_or(static_cast<u64*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void add_i32(int32_t* p, int32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void min_i32(int32_t* p, int32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void max_i32(int32_t* p, int32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// every lane of the wave calls this; lane 0 adds the wave's count
__device__ __forceinline__ void wave_add(int64_t* counter, bool c, int lane) {
    const u64 k = u64(__popcll(__ballot(c)));
    if (lane == 0 && k) add_u64(counter, k);
}

__global__ __launch_bounds__(kLedThreads) void clip_ledger_kernel(const float2* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                  const int64_t* __restrict__ entries, int64_t n, int epoch,
                                                                  ww_ledger_header* head, int64_t n_entries) {
    const int64_t i = int64_t(blockIdx.x) * kLedThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = i < n;
    float2 z = make_float2(0.0f, 0.0f);
    int64_t y = 0, e = -1;
    if (live) { z = logits[i]; y = labels[i]; e = entries[i]; }
    const bool skipped = live && e < 0;
    const bool bad_entry = live && e >= n_entries;                 // int64 against the argument: 2^32 + 1 is out of range, not entry 1
    const bool inside = live && e >= 0 && e < n_entries;
    const bool bad_label = inside && !(y == 0 || y == 1);
    const bool scored = inside && !bad_label;
    const float d = z.y - z.x;
    const int pred = int(z.y > z.x);                               // a tie or a NaN predicts 0
    const float m = y == 1 ? d : -d;
    const bool fin = isfinite(m);
    if (scored) {
        ww_ledger_entry* rec = reinterpret_cast<ww_ledger_entry*>(head + 1) + e;
        const bool right = pred == int(y);
        add_i32(&rec->seen, 1);
        if (right) add_i32(&rec->correct, 1);
        if (epoch >= 0) {
            const u64 bit = u64(1) << epoch;
            or_u64(&rec->seen_epochs, bit);
            if (!right) or_u64(&rec->wrong_epochs, bit);
        }
        if (!fin) {
            add_i32(&rec->nonfinite, 1);
        } else {
            const int32_t q = int32_t(rintf(fminf(fmaxf(m, -64.0f), 64.0f) * 65536.0f));
            add_u64(&rec->sum_q, u64(int64_t(q)));                  // two's complement: the unsigned add is the signed one
            add_u64(&rec->sum_q2, u64(int64_t(q) * int64_t(q)));
            min_i32(&rec->min_q, q);
            max_i32(&rec->max_q, q);
        }
    }
    wave_add(&head->rows, live, lane);
    wave_add(&head->skipped, skipped, lane);
    wave_add(&head->bad_entries, bad_entry, lane);
    wave_add(&head->bad_labels, bad_label, lane);
    wave_add(&head->nonfinite, scored && !fin, lane);
    if (i == 0) add_u64(&head->updates, 1);
}

// The buffer as 8-byte words: the header's n_entries and zeros, then per record four zero words, (seen, correct) = 0,
// (nonfinite, min_q) = (0, INT32_MAX) and (max_q, reserved) = (INT32_MIN, 0).
__global__ __launch_bounds__(kLedThreads) void clip_ledger_init_kernel(u64* __restrict__ words, int64_t n_entries) {
    const int64_t total = kLedHeaderWords + int64_t(kLedEntryWords) * n_entries;
    for (int64_t w = int64_t(blockIdx.x) * kLedThreads + threadIdx.x; w < total; w += int64_t(gridDim.x) * kLedThreads) {
        u64 v = 0;
        if (w == 0) v = u64(n_entries);
        if (w >= kLedHeaderWords) {
            const int r = int((w - kLedHeaderWords) % kLedEntryWords);
            if (r == 5) v = u64(uint32_t(INT32_MAX)) << 32;
            if (r == 6) v = u64(uint32_t(INT32_MIN));
        }
        words[w] = v;
    }
}

static int check_ledger(const void* ledger, int64_t n_entries) {
    if (n_entries < 0 || n_entries > kLedMaxEntries) return fail(WW_EINVAL, "n_entries %lld: expected 0..2^28", (long long)n_entries);
    if (!ledger) return fail(WW_EINVAL, "null ledger_dev pointer");
    if (reinterpret_cast<uintptr_t>(ledger) & 7) return fail(WW_EINVAL, "ledger_dev must be 8-byte aligned");
    return WW_OK;
}

}  // namespace ww

using namespace ww;

extern "C" {

int64_t ww_clip_ledger_bytes(int64_t n_entries) {
    if (n_entries < 0 || n_entries > kLedMaxEntries) return fail(WW_EINVAL, "n_entries %lld: expected 0..2^28", (long long)n_entries);
    return int64_t(sizeof(ww_ledger_header)) + int64_t(sizeof(ww_ledger_entry)) * n_entries;
}

int ww_clip_ledger_init(void* ledger_dev, int64_t n_entries, ww_stream_t stream) {
    if (int rc = check_ledger(ledger_dev, n_entries)) return rc;
    if (int rc = require_gfx950()) return rc;
    const int64_t total = kLedHeaderWords + int64_t(kLedEntryWords) * n_entries;
    const int64_t blocks = (total + kLedThreads - 1) / kLedThreads;
    return launch<clip_ledger_init_kernel>(dim3(unsigned(blocks < 4096 ? blocks : 4096)), dim3(kLedThreads), 0, static_cast<hipStream_t>(stream),
                                           static_cast<u64*>(ledger_dev), n_entries);
}

int ww_clip_ledger_update_f32(const float* logits_dev, const int64_t* labels_dev, const int64_t* entries_dev, int64_t n, int32_t epoch,
                              void* ledger_dev, int64_t n_entries, ww_stream_t stream) {
    if (n < 0 || n > kLedMaxRows) return fail(WW_EINVAL, "n %lld: expected 0..2^30", (long long)n);
    if (epoch < -1 || epoch > 63) return fail(WW_EINVAL, "epoch %d: expected 0..63, or -1 for no epoch bit", int(epoch));
    if (!logits_dev || !labels_dev || !entries_dev) return fail(WW_EINVAL, "null logits_dev / labels_dev / entries_dev pointer");
    if (reinterpret_cast<uintptr_t>(logits_dev) & 7) return fail(WW_EINVAL, "logits_dev must be 8-byte aligned (a row of two float32)");
    if (reinterpret_cast<uintptr_t>(labels_dev) & 7) return fail(WW_EINVAL, "labels_dev must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(entries_dev) & 7) return fail(WW_EINVAL, "entries_dev must be 8-byte aligned");
    if (int rc = check_ledger(ledger_dev, n_entries)) return rc;
    if (n == 0) return WW_OK;
    if (int rc = require_gfx950()) return rc;
    return launch<clip_ledger_kernel>(dim3(unsigned((n + kLedThreads - 1) / kLedThreads)), dim3(kLedThreads), 0, static_cast<hipStream_t>(stream),
                                      reinterpret_cast<const float2*>(logits_dev), labels_dev, entries_dev, n, int(epoch),
                                      static_cast<ww_ledger_header*>(ledger_dev), n_entries);
}

}  // extern "C"
