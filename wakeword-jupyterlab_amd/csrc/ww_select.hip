// Online hard example mining inside the fused training step: score a candidate batch with the step's own
// criterion, keep the hardest rows, gather them.
//   hard_select_kernel<P>  one workgroup of 1024 threads, one launch, no wait.  Three phases over the n <= 65536 rows:
//                            1. score   per row P::clip(z0, z1, t).loss of ww_loss_rules.h in float64 -- the per-clip loss BEFORE the mean's
//                                       division -- and the row's rank class; the workspace gets an order-preserving 64-bit image of the
//                                       score (`key`) and one byte (rank class, and whether the row is a positive)
//                            2. select  an MSB radix select for the keep-th row of the order (rank class desc, score desc): one pass over the
//                                       rank class, then eight passes of 8 bits over the key, each an LDS histogram of the rows still in
//                                       the race (integer LDS atomics: their result does not depend on order) and a descending scan of its
//                                       256 bins by the first wave.  It ends with the threshold (class, key) and r, the number of rows AT
//                                       the threshold that are kept: the first r of them by index
//                            3. emit    an ordered prefix scan in chunks of 1024 rows: a row above the threshold lands at
//                                       (rows above before it) + min(rows at the threshold before it, r), so sel rises with the row index
//                                       and keep == n is the identity.  One lane updates the ww_select_stats record.
//                          Everything is integer once the scores exist: the same bytes from run to run.
//   select_rows_kernel     one block per kept row j: row sel[j] of mel (16-byte accesses where the row size and both pointers allow them),
//                          of the targets, the entries and the labels -> row j.  An index outside [0, n) writes zeros and reads nothing.
#include "ww_internal.h"
#include "ww_loss_rules.h"

namespace ww {

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int64_t kSelMaxRows = 65536;
constexpr uint64_t kMsb = 0x8000000000000000ull;

// The byte beside a key: the rank class in bits 0-1, bit 2 set for a counting row of class 1.
constexpr unsigned kRankMask = 3, kPositiveBit = 4;

// float64 -> uint64 whose unsigned order is the float order (-inf lowest; NaN never gets here: such a row is rank 0 with score -inf).
__device__ __forceinline__ uint64_t sortable(double x) {
    const uint64_t b = uint64_t(__double_as_longlong(x));
    return (b & kMsb) ? ~b : b | kMsb;
}
__device__ __forceinline__ uint64_t unsortable(uint64_t s) { return (s & kMsb) ? s ^ kMsb : ~s; }

// The class of a counting row, -1 for a row that does not count (ignored, bad label, invalid probability row): the policy's own test.
__device__ __forceinline__ int row_class(const PlainLabels&, const int64_t* t) { return *t == 0 || *t == 1 ? int(*t) : -1; }
__device__ __forceinline__ int row_class(const OptLabels& p, const int64_t* t) {
    int c[2] = {0, 0};
    p.tally(t, c);
    return c[1] ? 1 : c[0] ? 0 : -1;
}
__device__ __forceinline__ int row_class(const Probs&, const float* t) { return Probs::counted(t) ? (t[1] > t[0] ? 1 : 0) : -1; }

__device__ __forceinline__ int lanes_below(uint64_t mask) {
    return int(__builtin_amdgcn_mbcnt_hi(unsigned(mask >> 32), __builtin_amdgcn_mbcnt_lo(unsigned(mask), 0u)));
}

template <class P>
__global__ __launch_bounds__(kSelThreads) void hard_select_kernel(const float* __restrict__ logits, const typename P::Target* __restrict__ targets,
                                                                  int n, int keep, const P pol, int keep_class, int64_t* __restrict__ sel,
                                                                  double* __restrict__ scores, ww_select_stats* __restrict__ stats,
                                                                  uint64_t* __restrict__ keys, uint8_t* __restrict__ cls) {
    constexpr int kPer = P::kPer;
    __shared__ unsigned hist[256];
    __shared__ unsigned pick[2];                             // the chosen bin and what is still needed inside it
    __shared__ int wave_cnt[2][2][kSelWaves];               // [chunk parity][above, at][wave]
    __shared__ int red[4][kSelWaves];
    __shared__ uint64_t red_min[kSelWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- 1. score ----
    for (int i = tid; i < n; i += kSelThreads) {
        const float z0 = logits[2 * i], z1 = logits[2 * i + 1];
        typename P::Target t[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) t[j] = targets[int64_t(kPer) * i + j];
        const LossClip a = pol.clip(z0, z1, t);
        const int c = row_class(pol, t);
        const bool ranked = c >= 0 && !a.nonfinite && isfinite(a.loss);
        const unsigned rank = !ranked ? 0u : c == keep_class ? 2u : 1u;
        const double score = ranked ? a.loss : -HUGE_VAL;
        keys[i] = sortable(score);
        cls[i] = uint8_t(rank | (c == 1 ? kPositiveBit : 0u));
        if (scores) scores[i] = score;
    }

    // ---- 2. select: digit 0 is the rank class, digits 1..8 the key's bytes from the top ----
    unsigned need = unsigned(keep), thr_rank = 0;
    uint64_t prefix = 0;
    for (int pass = 0; pass <= 8; ++pass) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();                                     // the first one also publishes keys and cls to the whole workgroup
        const int shift = 64 - 8 * pass;                     // of this pass's byte (passes 1..8)
        for (int i = tid; i < n; i += kSelThreads) {
            const unsigned rank = cls[i] & kRankMask;
            if (pass == 0) {
                atomicAdd(&hist[rank], 1u);
            } else if (rank == thr_rank) {
                const uint64_t k = keys[i];
                if (pass == 1 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[unsigned(k >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        if (wave == 0) {                                     // lane L owns the bins 255 - 4L .. 252 - 4L: a descending scan
            unsigned h[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { h[j] = hist[255 - 4 * lane - j]; sum += h[j]; }
            unsigned incl = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_up(incl, off);
                if (lane >= off) incl += v;
            }
            unsigned above = incl - sum;
            if (above < need && need <= incl) {              // exactly one lane: the race never holds fewer rows than are needed
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (need > above && need <= above + h[j]) { pick[0] = unsigned(255 - 4 * lane - j); pick[1] = need - above; }
                    above += h[j];
                }
            }
        }
        __syncthreads();
        const unsigned bin = pick[0];
        need = pick[1];
        if (pass == 0) thr_rank = bin;
        else prefix |= uint64_t(bin) << shift;
    }
    const uint64_t thr_key = prefix;
    const int at_kept = int(need);                           // rows AT the threshold that are kept: the first ones by index

    // ---- 3. emit in rising row index ----
    int above_total = 0, at_total = 0;
    int positive = 0, kept_positive = 0, unranked = 0, kept_unranked = 0;
    uint64_t kept_min = ~uint64_t(0);                       // the smallest key among the kept rows: with a keep_class it need not be the threshold's
    const int chunks = (n + kSelThreads - 1) / kSelThreads;
    for (int c = 0; c < chunks; ++c) {
        const int i = c * kSelThreads + tid;
        bool above = false, at = false;
        unsigned flags = 0;
        uint64_t k = 0;
        if (i < n) {
            flags = cls[i];
            const unsigned rank = flags & kRankMask;
            k = keys[i];
            above = rank > thr_rank || (rank == thr_rank && k > thr_key);
            at = rank == thr_rank && k == thr_key;
        }
        const uint64_t m_above = __ballot(above), m_at = __ballot(at);
        if (lane == 0) { wave_cnt[c & 1][0][wave] = __popcll(m_above); wave_cnt[c & 1][1][wave] = __popcll(m_at); }
        __syncthreads();                                     // one barrier per chunk: the counts alternate between two buffers
        int above_before = above_total, at_before = at_total;
#pragma unroll
        for (int w = 0; w < kSelWaves; ++w) {
            const int a = wave_cnt[c & 1][0][w], e = wave_cnt[c & 1][1][w];
            above_total += a; at_total += e;
            if (w < wave) { above_before += a; at_before += e; }
        }
        above_before += lanes_below(m_above);
        at_before += lanes_below(m_at);
        const bool kept = above || (at && at_before < at_kept);
        if (kept) {
            const int pos = above_before + (at_before < at_kept ? at_before : at_kept);
            if (pos < keep) sel[pos] = i;
            kept_min = k < kept_min ? k : kept_min;
        }
        if (i < n) {
            const bool pos1 = (flags & kPositiveBit) != 0, r0 = (flags & kRankMask) == 0;
            positive += pos1; kept_positive += kept && pos1;
            unranked += r0; kept_unranked += kept && r0;
        }
    }
    if (stats) {
        int v[4] = {positive, kept_positive, unranked, kept_unranked};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
            if (lane == 0) red[k][wave] = v[k];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = uint64_t(__shfl_xor((unsigned long long)kept_min, off));
            kept_min = o < kept_min ? o : kept_min;
        }
        if (lane == 0) red_min[wave] = kept_min;
        __syncthreads();
        if (tid == 0) {
            int64_t t[4] = {0, 0, 0, 0};
            for (int k = 0; k < 4; ++k)
                for (int w = 0; w < kSelWaves; ++w) t[k] += red[k][w];
            uint64_t lowest = red_min[0];
            for (int w = 1; w < kSelWaves; ++w) lowest = red_min[w] < lowest ? red_min[w] : lowest;
            stats->batches += 1;
            stats->candidates += n;
            stats->kept += keep;
            stats->candidate_positive += t[0];
            stats->kept_positive += t[1];
            stats->unranked += t[2];
            stats->kept_unranked += t[3];
            stats->threshold_bits = int64_t(unsortable(lowest));
        }
    }
}

template <class P>
static int launch_select(const float* logits, const void* targets, int64_t n, int64_t keep, const P& pol, int keep_class, int64_t* sel,
                         double* scores, ww_select_stats* stats, void* workspace, hipStream_t stream) {
    uint64_t* keys = static_cast<uint64_t*>(workspace);
    uint8_t* cls = static_cast<uint8_t*>(workspace) + up256(n * int64_t(sizeof(uint64_t)));
    return launch<hard_select_kernel<P>>(dim3(1), dim3(kSelThreads), 0, stream, logits, static_cast<const typename P::Target*>(targets), int(n),
                                         int(keep), pol, keep_class, sel, scores, stats, keys, cls);
}

// ---------------------------------------------------------------------------------------------
// the row gather
// ---------------------------------------------------------------------------------------------
constexpr int kRowThreads = 256;

struct RowGather {
    const float* mel; float* mel_out;
    const void* targets; void* targets_out;
    const int64_t* entries; int64_t* entries_out;
    const int64_t* labels; int64_t* labels_out;
    int64_t n;
    int32_t row_floats, probs, wide;                        // wide: the mel rows are whole 16-byte vectors on the 16-byte grid at both ends
};

__global__ __launch_bounds__(kRowThreads) void select_rows_kernel(const int64_t* __restrict__ sel, const RowGather g) {
    const int64_t j = blockIdx.x;
    const int64_t src = sel[j];
    const bool ok = src >= 0 && src < g.n;                   // the index is compared with n before any address is formed from it
    const int tid = threadIdx.x;
    if (g.mel) {
        const float* __restrict__ in = g.mel + (ok ? src : 0) * g.row_floats;
        float* __restrict__ out = g.mel_out + j * g.row_floats;
        if (g.wide) {
            for (int v = tid; v < g.row_floats / 4; v += kRowThreads)
                reinterpret_cast<float4*>(out)[v] = ok ? reinterpret_cast<const float4*>(in)[v] : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int e = tid; e < g.row_floats; e += kRowThreads) out[e] = ok ? in[e] : 0.f;
        }
    }
    if (tid == 0 && g.targets) {
        if (g.probs) {
            const float* t = static_cast<const float*>(g.targets);
            float* o = static_cast<float*>(g.targets_out);
            o[2 * j] = ok ? t[2 * src] : 0.f;
            o[2 * j + 1] = ok ? t[2 * src + 1] : 0.f;
        } else {
            static_cast<int64_t*>(g.targets_out)[j] = ok ? static_cast<const int64_t*>(g.targets)[src] : 0;
        }
    }
    if (tid == 64 && g.entries) g.entries_out[j] = ok ? g.entries[src] : 0;
    if (tid == 128 && g.labels) g.labels_out[j] = ok ? g.labels[src] : 0;
}

static bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
static bool meets(const void* x, int64_t xb, const void* y, int64_t yb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(x), a1 = a0 + uintptr_t(xb), b0 = reinterpret_cast<uintptr_t>(y), b1 = b0 + uintptr_t(yb);
    return a0 < b1 && b0 < a1;
}

}  // namespace ww

using namespace ww;

extern "C" {

int64_t ww_hard_select_workspace_bytes(int64_t n) {
    if (n < 1 || n > kSelMaxRows) return fail(WW_EINVAL, "n %lld: expected 1..%lld", (long long)n, (long long)kSelMaxRows);
    return up256(n * int64_t(sizeof(uint64_t))) + up256(n);
}

int ww_hard_select_f32(const float* logits_dev, const void* targets_dev, int target_kind, int64_t n, int64_t keep, const ww_loss_opts* opts_host,
                       int32_t keep_class, int64_t* sel_dev, double* scores_dev, ww_select_stats* stats_dev, void* workspace_dev,
                       ww_stream_t stream) {
    if (n < 1 || n > kSelMaxRows) return fail(WW_EINVAL, "n %lld: expected 1..%lld", (long long)n, (long long)kSelMaxRows);
    if (keep < 1 || keep > n) return fail(WW_EINVAL, "keep %lld: expected 1..n = %lld", (long long)keep, (long long)n);
    if (keep_class < -1 || keep_class > 1) return fail(WW_EINVAL, "keep_class %d: expected -1 (none), 0 or 1", int(keep_class));
    const bool probs = target_kind == WW_TARGET_PROBS;
    if (target_kind != WW_TARGET_LABELS && !probs) return fail(WW_EINVAL, "target_kind %d: expected WW_TARGET_LABELS or WW_TARGET_PROBS", target_kind);
    ww_loss_opts o = {{1.0, 1.0}, 0.0, 0.0, -100, WW_LOSS_CE, WW_REDUCE_MEAN};             // NULL with probabilities: nn.CrossEntropyLoss()'s defaults
    if (opts_host) {
        o = *opts_host;
        if (int rc = check_loss_opts(o)) return rc;
        if (probs && o.kind != WW_LOSS_CE) return fail(WW_EINVAL, "kind %d: class-probability targets take WW_LOSS_CE only", int(o.kind));
        if (probs && o.ignore_index != -100)
            return fail(WW_EINVAL, "ignore_index %lld: class-probability targets take none (leave it at -100)", (long long)o.ignore_index);
    }
    if (!logits_dev || !targets_dev || !sel_dev || !workspace_dev) return fail(WW_EINVAL, "null logits / targets / sel / workspace pointer");
    if (misaligned(logits_dev, 3) || (probs && misaligned(targets_dev, 3))) return fail(WW_EINVAL, "logits_dev / targets_dev must be 4-byte aligned");
    if ((!probs && misaligned(targets_dev, 7)) || misaligned(sel_dev, 7) || misaligned(scores_dev, 7) || misaligned(stats_dev, 7))
        return fail(WW_EINVAL, "labels_dev / sel_dev / scores_dev / stats_dev must be 8-byte aligned");
    if (misaligned(workspace_dev, 255)) return fail(WW_EINVAL, "workspace_dev must be 256-byte aligned");
    if (int rc = require_gfx950()) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (probs) return launch_select(logits_dev, targets_dev, n, keep, Probs{o}, keep_class, sel_dev, scores_dev, stats_dev, workspace_dev, s);
    if (opts_host) return launch_select(logits_dev, targets_dev, n, keep, OptLabels{o}, keep_class, sel_dev, scores_dev, stats_dev, workspace_dev, s);
    return launch_select(logits_dev, targets_dev, n, keep, PlainLabels{}, keep_class, sel_dev, scores_dev, stats_dev, workspace_dev, s);
}

int ww_select_rows_f32(const float* mel_dev, int64_t n, int32_t width, const int64_t* sel_dev, int64_t keep, float* mel_out,
                       const void* targets_dev, int target_kind, void* targets_out, const int64_t* entries_dev, int64_t* entries_out,
                       const int64_t* labels_dev, int64_t* labels_out, ww_stream_t stream) {
    if (n < 1 || n > (int64_t(1) << 30)) return fail(WW_EINVAL, "n %lld: expected 1..2^30", (long long)n);
    if (keep < 1 || keep > n) return fail(WW_EINVAL, "keep %lld: expected 1..n = %lld", (long long)keep, (long long)n);
    if (width < 1 || width > WW_N_FRAMES) return fail(WW_EUNSUPPORTED, "width %d: expected 1..%d", int(width), WW_N_FRAMES);
    const bool probs = target_kind == WW_TARGET_PROBS;
    if (targets_dev && target_kind != WW_TARGET_LABELS && !probs)
        return fail(WW_EINVAL, "target_kind %d: expected WW_TARGET_LABELS or WW_TARGET_PROBS", target_kind);
    if (!sel_dev) return fail(WW_EINVAL, "null sel pointer");
    if (!mel_dev != !mel_out || !targets_dev != !targets_out || !entries_dev != !entries_out || !labels_dev != !labels_out)
        return fail(WW_EINVAL, "mel / targets / entries / labels: a source and its output must both be given or both be NULL");
    if (!mel_dev && !targets_dev && !entries_dev && !labels_dev) return fail(WW_EINVAL, "nothing to gather: every pair is NULL");
    if (misaligned(mel_dev, 3) || misaligned(mel_out, 3) || (probs && (misaligned(targets_dev, 3) || misaligned(targets_out, 3))))
        return fail(WW_EINVAL, "mel_dev / mel_out / targets_dev / targets_out must be 4-byte aligned");
    if (misaligned(sel_dev, 7) || (!probs && (misaligned(targets_dev, 7) || misaligned(targets_out, 7))) || misaligned(entries_dev, 7) ||
        misaligned(entries_out, 7) || misaligned(labels_dev, 7) || misaligned(labels_out, 7))
        return fail(WW_EINVAL, "sel_dev / labels / entries (and integer targets) must be 8-byte aligned");
    const int64_t row_floats = int64_t(WW_N_MELS) * width, tb = 8;      // a target row is 8 bytes of either kind
    if ((mel_dev && meets(mel_dev, n * row_floats * 4, mel_out, keep * row_floats * 4)) ||
        (targets_dev && meets(targets_dev, n * tb, targets_out, keep * tb)) || (entries_dev && meets(entries_dev, n * 8, entries_out, keep * 8)) ||
        (labels_dev && meets(labels_dev, n * 8, labels_out, keep * 8)))
        return fail(WW_EINVAL, "the gather is out of place: an output overlaps its source");
    if (int rc = require_gfx950()) return rc;
    RowGather g = {mel_dev, mel_out, targets_dev, targets_out, entries_dev, entries_out, labels_dev, labels_out, n, int32_t(row_floats), probs ? 1 : 0,
                   (row_floats % 4 == 0 && !misaligned(mel_dev, 15) && !misaligned(mel_out, 15)) ? 1 : 0};
    return launch<select_rows_kernel>(dim3(unsigned(keep)), dim3(kRowThreads), 0, static_cast<hipStream_t>(stream), sel_dev, g);
}

}  // extern "C"
