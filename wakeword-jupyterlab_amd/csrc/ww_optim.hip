// What sits between the training forward and backward kernels and after them: cross-entropy with its
// gradient and the epoch's running metrics, a multi-tensor Adam step, and the global gradient norm that clips it.
//   loss_kernel<P>      one workgroup: per clip the loss and d loss / d logits in float64, the batch sum folded in a fixed order and
//                       divided once, one lane updates the ww_loss_stats record (stream order serialises the calls: no atomics).  The
//                       skeleton owns the walk over the clips, the loads and stores, the counting pass and every sum; a policy P
//                       supplies the target type, the per-clip formula and the mean's denominator.  Three policies:
//                         PlainLabels  int64 labels, the mean over n (section 3h)
//                         OptLabels    labels with class weights, label smoothing, ignore_index, a sum reduction and the focal loss
//                                      (section 3k): under the mean a pass over the labels alone first gives the denominator
//                         Probs        class probabilities [n][2] with weights, smoothing, mean or sum (section 3n)
//                       All three go through softmax2 and one order of summation, so where their formulas reduce to one another
//                       (unit options, one-hot rows) so do their bits (tests/test_gpu_loss.py, tests/test_gpu_mixup.py).
//   distill_loss_kernel<P>  loss_kernel's shape with the teacher's logits as a second stream (section 3p): the hard term of OptLabels, Probs
//                       or of no target at all (NoTarget) and Hinton's teacher term, each over its own denominator, in one loss and
//                       one gradient; updates ww_loss_stats as the policy's own kernel does, and ww_distill_stats
//   adam_kernel         one launch over up to 16 tensors, the table in the kernel arguments; torch's single-tensor Adam arithmetic
//   adam_avg_kernel     the same launch with an averaged copy of the weights (EMA / SWA): after adam_one the
//                       register value of p goes through avg_one into a second tensor -- one more read and one more write per
//                       element, 36 bytes against Adam's 28 (32 when the weight is 1: the average is then written, never read);
//                       p, m and v take the path and get the bits of adam_kernel
//   weight_average_kernel  the averaging alone over the same table layout: reads p, writes the average, 12 bytes per element (8 when the
//                       weight is 1).  Both are memory-bound, 256 threads with one 16-byte vector per lane, no atomics and no LDS.
//   grad_norm_kernel    float64 partial sums of g^2 per 4096 elements; grad_norm_finish_kernel adds them and writes norm and clip scale
// All of them are memory- and latency-bound.  No float atomics anywhere: every sum has one order, so results repeat bit for bit.
#include <cmath>
#include <type_traits>

#include "ww_internal.h"
#include "ww_loss_rules.h"

namespace ww {

// ---------------------------------------------------------------------------------------------
// cross-entropy, two classes: one workgroup skeleton, three per-clip rules
// ---------------------------------------------------------------------------------------------
constexpr int kCeThreads = 256;         // the per-clip rules (LossClip, softmax2, PlainLabels, OptLabels, Probs): ww_loss_rules.h

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// The four wave sums of a 256-thread workgroup, added in wave order: the last step of every sum in this file.
template <class T>
__device__ __forceinline__ T fold_waves(const T* red) { return ((red[0] + red[1]) + red[2]) + red[3]; }

// The 16 bytes of clip pair (i, i + 1), PER elements a clip: one 16-byte load where `wide` (src on the 16-byte grid) and the pair is
// whole, single elements otherwise.  The second clip of an odd tail reads as zeros and is never used.  Zeros first, then every path
// loads into v itself: filled any other way the paths end in register copies, and the compiler puts a wait for the logits in front of
// the targets' load -- two memory latencies per pair instead of one (profiles/loss_refactor_bench.json, `first_attempt`).
template <class T, int PER>
__device__ __forceinline__ void load_pair(const T* __restrict__ src, int64_t i, bool two, bool wide, T (&v)[2 * PER]) {
    static_assert(sizeof(T) * PER * 2 == 16, "a pair of clips is 16 bytes");
    typedef T Pair __attribute__((ext_vector_type(2 * PER)));   // float4 / longlong2: 16 bytes, 16-byte aligned
#pragma unroll
    for (int j = 0; j < 2 * PER; ++j) v[j] = T(0);
    if (two && wide) {
        const Pair w = *reinterpret_cast<const Pair*>(src + PER * i);
#pragma unroll
        for (int j = 0; j < 2 * PER; ++j) v[j] = w[j];
    } else {
#pragma unroll
        for (int j = 0; j < PER; ++j) v[j] = src[PER * i + j];
        if (two) {
#pragma unroll
            for (int j = 0; j < PER; ++j) v[PER + j] = src[PER * (i + 1) + j];
        }
    }
}

// Lane t owns the clip pairs t, t + 256, ...: a pair is 16 bytes of logits and 16 bytes of targets.  Its float64 sum runs over its clips
// in rising order; the 256 lane sums are folded by the butterfly of wave_sum and the four wave sums are added in wave order -- an order
// set by kCeThreads alone.  The pointers need 4-byte (labels: 8-byte) alignment only; the 16-byte accesses are taken where they are
// aligned.  A policy with kCounts > 0 gets, when its counts_first() says so, a pass over the targets alone in front: kCounts integer
// tallies per clip, summed exactly, become the denominator every gradient is divided by; a denominator of 0 makes the batch `empty`:
// a NaN loss, as in torch, and a gradient of zeros.  The policy (the options in it) travels by value in the kernel arguments.
template <class P>
__global__ __launch_bounds__(kCeThreads) void loss_kernel(const float* __restrict__ logits, const typename P::Target* __restrict__ targets, int64_t n,
                                                          const P pol, float* __restrict__ dlogits, float* __restrict__ loss_out,
                                                          ww_loss_stats* __restrict__ stats) {
    using Target = typename P::Target;
    constexpr int kPer = P::kPer, kCounts = P::kCounts, kWaves = kCeThreads / 64;
    __shared__ double red_loss[kWaves];
    __shared__ int red_cnt[3][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool z_wide = (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    const bool t_wide = (reinterpret_cast<uintptr_t>(targets) & 15) == 0;
    const bool d_wide = (reinterpret_cast<uintptr_t>(dlogits) & 15) == 0;
    const int64_t pairs = (n + 1) >> 1;
    double inv = 1.0;                                       // 1 / denominator; 0 when the denominator is 0: such a batch moves no weight
    bool empty = false;
    if constexpr (kCounts == 0) {
        inv = 1.0 / double(n);
    } else if (pol.counts_first()) {
        __shared__ int red_tally[kCounts][kWaves];
        int c[kCounts] = {};
        for (int64_t p = tid; p < pairs; p += kCeThreads) {
            const int64_t i = 2 * p;
            const bool two = i + 1 < n;
            Target t[2 * kPer];
            load_pair<Target, kPer>(targets, i, two, t_wide, t);
            pol.tally(t, c);
            if (two) pol.tally(t + kPer, c);
        }
        int64_t totals[kCounts];
#pragma unroll
        for (int k = 0; k < kCounts; ++k) {
            c[k] = wave_sum(c[k]);
            if (lane == 0) red_tally[k][wave] = c[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kCounts; ++k) totals[k] = fold_waves(red_tally[k]);
        const double denom = pol.denominator(totals);
        empty = !(denom > 0.0);
        inv = empty ? 0.0 : 1.0 / denom;
    }
    double loss = 0.0;
    int correct = 0, bad = 0, nonfinite = 0;
    for (int64_t p = tid; p < pairs; p += kCeThreads) {
        const int64_t i = 2 * p;
        const bool two = i + 1 < n;
        float z[4];
        Target t[2 * kPer];
        load_pair<float, 2>(logits, i, two, z_wide, z);
        load_pair<Target, kPer>(targets, i, two, t_wide, t);
        const LossClip a = pol.clip(z[0], z[1], t);
        loss += a.loss; correct += a.correct; bad += a.bad; nonfinite += a.nonfinite;
        float d[4] = {float(a.d0 * inv), float(a.d1 * inv), 0.f, 0.f};
        if (two) {
            const LossClip b = pol.clip(z[2], z[3], t + kPer);
            loss += b.loss; correct += b.correct; bad += b.bad; nonfinite += b.nonfinite;
            d[2] = float(b.d0 * inv); d[3] = float(b.d1 * inv);
        }
        if (empty) d[0] = d[1] = d[2] = d[3] = 0.f;         // not 0 x NaN
        if (dlogits) {
            if (two && d_wide) {
                *reinterpret_cast<float4*>(dlogits + 2 * i) = make_float4(d[0], d[1], d[2], d[3]);
            } else {
                dlogits[2 * i] = d[0]; dlogits[2 * i + 1] = d[1];
                if (two) { dlogits[2 * i + 2] = d[2]; dlogits[2 * i + 3] = d[3]; }
            }
        }
    }
    loss = wave_sum(loss); correct = wave_sum(correct); bad = wave_sum(bad); nonfinite = wave_sum(nonfinite);
    if (lane == 0) { red_loss[wave] = loss; red_cnt[0][wave] = correct; red_cnt[1][wave] = bad; red_cnt[2][wave] = nonfinite; }
    __syncthreads();
    if (tid == 0) {
        const float value = empty ? __builtin_nanf("") : float(fold_waves(red_loss) * inv);    // a mean over nothing is NaN, as in torch; rounded once
        if (loss_out) *loss_out = value;
        if (stats) {
            stats->loss_sum += double(value);               // what `running_loss += loss.item()` adds
            stats->correct += fold_waves(red_cnt[0]);
            stats->total += n;
            stats->batches += 1;
            stats->bad_labels += fold_waves(red_cnt[1]);
            stats->nonfinite += fold_waves(red_cnt[2]);
        }
    }
}

template <class P>
static int launch_loss(const float* logits, const typename P::Target* targets, int64_t n, const P& pol, float* dlogits, float* loss,
                       ww_loss_stats* stats, hipStream_t stream) {
    return launch<loss_kernel<P>>(dim3(1), dim3(kCeThreads), 0, stream, logits, targets, n, pol, dlogits, loss, stats);
}

static int launch_ce_loss(const float* logits, const int64_t* labels, int64_t n, float* dlogits, float* loss, ww_loss_stats* stats, hipStream_t stream) {
    return launch_loss(logits, labels, n, PlainLabels{}, dlogits, loss, stats, stream);
}
static int launch_ce_loss_ex(const float* logits, const int64_t* labels, int64_t n, const ww_loss_opts& opts, float* dlogits, float* loss,
                             ww_loss_stats* stats, hipStream_t stream) {
    return launch_loss(logits, labels, n, OptLabels{opts}, dlogits, loss, stats, stream);
}
static int launch_ce_loss_soft(const float* logits, const float* targets, int64_t n, const ww_loss_opts& opts, float* dlogits, float* loss,
                               ww_loss_stats* stats, hipStream_t stream) {
    return launch_loss(logits, targets, n, Probs{opts}, dlogits, loss, stats, stream);
}

// ---------------------------------------------------------------------------------------------
// knowledge distillation: the hard term of a policy above and the teacher term in one loss
// ---------------------------------------------------------------------------------------------
// No target at all (unlabelled audio): the hard term is absent and L = T^2 KD.
struct NoTarget {};

struct DistillArgs { double alpha, temperature; int32_t reduction; };      // reduction: the policy's own, repeated where NoTarget has none

// One clip's teacher term in float64, NOT yet times T^2 or divided: kd = sum_c q_c (log q_c - log p_c) with q = softmax(zt / T) and
// p = softmax(z / T), log q_c = zt_c / T - lse (a q_c that underflows to 0 multiplies a finite difference); d_k = p_k - q_k, the
// gradient but for its factor 1 / T.  A row counts iff both teacher logits are finite.
struct KdClip { double kd, d0, d1; int counted, agree; };

__device__ __forceinline__ KdClip kd_clip(float z0f, float z1f, float t0f, float t1f, double T) {
    KdClip r;
    const bool counted = isfinite(t0f) && isfinite(t1f);
    const Softmax2 s = softmax2(double(z0f) / T, double(z1f) / T), t = softmax2(double(t0f) / T, double(t1f) / T);
    const double kd = t.p0 * ((t.z0 - t.lse) - (s.z0 - s.lse)) + t.p1 * ((t.z1 - t.lse) - (s.z1 - s.lse));
    r.kd = counted ? kd : 0.0;
    r.d0 = counted ? s.p0 - t.p0 : 0.0;
    r.d1 = counted ? s.p1 - t.p1 : 0.0;
    r.counted = counted;
    r.agree = counted && (z1f > z0f) == (t1f > t0f);         // a tie predicts class 0 on either side
    return r;
}

// loss_kernel's shape with a second 16-byte stream, the teacher's logits, beside the student's.  The pass in front always runs: it
// gives the policy's tallies (its denominator under the mean, hard_rows always) and the number of KD rows before the first gradient
// is written.  The hard term is P::clip, P::tally and P::denominator as loss_kernel uses them; the teacher's accuracy is the `correct`
// of P::clip on the TEACHER's logits (the rest of that clip is dead code).  Each term has its own denominator and its own float64 sum
// in loss_kernel's order; a term is selected into loss and gradient, never multiplied in, so one that is absent, empty or weighted 0
// contributes exactly 0 and no 0 x NaN is formed.  With alpha = 0 the selects leave (1.0 * x) + 0.0: loss_kernel<P>'s bits.
template <class P>
__global__ __launch_bounds__(kCeThreads) void distill_loss_kernel(const float* __restrict__ logits, const float* __restrict__ teacher,
                                                                  const void* __restrict__ targets_raw, int64_t n, const P pol, const DistillArgs da,
                                                                  float* __restrict__ dlogits, float* __restrict__ loss_out,
                                                                  ww_loss_stats* __restrict__ stats, ww_distill_stats* __restrict__ dstats) {
    constexpr bool kHard = !std::is_same<P, NoTarget>::value;
    using Hard = std::conditional_t<kHard, P, PlainLabels>;  // NoTarget: a target type that is never loaded, and no tallies
    using Target = typename Hard::Target;
    constexpr int kPer = Hard::kPer, kCounts = Hard::kCounts, kWaves = kCeThreads / 64;
    constexpr int kTally = kCounts + 2;                      // the policy's tallies, then KD rows and non-finite teacher rows
    const Target* __restrict__ targets = static_cast<const Target*>(targets_raw);
    __shared__ int red_tally[kTally][kWaves];
    __shared__ double red_loss[2][kWaves];
    __shared__ int red_cnt[5][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool z_wide = (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    const bool q_wide = (reinterpret_cast<uintptr_t>(teacher) & 15) == 0;
    const bool t_wide = (reinterpret_cast<uintptr_t>(targets) & 15) == 0;
    const bool d_wide = (reinterpret_cast<uintptr_t>(dlogits) & 15) == 0;
    const int64_t pairs = (n + 1) >> 1;
    const bool mean = da.reduction == WW_REDUCE_MEAN;
    const double T = da.temperature;

    int c[kTally] = {};
    for (int64_t p = tid; p < pairs; p += kCeThreads) {
        const int64_t i = 2 * p;
        const bool two = i + 1 < n;
        float q[4];
        load_pair<float, 2>(teacher, i, two, q_wide, q);
        if constexpr (kHard) {
            Target t[2 * kPer];
            load_pair<Target, kPer>(targets, i, two, t_wide, t);
            pol.tally(t, c);
            if (two) pol.tally(t + kPer, c);
        }
        const bool f0 = isfinite(q[0]) && isfinite(q[1]), f1 = two && isfinite(q[2]) && isfinite(q[3]);
        c[kCounts] += int(f0) + int(f1);
        c[kCounts + 1] += int(!f0) + int(two && !f1);
    }
    int64_t totals[kTally];
#pragma unroll
    for (int k = 0; k < kTally; ++k) {
        c[k] = wave_sum(c[k]);
        if (lane == 0) red_tally[k][wave] = c[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTally; ++k) totals[k] = fold_waves(red_tally[k]);
    const int64_t kd_rows = totals[kCounts], teacher_nonfinite = totals[kCounts + 1];
    int64_t hard_rows = 0;
    double hard_denom = 0.0;
    if constexpr (kHard) {
#pragma unroll
        for (int k = 0; k < kCounts; ++k) hard_rows += totals[k];
        hard_denom = mean ? pol.denominator(totals) : 1.0;
    }
    const double kd_denom = mean ? double(kd_rows) : 1.0;
    const bool hard_has = kHard && hard_denom > 0.0, kd_has = kd_denom > 0.0;
    const bool empty = !hard_has && !kd_has;                // under the mean only: a sum divides by 1
    const double inv_h = hard_has ? 1.0 / hard_denom : 0.0, inv_k = kd_has ? 1.0 / kd_denom : 0.0;
    const double ch = kHard ? 1.0 - da.alpha : 0.0, ck = kHard ? da.alpha : 1.0;       // the coefficients of H and of T^2 KD
    const bool hard_on = hard_has && ch > 0.0, kd_on = kd_has && ck > 0.0;
    const double gk = ck * T;                               // alpha T^2 / T: the gradient's factor on p - q

    double loss_h = 0.0, loss_k = 0.0;
    int correct = 0, bad = 0, nonfinite = 0, agree = 0, teacher_correct = 0;
    for (int64_t p = tid; p < pairs; p += kCeThreads) {
        const int64_t i = 2 * p;
        const bool two = i + 1 < n;
        float z[4], q[4];
        Target t[2 * kPer] = {};
        load_pair<float, 2>(logits, i, two, z_wide, z);
        load_pair<float, 2>(teacher, i, two, q_wide, q);
        if constexpr (kHard) load_pair<Target, kPer>(targets, i, two, t_wide, t);
        (void)t;
        float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j == 1 && !two) break;
            const float z0 = z[2 * j], z1 = z[2 * j + 1], q0 = q[2 * j], q1 = q[2 * j + 1];
            LossClip a;
            if constexpr (kHard) {
                a = pol.clip(z0, z1, t + kPer * j);
                teacher_correct += pol.clip(q0, q1, t + kPer * j).correct;
            } else {
                a.loss = a.d0 = a.d1 = 0.0;
                clip_counts(a, z0, z1, false, true, 0);     // nothing is valid and nothing is bad: `nonfinite` alone
            }
            const KdClip k = kd_clip(z0, z1, q0, q1, T);
            loss_h += a.loss; loss_k += k.kd;
            correct += a.correct; bad += a.bad; nonfinite += a.nonfinite; agree += k.agree;
            const double dh0 = hard_on ? ch * (a.d0 * inv_h) : 0.0, dh1 = hard_on ? ch * (a.d1 * inv_h) : 0.0;
            const double dk0 = kd_on ? gk * k.d0 * inv_k : 0.0, dk1 = kd_on ? gk * k.d1 * inv_k : 0.0;
            d[2 * j] = float(dh0 + dk0); d[2 * j + 1] = float(dh1 + dk1);
        }
        if (dlogits) {
            if (two && d_wide) {
                *reinterpret_cast<float4*>(dlogits + 2 * i) = make_float4(d[0], d[1], d[2], d[3]);
            } else {
                dlogits[2 * i] = d[0]; dlogits[2 * i + 1] = d[1];
                if (two) { dlogits[2 * i + 2] = d[2]; dlogits[2 * i + 3] = d[3]; }
            }
        }
    }
    loss_h = wave_sum(loss_h); loss_k = wave_sum(loss_k);
    correct = wave_sum(correct); bad = wave_sum(bad); nonfinite = wave_sum(nonfinite); agree = wave_sum(agree);
    teacher_correct = wave_sum(teacher_correct);
    if (lane == 0) {
        red_loss[0][wave] = loss_h; red_loss[1][wave] = loss_k;
        red_cnt[0][wave] = correct; red_cnt[1][wave] = bad; red_cnt[2][wave] = nonfinite; red_cnt[3][wave] = agree;
        red_cnt[4][wave] = teacher_correct;
    }
    __syncthreads();
    if (tid == 0) {
        const double hard = hard_has ? fold_waves(red_loss[0]) * inv_h : 0.0;           // H and T^2 KD, each over its own denominator
        const double kd = kd_has ? T * T * (fold_waves(red_loss[1]) * inv_k) : 0.0;
        const double total = (hard_on ? ch * hard : 0.0) + (kd_on ? ck * kd : 0.0);
        const float value = empty ? __builtin_nanf("") : float(total);                  // rounded once
        if (loss_out) *loss_out = value;
        if (stats) {
            stats->loss_sum += double(value);
            stats->correct += fold_waves(red_cnt[0]);
            stats->total += n;
            stats->batches += 1;
            stats->bad_labels += fold_waves(red_cnt[1]);
            stats->nonfinite += fold_waves(red_cnt[2]);
        }
        if (dstats) {
            dstats->hard_sum += double(float(hard));
            dstats->kd_sum += double(float(kd));
            dstats->kd_rows += kd_rows;
            dstats->hard_rows += hard_rows;
            dstats->agree += fold_waves(red_cnt[3]);
            dstats->teacher_correct += fold_waves(red_cnt[4]);
            dstats->teacher_nonfinite += teacher_nonfinite;
            dstats->batches += 1;
        }
    }
}

template <class P>
static int launch_distill(const float* logits, const float* teacher, const void* targets, int64_t n, const P& pol, const DistillArgs& da,
                          float* dlogits, float* loss, ww_loss_stats* stats, ww_distill_stats* dstats, hipStream_t stream) {
    return launch<distill_loss_kernel<P>>(dim3(1), dim3(kCeThreads), 0, stream, logits, teacher, targets, n, pol, da, dlogits, loss, stats, dstats);
}

// ---------------------------------------------------------------------------------------------
// the tensor table of the Adam and norm kernels: by value in the kernel arguments
// ---------------------------------------------------------------------------------------------
constexpr int kMaxTensors = WW_ADAM_MAX_TENSORS;
struct TensorTable {
    ww_adam_tensor t[kMaxTensors];
    int32_t first_block[kMaxTensors + 1];                   // prefix sums of the tensors' block counts
    int32_t n_tensors;
};

// The tensor a block belongs to: the largest k with first_block[k] <= block (n_tensors <= 16: a linear scan over scalars).
__device__ __forceinline__ int tensor_of(const TensorTable& tab, int block) {
    int k = 0;
    for (int j = 1; j < tab.n_tensors; ++j) k = tab.first_block[j] <= block ? j : k;
    return k;
}

// ---------------------------------------------------------------------------------------------
// Adam
// ---------------------------------------------------------------------------------------------
constexpr int kAdamThreads = 256;
constexpr int kAdamChunk = kAdamThreads * 4;                // one 16-byte vector per thread

struct AdamScalars { float lr_c1, inv_c2_sqrt, eps, omb1, beta2, omb2, weight_decay; };   // lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), ...

// torch's single-tensor Adam (no amsgrad, no maximize):  g' = g scale + wd p;  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g'^2;
// p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float scale, const AdamScalars& s) {
    g = g * scale + s.weight_decay * p;
    m = m + (g - m) * s.omb1;
    v = s.beta2 * v + s.omb2 * g * g;
    const float denom = sqrtf(v) * s.inv_c2_sqrt + s.eps;
    p = p - s.lr_c1 * (m / denom);
}

// The averaged weights: one average pointer per entry of the tensor table, and the weight w of this update
// as the host rounded it from double -- w32 = float(w), omw32 = float(1 - w).  A weight of 0 never reaches a kernel (the average
// keeps its bits: nothing is launched for it), so three rules remain.
constexpr int kAvgCopy = 0, kAvgLow = 1, kAvgHigh = 2;     // w == 1;  w32 < 0.5 (torch.lerp's threshold);  the rest
struct AvgArgs {
    float* a[kMaxTensors];
    float w32, omw32;
    int32_t rule;
};
struct NoAvg {};                                            // the plain Adam launch: no average in the kernel arguments

// torch.lerp(a, p, w) with each branch one explicit fma of the one difference p - a: nothing is left for the compiler to contract.
__device__ __forceinline__ float avg_one(float a, float p, float w32, float omw32, bool low) {
    const float d = p - a;
    return low ? fmaf(w32, d, a) : fmaf(-omw32, d, p);
}

__device__ __forceinline__ int phase_of(const void* ptr) { return int((reinterpret_cast<uintptr_t>(ptr) >> 2) & 3); }

// A block owns 256 vectors of one tensor.  Vectors are laid on the 16-byte grid of the ADDRESSES: with a = the phase of p in floats,
// vector q holds the elements 4 q - a .. 4 q - a + 3, so a tensor that starts between grid lines gets a scalar head and tail and 16-byte
// accesses between them -- when p, g, m and v share the phase (views cut the same way do); otherwise every element goes alone.
// With an average (A = AvgArgs) the value of p that is stored also goes through avg_one; under kAvgCopy the average is written and
// never loaded, so whatever it held (NaN, uninitialised memory) is gone.  The average never decides which path Adam takes: the compiler
// contracts adam_one's sums of two products differently on the two paths (v differs in its last bit), and p, m and v must be
// ww_adam_step_f32's bit for bit.  So on the 16-byte path an average of another phase is read and written one float at a time; its own
// bits do not depend on that (avg_one is explicit fmas).
template <class A>
__device__ __forceinline__ void adam_block(const TensorTable& tab, const AdamScalars& s, const float* __restrict__ grad_scale, const A& avg) {
    constexpr bool kAvg = !std::is_same<A, NoAvg>::value;
    const int k = tensor_of(tab, int(blockIdx.x));
    const ww_adam_tensor t = tab.t[k];
    const float scale = grad_scale ? *grad_scale : 1.0f;
    const int a = int((reinterpret_cast<uintptr_t>(t.p) >> 2) & 3);
    float* av = nullptr;
    bool read_avg = false, low = false, avg_wide = false;
    float w32 = 0.f, omw32 = 0.f;
    if constexpr (kAvg) {
        av = avg.a[k];
        avg_wide = a == phase_of(av);
        read_avg = avg.rule != kAvgCopy;
        low = avg.rule == kAvgLow;
        w32 = avg.w32; omw32 = avg.omw32;
    }
    const bool same = a == int((reinterpret_cast<uintptr_t>(t.g) >> 2) & 3) && a == int((reinterpret_cast<uintptr_t>(t.m) >> 2) & 3) &&
                      a == int((reinterpret_cast<uintptr_t>(t.v) >> 2) & 3);
    const int shift = same ? a : 0;
    const int64_t q = int64_t(int(blockIdx.x) - tab.first_block[k]) * kAdamThreads + threadIdx.x;
    const int64_t e0 = 4 * q - shift;                       // first element of this thread's vector
    if (e0 >= t.n) return;
    if (same && e0 >= 0 && e0 + 4 <= t.n) {
        float4 p = *reinterpret_cast<const float4*>(t.p + e0);
        const float4 g = *reinterpret_cast<const float4*>(t.g + e0);
        float4 m = *reinterpret_cast<const float4*>(t.m + e0);
        float4 v = *reinterpret_cast<const float4*>(t.v + e0);
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (kAvg) {
            if (read_avg) {
                if (avg_wide) x = *reinterpret_cast<const float4*>(av + e0);
                else x = make_float4(av[e0], av[e0 + 1], av[e0 + 2], av[e0 + 3]);
            }
        }
        adam_one(p.x, g.x, m.x, v.x, scale, s);
        adam_one(p.y, g.y, m.y, v.y, scale, s);
        adam_one(p.z, g.z, m.z, v.z, scale, s);
        adam_one(p.w, g.w, m.w, v.w, scale, s);
        *reinterpret_cast<float4*>(t.p + e0) = p;
        *reinterpret_cast<float4*>(t.m + e0) = m;
        *reinterpret_cast<float4*>(t.v + e0) = v;
        if constexpr (kAvg) {
            if (read_avg) {
                x.x = avg_one(x.x, p.x, w32, omw32, low);
                x.y = avg_one(x.y, p.y, w32, omw32, low);
                x.z = avg_one(x.z, p.z, w32, omw32, low);
                x.w = avg_one(x.w, p.w, w32, omw32, low);
            } else {
                x = p;
            }
            if (avg_wide) {
                *reinterpret_cast<float4*>(av + e0) = x;
            } else {
                av[e0] = x.x; av[e0 + 1] = x.y; av[e0 + 2] = x.z; av[e0 + 3] = x.w;
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t e = e0 + j;
        if (e < 0 || e >= t.n) continue;
        float p = t.p[e], m = t.m[e], v = t.v[e];
        adam_one(p, t.g[e], m, v, scale, s);
        t.p[e] = p; t.m[e] = m; t.v[e] = v;
        if constexpr (kAvg) av[e] = read_avg ? avg_one(av[e], p, w32, omw32, low) : p;
    }
}

__global__ __launch_bounds__(kAdamThreads) void adam_kernel(const TensorTable tab, const AdamScalars s, const float* __restrict__ grad_scale) {
    adam_block(tab, s, grad_scale, NoAvg{});
}

__global__ __launch_bounds__(kAdamThreads) void adam_avg_kernel(const TensorTable tab, const AdamScalars s, const float* __restrict__ grad_scale,
                                                                const AvgArgs avg) {
    adam_block(tab, s, grad_scale, avg);
}

// The averaging alone: avg_one over the p of every entry (g, m and v of the table are not read), the block decomposition of adam_kernel
// with the phases of p and the average deciding between the 16-byte and the one-float path.  The bits are those of adam_avg_kernel.
__global__ __launch_bounds__(kAdamThreads) void weight_average_kernel(const TensorTable tab, const AvgArgs avg) {
    const int k = tensor_of(tab, int(blockIdx.x));
    const float* __restrict__ src = tab.t[k].p;
    float* __restrict__ av = avg.a[k];
    const int64_t n = tab.t[k].n;
    const int a = phase_of(src);
    const bool same = a == phase_of(av);
    const bool read_avg = avg.rule != kAvgCopy, low = avg.rule == kAvgLow;
    const float w32 = avg.w32, omw32 = avg.omw32;
    const int shift = same ? a : 0;
    const int64_t q = int64_t(int(blockIdx.x) - tab.first_block[k]) * kAdamThreads + threadIdx.x;
    const int64_t e0 = 4 * q - shift;
    if (e0 >= n) return;
    if (same && e0 >= 0 && e0 + 4 <= n) {
        const float4 p = *reinterpret_cast<const float4*>(src + e0);
        float4 x = p;
        if (read_avg) {
            x = *reinterpret_cast<const float4*>(av + e0);
            x.x = avg_one(x.x, p.x, w32, omw32, low);
            x.y = avg_one(x.y, p.y, w32, omw32, low);
            x.z = avg_one(x.z, p.z, w32, omw32, low);
            x.w = avg_one(x.w, p.w, w32, omw32, low);
        }
        *reinterpret_cast<float4*>(av + e0) = x;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t e = e0 + j;
        if (e < 0 || e >= n) continue;
        const float p = src[e];
        av[e] = read_avg ? avg_one(av[e], p, w32, omw32, low) : p;
    }
}

// Blocks of `chunk` elements per tensor (+3: the phase shift can push the last elements into one more vector).
static int fill_table(const ww_adam_tensor* tensors, int n_tensors, int chunk, TensorTable* tab) {
    int64_t blocks = 0;
    for (int k = 0; k < n_tensors; ++k) {
        tab->t[k] = tensors[k];
        tab->first_block[k] = int32_t(blocks);
        blocks += (tensors[k].n + 3 + chunk - 1) / chunk;
        if (blocks > (int64_t(1) << 30)) return fail(WW_EUNSUPPORTED, "tensors[%d].n: the table needs more than 2^30 blocks", k);
    }
    for (int k = n_tensors; k <= kMaxTensors; ++k) tab->first_block[k] = int32_t(blocks);
    for (int k = n_tensors; k < kMaxTensors; ++k) tab->t[k] = ww_adam_tensor{nullptr, nullptr, nullptr, nullptr, 0};
    tab->n_tensors = n_tensors;
    return WW_OK;
}

int launch_adam(const ww_adam_tensor* tensors, int n_tensors, const AdamScalars& s, const float* grad_scale, hipStream_t stream) {
    TensorTable tab;
    if (int rc = fill_table(tensors, n_tensors, kAdamChunk, &tab)) return rc;
    return launch<adam_kernel>(dim3(unsigned(tab.first_block[kMaxTensors])), dim3(kAdamThreads), 0, stream, tab, s, grad_scale);
}

// The kernel arguments of an averaging launch from the weight in double: the two float32 roundings and the rule.  The comparison with
// 0.5 is made on w32, the value torch.lerp compares.  Callers send a weight of 0 nowhere near a kernel.
static AvgArgs avg_args(float* const* avg, int n_tensors, double weight) {
    AvgArgs a;
    for (int k = 0; k < kMaxTensors; ++k) a.a[k] = k < n_tensors ? avg[k] : nullptr;
    a.w32 = float(weight);
    a.omw32 = float(1.0 - weight);
    a.rule = weight == 1.0 ? kAvgCopy : a.w32 < 0.5f ? kAvgLow : kAvgHigh;
    return a;
}

int launch_adam_avg(const ww_adam_tensor* tensors, float* const* avg, int n_tensors, const AdamScalars& s, const float* grad_scale, double weight,
                    hipStream_t stream) {
    if (weight == 0.0) return launch_adam(tensors, n_tensors, s, grad_scale, stream);      // the average keeps its bits: the plain kernel
    TensorTable tab;
    if (int rc = fill_table(tensors, n_tensors, kAdamChunk, &tab)) return rc;
    return launch<adam_avg_kernel>(dim3(unsigned(tab.first_block[kMaxTensors])), dim3(kAdamThreads), 0, stream, tab, s, grad_scale,
                                   avg_args(avg, n_tensors, weight));
}

int launch_weight_average(const ww_adam_tensor* tensors, float* const* avg, int n_tensors, double weight, hipStream_t stream) {
    if (weight == 0.0) return WW_OK;                        // nothing moves: nothing is launched
    TensorTable tab;
    ww_adam_tensor only_p[kMaxTensors];                     // g, m and v of the caller's table are not read: they do not travel either
    for (int k = 0; k < n_tensors; ++k) only_p[k] = ww_adam_tensor{tensors[k].p, nullptr, nullptr, nullptr, tensors[k].n};
    if (int rc = fill_table(only_p, n_tensors, kAdamChunk, &tab)) return rc;
    return launch<weight_average_kernel>(dim3(unsigned(tab.first_block[kMaxTensors])), dim3(kAdamThreads), 0, stream, tab,
                                         avg_args(avg, n_tensors, weight));
}

// ---------------------------------------------------------------------------------------------
// global L2 norm of the table's gradients, and the clip scale
// ---------------------------------------------------------------------------------------------
constexpr int kNormThreads = 256;
constexpr int kNormVecs = 4;
constexpr int kNormChunk = kNormThreads * kNormVecs * 4;    // 4096 elements per partial sum

// partial[block] = sum of g^2 over elements [4096 c, 4096 c + 4096) of the block's tensor, in float64: thread t adds its elements
// 4 (t + 256 j) .. + 3, j = 0 .. 3, in rising order, then the butterfly and the wave order of loss_kernel.  The order is in ELEMENT
// coordinates, so it does not move with the pointer's alignment (a g off the 16-byte grid is read one float at a time).
__global__ __launch_bounds__(kNormThreads) void grad_norm_kernel(const TensorTable tab, double* __restrict__ partial) {
    __shared__ double red[kNormThreads / 64];
    const int k = tensor_of(tab, int(blockIdx.x));
    const float* __restrict__ g = tab.t[k].g;
    const int64_t n = tab.t[k].n;
    const bool wide = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    const int64_t base = int64_t(int(blockIdx.x) - tab.first_block[k]) * kNormChunk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kNormVecs; ++j) {
        const int64_t e0 = base + 4 * int64_t(tid + kNormThreads * j);
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (wide && e0 + 4 <= n) {
            const float4 v = *reinterpret_cast<const float4*>(g + e0);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e0 + i < n) x[i] = g[e0 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc += double(x[i]) * double(x[i]);
    }
    acc = wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = fold_waves(red);
}

// One workgroup: thread t adds the partials t, t + 256, ... in rising order; same fold.  scale = min(1, max_norm / (norm + 1e-6)).
__global__ __launch_bounds__(kNormThreads) void grad_norm_finish_kernel(const double* __restrict__ partial, int n_partial, double max_norm,
                                                                        double* __restrict__ norm_out, float* __restrict__ scale_out) {
    __shared__ double red[kNormThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc = 0.0;
    for (int i = tid; i < n_partial; i += kNormThreads) acc += partial[i];
    acc = wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        const double norm = sqrt(fold_waves(red));
        const double coef = max_norm / (norm + 1e-6);
        *norm_out = norm;
        *scale_out = float(coef < 1.0 ? coef : 1.0);        // a NaN norm leaves the gradients unscaled: they carry the NaN themselves
    }
}

static int64_t norm_blocks(const ww_adam_tensor* tensors, int n_tensors) {
    int64_t blocks = 0;
    for (int k = 0; k < n_tensors; ++k) blocks += (tensors[k].n + 3 + kNormChunk - 1) / kNormChunk;
    return blocks;
}

int launch_grad_norm(const ww_adam_tensor* tensors, int n_tensors, double max_norm, double* norm, float* scale, void* workspace, hipStream_t stream) {
    TensorTable tab;
    if (int rc = fill_table(tensors, n_tensors, kNormChunk, &tab)) return rc;
    const int blocks = tab.first_block[kMaxTensors];
    double* partial = static_cast<double*>(workspace);
    if (int rc = launch<grad_norm_kernel>(dim3(unsigned(blocks)), dim3(kNormThreads), 0, stream, tab, partial)) return rc;
    return launch<grad_norm_finish_kernel>(dim3(1), dim3(kNormThreads), 0, stream, partial, blocks, max_norm, norm, scale);
}

// Host checks of a table, before any HIP call.  `state`: p, m and v are read and written (Adam); the norm reads g alone.
static int check_table(const ww_adam_tensor* tensors, int64_t n_tensors, bool state) {
    if (n_tensors < 1 || n_tensors > kMaxTensors) return fail(WW_EINVAL, "n_tensors %lld: expected 1..%d", (long long)n_tensors, kMaxTensors);
    if (!tensors) return fail(WW_EINVAL, "null tensors pointer");
    for (int k = 0; k < int(n_tensors); ++k) {
        const ww_adam_tensor& t = tensors[k];
        if (t.n <= 0 || t.n > (int64_t(1) << 40)) return fail(WW_EINVAL, "tensors[%d].n %lld: expected 1..2^40", k, (long long)t.n);
        if (!t.g || (state && (!t.p || !t.m || !t.v))) return fail(WW_EINVAL, "tensors[%d]: null p / g / m / v pointer", k);
        if ((reinterpret_cast<uintptr_t>(t.g) & 3) ||
            (state && ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.m) | reinterpret_cast<uintptr_t>(t.v)) & 3)))
            return fail(WW_EINVAL, "tensors[%d]: p / g / m / v must be 4-byte aligned", k);
    }
    if (!state) return WW_OK;
    // p, m and v are written: no two of the 3 n_tensors ranges may overlap (g is only read and may be shared)
    const float* lo[3 * kMaxTensors];
    int cnt = 0;
    int64_t len[3 * kMaxTensors];
    for (int k = 0; k < int(n_tensors); ++k)
        for (const float* ptr : {static_cast<const float*>(tensors[k].p), static_cast<const float*>(tensors[k].m), static_cast<const float*>(tensors[k].v)}) {
            lo[cnt] = ptr; len[cnt] = tensors[k].n; ++cnt;
        }
    for (int i = 0; i < cnt; ++i)
        for (int j = i + 1; j < cnt; ++j) {
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(lo[i]), a1 = a0 + uintptr_t(len[i]) * 4;
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(lo[j]), b1 = b0 + uintptr_t(len[j]) * 4;
            if (a0 < b1 && b0 < a1) return fail(WW_EINVAL, "tensors[%d] and tensors[%d]: p / m / v ranges overlap", i / 3, j / 3);
        }
    return WW_OK;
}

// Host checks of an averaging call, before any HIP call.  `adam`: the table went through check_table(..., true) and its g, m and v are
// live as well as p; otherwise only p and n of an entry are read, and they are checked here.  An average is written, so its range may
// meet no other average and nothing of the table that the launch reads or writes -- the gradients included.
static int check_average(const ww_adam_tensor* tensors, float* const* avg, int64_t n_tensors, double weight, bool adam) {
    if (!adam) {
        if (n_tensors < 1 || n_tensors > kMaxTensors) return fail(WW_EINVAL, "n_tensors %lld: expected 1..%d", (long long)n_tensors, kMaxTensors);
        if (!tensors) return fail(WW_EINVAL, "null tensors pointer");
        for (int k = 0; k < int(n_tensors); ++k) {
            if (tensors[k].n <= 0 || tensors[k].n > (int64_t(1) << 40))
                return fail(WW_EINVAL, "tensors[%d].n %lld: expected 1..2^40", k, (long long)tensors[k].n);
            if (!tensors[k].p) return fail(WW_EINVAL, "tensors[%d]: null p pointer", k);
            if (reinterpret_cast<uintptr_t>(tensors[k].p) & 3) return fail(WW_EINVAL, "tensors[%d]: p must be 4-byte aligned", k);
        }
    }
    if (!(weight >= 0.0 && weight <= 1.0)) return fail(WW_EINVAL, "avg_weight %g: expected [0, 1]", weight);
    if (!avg) return fail(WW_EINVAL, "null avg_host pointer");
    for (int k = 0; k < int(n_tensors); ++k) {
        if (!avg[k]) return fail(WW_EINVAL, "avg_host[%d]: null pointer", k);
        if (reinterpret_cast<uintptr_t>(avg[k]) & 3) return fail(WW_EINVAL, "avg_host[%d] must be 4-byte aligned", k);
    }
    const auto meets = [](const void* x, const void* y, int64_t nx, int64_t ny) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(x), a1 = a0 + uintptr_t(nx) * 4;
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(y), b1 = b0 + uintptr_t(ny) * 4;
        return a0 < b1 && b0 < a1;
    };
    for (int i = 0; i < int(n_tensors); ++i)
        for (int j = 0; j < int(n_tensors); ++j) {
            const ww_adam_tensor& t = tensors[j];
            if (j > i && meets(avg[i], avg[j], tensors[i].n, t.n)) return fail(WW_EINVAL, "avg_host[%d] and avg_host[%d]: ranges overlap", i, j);
            if (meets(avg[i], t.p, tensors[i].n, t.n) ||
                (adam && (meets(avg[i], t.g, tensors[i].n, t.n) || meets(avg[i], t.m, tensors[i].n, t.n) || meets(avg[i], t.v, tensors[i].n, t.n))))
                return fail(WW_EINVAL, "avg_host[%d] and tensors[%d]: the average's range overlaps %s", i, j, adam ? "p / g / m / v" : "p");
        }
    return WW_OK;
}

// Host checks of an Adam call's scalars and table, before any HIP call, and the kernel's float32 scalars: the bias corrections in
// double, as torch computes them, then one rounding.
static int adam_prepare(const ww_adam_tensor* tensors_host, int64_t n_tensors, double lr, double beta1, double beta2, double eps, double weight_decay,
                        int64_t step, const float* grad_scale_dev, AdamScalars* s) {
    if (!(lr >= 0.0) || std::isinf(lr)) return fail(WW_EINVAL, "lr %g: expected a finite value >= 0", lr);
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(WW_EINVAL, "beta1 %g: expected [0, 1)", beta1);
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(WW_EINVAL, "beta2 %g: expected [0, 1)", beta2);
    if (!(eps > 0.0) || std::isinf(eps)) return fail(WW_EINVAL, "eps %g: expected a finite value > 0", eps);
    if (!(weight_decay >= 0.0) || std::isinf(weight_decay)) return fail(WW_EINVAL, "weight_decay %g: expected a finite value >= 0", weight_decay);
    if (step < 1) return fail(WW_EINVAL, "step %lld: expected >= 1", (long long)step);
    if (int rc = check_table(tensors_host, n_tensors, true)) return rc;
    if (reinterpret_cast<uintptr_t>(grad_scale_dev) & 3) return fail(WW_EINVAL, "grad_scale_dev must be 4-byte aligned");
    const double c1 = 1.0 - std::pow(beta1, double(step)), c2 = 1.0 - std::pow(beta2, double(step));
    s->lr_c1 = float(lr / c1);
    s->inv_c2_sqrt = float(1.0 / std::sqrt(c2));
    s->eps = float(eps);
    s->omb1 = float(1.0 - beta1);
    s->beta2 = float(beta2);
    s->omb2 = float(1.0 - beta2);
    s->weight_decay = float(weight_decay);
    return WW_OK;
}

// Host checks of the loss options, before any HIP call: what ww_ce_loss_ex_f32, ww_ce_loss_soft_f32 and ww_hard_select_f32 share.
int check_loss_opts(const ww_loss_opts& o) {
    for (int c = 0; c < 2; ++c)
        if (!(o.class_weight[c] >= 0.0) || std::isinf(o.class_weight[c]))
            return fail(WW_EINVAL, "class_weight[%d] %g: expected a finite value >= 0", c, o.class_weight[c]);
    if (!(o.label_smoothing >= 0.0 && o.label_smoothing <= 1.0)) return fail(WW_EINVAL, "label_smoothing %g: expected [0, 1]", o.label_smoothing);
    if (!(o.focal_gamma >= 0.0) || std::isinf(o.focal_gamma)) return fail(WW_EINVAL, "focal_gamma %g: expected a finite value >= 0", o.focal_gamma);
    if (o.kind != WW_LOSS_CE && o.kind != WW_LOSS_FOCAL) return fail(WW_EINVAL, "kind %d: expected WW_LOSS_CE or WW_LOSS_FOCAL", int(o.kind));
    if (o.reduction != WW_REDUCE_MEAN && o.reduction != WW_REDUCE_SUM)
        return fail(WW_EINVAL, "reduction %d: expected WW_REDUCE_MEAN or WW_REDUCE_SUM", int(o.reduction));
    if (o.kind == WW_LOSS_FOCAL && o.label_smoothing != 0.0)
        return fail(WW_EINVAL, "label_smoothing %g: the focal loss takes none", o.label_smoothing);
    return WW_OK;
}

// Host checks of a loss call, before any HIP call, in the one order the three entries keep: n; under `probs` (float32 targets [n][2],
// a NULL opts_host leaves *o at the defaults it came with) the options; the NULL pointers -- with integer labels and options (`o`
// given) opts_host among them; the 4-byte and 8-byte alignments; the options of integer labels; the device.  `o` receives the options.
static int check_loss_call(const void* logits, const void* targets, bool probs, int64_t n, const ww_loss_opts* opts_host, ww_loss_opts* o,
                           const void* dlogits, const void* loss, const void* stats) {
    const auto off = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (n <= 0 || n > (int64_t(1) << 30)) return fail(WW_EINVAL, "n %lld: expected 1..2^30", (long long)n);
    if (probs) {
        if (opts_host) *o = *opts_host;
        if (int rc = check_loss_opts(*o)) return rc;
        if (o->kind != WW_LOSS_CE) return fail(WW_EINVAL, "kind %d: class-probability targets take WW_LOSS_CE only", int(o->kind));
        if (o->ignore_index != -100)
            return fail(WW_EINVAL, "ignore_index %lld: class-probability targets take none (leave it at -100)", (long long)o->ignore_index);
    }
    if (!logits || !targets) return fail(WW_EINVAL, "null logits / %s pointer", probs ? "targets" : "labels");
    if (o && !probs && !opts_host) return fail(WW_EINVAL, "null opts_host pointer");
    if (off(logits, 3) || (probs && off(targets, 3)) || off(dlogits, 3) || off(loss, 3))
        return fail(WW_EINVAL, "logits_dev / %sdlogits_dev / loss_dev must be 4-byte aligned", probs ? "targets_dev / " : "");
    if ((!probs && off(targets, 7)) || off(stats, 7)) return fail(WW_EINVAL, "%sstats_dev must be 8-byte aligned", probs ? "" : "labels_dev / ");
    if (o && !probs) {
        *o = *opts_host;
        if (int rc = check_loss_opts(*o)) return rc;
    }
    return require_gfx950();
}

}  // namespace ww

using namespace ww;

extern "C" {

int ww_ce_loss_f32(const float* logits_dev, const int64_t* labels_dev, int64_t n, float* dlogits_dev, float* loss_dev, ww_loss_stats* stats_dev,
                   ww_stream_t stream) {
    if (int rc = check_loss_call(logits_dev, labels_dev, false, n, nullptr, nullptr, dlogits_dev, loss_dev, stats_dev)) return rc;
    return launch_ce_loss(logits_dev, labels_dev, n, dlogits_dev, loss_dev, stats_dev, static_cast<hipStream_t>(stream));
}

int ww_ce_loss_ex_f32(const float* logits_dev, const int64_t* labels_dev, int64_t n, const ww_loss_opts* opts_host, float* dlogits_dev,
                      float* loss_dev, ww_loss_stats* stats_dev, ww_stream_t stream) {
    ww_loss_opts o;
    if (int rc = check_loss_call(logits_dev, labels_dev, false, n, opts_host, &o, dlogits_dev, loss_dev, stats_dev)) return rc;
    return launch_ce_loss_ex(logits_dev, labels_dev, n, o, dlogits_dev, loss_dev, stats_dev, static_cast<hipStream_t>(stream));
}

int ww_ce_loss_soft_f32(const float* logits_dev, const float* targets_dev, int64_t n, const ww_loss_opts* opts_host, float* dlogits_dev,
                        float* loss_dev, ww_loss_stats* stats_dev, ww_stream_t stream) {
    ww_loss_opts o = {{1.0, 1.0}, 0.0, 0.0, -100, WW_LOSS_CE, WW_REDUCE_MEAN};             // NULL: nn.CrossEntropyLoss()'s defaults
    if (int rc = check_loss_call(logits_dev, targets_dev, true, n, opts_host, &o, dlogits_dev, loss_dev, stats_dev)) return rc;
    return launch_ce_loss_soft(logits_dev, targets_dev, n, o, dlogits_dev, loss_dev, stats_dev, static_cast<hipStream_t>(stream));
}

int ww_distill_loss_f32(const float* logits_dev, const float* teacher_logits_dev, const void* targets_dev, int target_kind, int64_t n,
                        const ww_loss_opts* opts_host, double alpha, double temperature, float* dlogits_dev, float* loss_dev,
                        ww_loss_stats* stats_dev, ww_distill_stats* distill_stats_dev, ww_stream_t stream) {
    const auto off = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    ww_loss_opts o = {{1.0, 1.0}, 0.0, 0.0, -100, WW_LOSS_CE, WW_REDUCE_MEAN};             // NULL: nn.CrossEntropyLoss()'s defaults
    const ww_loss_opts defaults = o;
    const bool probs = target_kind == WW_TARGET_PROBS;
    // the distillation's own arguments first: check_loss_call ends with the device query
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(WW_EINVAL, "alpha %g: expected [0, 1]", alpha);
    if (!(temperature > 0.0) || std::isinf(temperature)) return fail(WW_EINVAL, "temperature %g: expected a finite value > 0", temperature);
    if (!teacher_logits_dev) return fail(WW_EINVAL, "null teacher_logits pointer");
    if (off(teacher_logits_dev, 3)) return fail(WW_EINVAL, "teacher_logits_dev must be 4-byte aligned");
    if (off(distill_stats_dev, 7)) return fail(WW_EINVAL, "distill_stats_dev must be 8-byte aligned");
    if (targets_dev) {
        if (target_kind != WW_TARGET_LABELS && !probs) return fail(WW_EINVAL, "target_kind %d: expected WW_TARGET_LABELS or WW_TARGET_PROBS", target_kind);
        if (int rc = check_loss_call(logits_dev, targets_dev, probs, n, probs || opts_host ? opts_host : &defaults, &o, dlogits_dev, loss_dev, stats_dev))
            return rc;
    } else {                                                // no target: of the options only the reduction is read
        if (n <= 0 || n > (int64_t(1) << 30)) return fail(WW_EINVAL, "n %lld: expected 1..2^30", (long long)n);
        if (opts_host) o = *opts_host;
        if (int rc = check_loss_opts(o)) return rc;
        if (!logits_dev) return fail(WW_EINVAL, "null logits pointer");
        if (off(logits_dev, 3) || off(dlogits_dev, 3) || off(loss_dev, 3)) return fail(WW_EINVAL, "logits_dev / dlogits_dev / loss_dev must be 4-byte aligned");
        if (off(stats_dev, 7)) return fail(WW_EINVAL, "stats_dev must be 8-byte aligned");
        if (int rc = require_gfx950()) return rc;
    }
    const DistillArgs da = {alpha, temperature, o.reduction};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!targets_dev) return launch_distill(logits_dev, teacher_logits_dev, nullptr, n, NoTarget{}, da, dlogits_dev, loss_dev, stats_dev, distill_stats_dev, s);
    if (probs) return launch_distill(logits_dev, teacher_logits_dev, targets_dev, n, Probs{o}, da, dlogits_dev, loss_dev, stats_dev, distill_stats_dev, s);
    return launch_distill(logits_dev, teacher_logits_dev, targets_dev, n, OptLabels{o}, da, dlogits_dev, loss_dev, stats_dev, distill_stats_dev, s);
}

int ww_adam_step_f32(const ww_adam_tensor* tensors_host, int64_t n_tensors, double lr, double beta1, double beta2, double eps, double weight_decay,
                     int64_t step, const float* grad_scale_dev, ww_stream_t stream) {
    AdamScalars s;
    if (int rc = adam_prepare(tensors_host, n_tensors, lr, beta1, beta2, eps, weight_decay, step, grad_scale_dev, &s)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_adam(tensors_host, int(n_tensors), s, grad_scale_dev, static_cast<hipStream_t>(stream));
}

int ww_adam_avg_step_f32(const ww_adam_tensor* tensors_host, float* const* avg_host, int64_t n_tensors, double lr, double beta1, double beta2,
                         double eps, double weight_decay, int64_t step, const float* grad_scale_dev, double avg_weight, ww_stream_t stream) {
    AdamScalars s;
    if (int rc = adam_prepare(tensors_host, n_tensors, lr, beta1, beta2, eps, weight_decay, step, grad_scale_dev, &s)) return rc;
    if (int rc = check_average(tensors_host, avg_host, n_tensors, avg_weight, true)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_adam_avg(tensors_host, avg_host, int(n_tensors), s, grad_scale_dev, avg_weight, static_cast<hipStream_t>(stream));
}

int ww_weight_average_f32(const ww_adam_tensor* tensors_host, float* const* avg_host, int64_t n_tensors, double avg_weight, ww_stream_t stream) {
    if (int rc = check_average(tensors_host, avg_host, n_tensors, avg_weight, false)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_weight_average(tensors_host, avg_host, int(n_tensors), avg_weight, static_cast<hipStream_t>(stream));
}

int64_t ww_grad_norm_workspace_bytes(const ww_adam_tensor* tensors_host, int64_t n_tensors) {
    if (int rc = check_table(tensors_host, n_tensors, false)) return rc;
    return up256(norm_blocks(tensors_host, int(n_tensors)) * int64_t(sizeof(double)));
}

int ww_grad_norm_f32(const ww_adam_tensor* tensors_host, int64_t n_tensors, double max_norm, double* norm_dev, float* scale_dev, void* workspace_dev,
                     ww_stream_t stream) {
    if (!(max_norm > 0.0)) return fail(WW_EINVAL, "max_norm %g: expected > 0 (infinity: measure without clipping)", max_norm);
    if (int rc = check_table(tensors_host, n_tensors, false)) return rc;
    if (!norm_dev || !scale_dev || !workspace_dev) return fail(WW_EINVAL, "null norm / scale / workspace pointer");
    if ((reinterpret_cast<uintptr_t>(norm_dev) & 7) || (reinterpret_cast<uintptr_t>(scale_dev) & 3) || (reinterpret_cast<uintptr_t>(workspace_dev) & 255))
        return fail(WW_EINVAL, "norm_dev must be 8-byte, scale_dev 4-byte and workspace_dev 256-byte aligned");
    if (int rc = require_gfx950()) return rc;
    return launch_grad_norm(tensors_host, int(n_tensors), max_norm, norm_dev, scale_dev, workspace_dev, static_cast<hipStream_t>(stream));
}

}  // extern "C"
