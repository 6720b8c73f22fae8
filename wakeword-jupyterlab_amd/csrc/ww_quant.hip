// Post-training weight quantisation: symmetric intN per quantisation group, N = 2..8, stored as int8.
//   quant_kernel   one launch over up to 16 tensors, the table in the kernel arguments (the shape of adam_kernel's TensorTable).  A tensor is
//                  rows x cols and a row is a group with one scale.  Two mappings, chosen per tensor by cols alone:
//                    cols <= 1024   a wave per row, 16 rows per workgroup: lane l holds the elements l, l + 64, ... of its row in registers
//                                   (one read of w), the row's amax and sums are butterflies over the wave -- a 9-element conv1 row costs a
//                                   wave, not a workgroup
//                    cols  > 1024   a workgroup per row (per-tensor mode: the whole tensor): thread t owns the 4-element vectors t, t + 1024,
//                                   ... in ELEMENT coordinates (16-byte accesses where the row starts on the 16-byte grid, single elements
//                                   otherwise: the same order, the same bits), two passes over w -- amax, then quantise -- folded through
//                                   LDS in wave order.  No row crosses workgroups, so there are no atomics and no second launch.
//                  Per element (include/wakeword_amd.h has the rule): two correctly rounded float32 operations, written with the explicit
//                  round-to-nearest intrinsics so no reciprocal and no contraction can take their place.  The error sums are float64 fmas in
//                  an order set by the mapping alone: the same input gives the same bytes.
//   quant_kernel<true>   the same kernel with one clip index per row (uint8, device memory) and a per-row count of the elements the clamp
//                  moved (ww_quant_weights_clip_f32): scale_j = max((amax * f_j) / qmax, 2^-126), f_j = (64 - j) / 64.
//                  j = 0 multiplies by 1.0f: the bits of quant_kernel<false>.  This is the launch in front of a QAT step's forward.
//   search_kernel  all WW_QUANT_CLIP_STEPS candidates of a row: the float64 sum of (w - deq_j)^2 per candidate in quant_kernel's own
//                  lane mapping and order of summation (candidate 0 IS its err[row][1]), the first argmin and its scale.  A wave keeps its
//                  row in registers and loops over the candidates; a workgroup per long row makes one pass for amax and one that carries 48
//                  float64 sums per thread (the 48 scales sit in LDS), folded through LDS in wave order.  Calibration, not a per-step path.
//   ste_kernel     the straight-through estimator with clipping: g = +0.0 where a finite w lies outside the clipped range (a store, so a
//                  NaN gradient there goes too); every other g is neither read nor written.
// Memory- and latency-bound; the models' weights are 0.6 M and 1.0 M floats.
#include "ww_internal.h"

namespace ww {
namespace {

constexpr int kQuantThreads = 1024;
constexpr int kQuantWaves = kQuantThreads / 64;
constexpr int kQuantWaveCols = 1024;                         // the longest row a wave takes
constexpr int kQuantPerLane = kQuantWaveCols / 64;
constexpr int kQuantMax = WW_QUANT_MAX_TENSORS;

constexpr int kClipSteps = WW_QUANT_CLIP_STEPS;

template <class Tensor>
struct QuantTableOf {
    Tensor t[kQuantMax];
    int32_t first_block[kQuantMax + 1];                     // prefix sums of the tensors' block counts
    int32_t n_tensors;
    float qmax;                                             // 2^(bits - 1) - 1
};
using QuantTable = QuantTableOf<ww_quant_tensor>;
using ClipTable = QuantTableOf<ww_quant_clip_tensor>;
using SteTable = QuantTableOf<ww_quant_ste_tensor>;

__device__ __forceinline__ float qwave_max(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
    return x;
}
__device__ __forceinline__ double qwave_max(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off));
    return x;
}
__device__ __forceinline__ double qwave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ int qwave_sum(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

__device__ __forceinline__ float finite_abs(float w) { return isfinite(w) ? fabsf(w) : 0.0f; }

__device__ __forceinline__ float scale_of(float amax, float qmax) { return fmaxf(__fdiv_rn(amax, qmax), 0x1p-126f); }
// Candidate j of the clipped rule: the fraction (64 - j) / 64 is exact, an index past the last candidate counts as the last.
__device__ __forceinline__ float clip_fraction(int j) { return __fmul_rn(float(64 - min(j, kClipSteps - 1)), 0x1p-6f); }
__device__ __forceinline__ float scale_of(float amax, float fraction, float qmax) { return scale_of(__fmul_rn(amax, fraction), qmax); }

// What one lane gathers over its elements: the float64 sums of w^2 and (w - deq)^2, the largest |w - deq|, the non-finite count.
struct QuantAcc {
    double sw = 0.0, se = 0.0, emax = 0.0;
    int bad = 0, sat = 0;                                   // sat: elements the clamp moved (always 0 under the unclipped scale)
};

// One element.  A non-finite w quantises to 0, is counted, and enters no sum.
__device__ __forceinline__ void quant_one(float w, float scale, float qmax, int& q, float& deq, QuantAcc& acc) {
    const bool fin = isfinite(w);
    float r = rintf(__fdiv_rn(fin ? w : 0.0f, scale));     // ties to even
    acc.sat += fabsf(r) > qmax ? 1 : 0;
    r = fminf(fmaxf(r, -qmax), qmax);
    q = int(r);
    deq = __fmul_rn(float(q), scale);
    if (fin) {
        const double dw = double(w), d = dw - double(deq);
        acc.sw = fma(dw, dw, acc.sw);
        acc.se = fma(d, d, acc.se);
        acc.emax = fmax(acc.emax, fabs(d));
    } else {
        acc.bad += 1;
    }
}

template <class Table>
__device__ __forceinline__ int tensor_of(const Table& tab, int block) {
    int k = 0;
    for (int j = 1; j < tab.n_tensors; ++j) k = tab.first_block[j] <= block ? j : k;
    return k;
}

// kClip: the table's tensors carry a clip index per row (read) and a saturation count per row (written, optional)
template <bool kClip>
__global__ __launch_bounds__(kQuantThreads) void quant_kernel(const std::conditional_t<kClip, ClipTable, QuantTable> tab) {
    __shared__ float red_amax[kQuantWaves];
    __shared__ double red_d[3][kQuantWaves];
    __shared__ int red_bad[kQuantWaves];
    __shared__ int red_sat[kQuantWaves];
    const int k = tensor_of(tab, int(blockIdx.x));
    const auto t = tab.t[k];
    const float qmax = tab.qmax;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = int64_t(int(blockIdx.x) - tab.first_block[k]);
    const int64_t cols = t.cols;

    if (cols <= kQuantWaveCols) {
        // ---- a wave per row: no LDS, no barrier (a wave past the last row leaves) ----
        const int64_t row = blk * kQuantWaves + wave;
        if (row >= t.rows) return;
        const int64_t base = row * cols;
        const int n = int(cols);
        float v[kQuantPerLane];
        float amax = 0.0f;
#pragma unroll
        for (int j = 0; j < kQuantPerLane; ++j) {
            const int c = lane + 64 * j;
            v[j] = c < n ? t.w[base + c] : 0.0f;
            amax = fmaxf(amax, finite_abs(v[j]));
        }
        amax = qwave_max(amax);
        float scale;
        if constexpr (kClip) scale = scale_of(amax, clip_fraction(t.clip[row]), qmax);
        else scale = scale_of(amax, qmax);
        QuantAcc acc;
#pragma unroll
        for (int j = 0; j < kQuantPerLane; ++j) {
            const int c = lane + 64 * j;
            if (c < n) {
                int q;
                float deq;
                quant_one(v[j], scale, qmax, q, deq, acc);
                if (t.q) t.q[base + c] = int8_t(q);
                if (t.deq) t.deq[base + c] = deq;
            }
        }
        const double sw = qwave_sum(acc.sw), se = qwave_sum(acc.se), emax = qwave_max(acc.emax);
        const int bad = qwave_sum(acc.bad);
        if (lane == 0) {
            t.scale[row] = scale;
            if (t.err) { t.err[3 * row] = sw; t.err[3 * row + 1] = se; t.err[3 * row + 2] = emax; }
            if (t.bad) t.bad[row] = bad;
        }
        if constexpr (kClip) {
            const int sat = qwave_sum(acc.sat);
            if (lane == 0 && t.sat) t.sat[row] = sat;
        }
        return;
    }

    // ---- a workgroup per row ----
    const int64_t row = blk;                                // < rows by the table's block counts
    const float* __restrict__ w = t.w + row * cols;
    int8_t* __restrict__ qo = t.q ? t.q + row * cols : nullptr;
    float* __restrict__ dq = t.deq ? t.deq + row * cols : nullptr;
    const bool w_wide = (reinterpret_cast<uintptr_t>(w) & 15) == 0;
    const bool d_wide = (reinterpret_cast<uintptr_t>(dq) & 15) == 0;
    const bool q_wide = (reinterpret_cast<uintptr_t>(qo) & 3) == 0;
    float amax = 0.0f;
#pragma unroll 4
    for (int64_t e0 = 4 * int64_t(tid); e0 < cols; e0 += 4 * kQuantThreads) {
        if (w_wide && e0 + 4 <= cols) {
            const float4 x = *reinterpret_cast<const float4*>(w + e0);
            amax = fmaxf(fmaxf(amax, finite_abs(x.x)), fmaxf(finite_abs(x.y), fmaxf(finite_abs(x.z), finite_abs(x.w))));
        } else {
            for (int i = 0; i < 4; ++i)
                if (e0 + i < cols) amax = fmaxf(amax, finite_abs(w[e0 + i]));
        }
    }
    amax = qwave_max(amax);
    if (lane == 0) red_amax[wave] = amax;
    __syncthreads();
    amax = red_amax[0];
#pragma unroll
    for (int j = 1; j < kQuantWaves; ++j) amax = fmaxf(amax, red_amax[j]);
    float scale;
    if constexpr (kClip) scale = scale_of(amax, clip_fraction(t.clip[row]), qmax);
    else scale = scale_of(amax, qmax);
    QuantAcc acc;
    for (int64_t e0 = 4 * int64_t(tid); e0 < cols; e0 += 4 * kQuantThreads) {
        const bool whole = e0 + 4 <= cols;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (w_wide && whole) {
            const float4 f = *reinterpret_cast<const float4*>(w + e0);
            x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e0 + i < cols) x[i] = w[e0 + i];
        }
        int q[4] = {0, 0, 0, 0};
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e0 + i < cols) quant_one(x[i], scale, qmax, q[i], d[i], acc);      // rising element order within the thread
        if (dq) {
            if (d_wide && whole) {
                *reinterpret_cast<float4*>(dq + e0) = make_float4(d[0], d[1], d[2], d[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (e0 + i < cols) dq[e0 + i] = d[i];
            }
        }
        if (qo) {
            if (q_wide && whole) {
                *reinterpret_cast<uint32_t*>(qo + e0) = uint32_t(q[0] & 255) | (uint32_t(q[1] & 255) << 8) | (uint32_t(q[2] & 255) << 16) |
                                                        (uint32_t(q[3] & 255) << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (e0 + i < cols) qo[e0 + i] = int8_t(q[i]);
            }
        }
    }
    const double sw = qwave_sum(acc.sw), se = qwave_sum(acc.se), emax = qwave_max(acc.emax);
    const int bad = qwave_sum(acc.bad);
    if (lane == 0) { red_d[0][wave] = sw; red_d[1][wave] = se; red_d[2][wave] = emax; red_bad[wave] = bad; }
    if constexpr (kClip) {
        const int sat = qwave_sum(acc.sat);
        if (lane == 0) red_sat[wave] = sat;
    }
    __syncthreads();
    if (tid == 0) {
        double a = red_d[0][0], b = red_d[1][0], c = red_d[2][0];
        int nb = red_bad[0];
        for (int j = 1; j < kQuantWaves; ++j) { a += red_d[0][j]; b += red_d[1][j]; c = fmax(c, red_d[2][j]); nb += red_bad[j]; }   // wave order
        t.scale[row] = scale;
        if (t.err) { t.err[3 * row] = a; t.err[3 * row + 1] = b; t.err[3 * row + 2] = c; }
        if (t.bad) t.bad[row] = nb;
        if constexpr (kClip) {
            int ns = red_sat[0];
            for (int j = 1; j < kQuantWaves; ++j) ns += red_sat[j];
            if (t.sat) t.sat[row] = ns;
        }
    }
}

// (w - deq)^2 of one element under `scale`, added to `se` as quant_one adds it to its sum: the one definition, the other sums unused.
__device__ __forceinline__ double add_sq_err(float w, float scale, float qmax, double se) {
    QuantAcc acc;
    acc.se = se;
    int q;
    float deq;
    quant_one(w, scale, qmax, q, deq, acc);
    return acc.se;
}

// The clip search: quant_kernel's two mappings, element for element and sum for sum, over all kClipSteps candidates of a row.
__global__ __launch_bounds__(kQuantThreads) void search_kernel(const ClipTable tab) {
    __shared__ float red_amax[kQuantWaves];
    __shared__ float cand_scale[kClipSteps];
    __shared__ double red_c[kClipSteps][kQuantWaves];
    const int k = tensor_of(tab, int(blockIdx.x));
    const ww_quant_clip_tensor t = tab.t[k];
    const float qmax = tab.qmax;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = int64_t(int(blockIdx.x) - tab.first_block[k]);
    const int64_t cols = t.cols;

    if (cols <= kQuantWaveCols) {
        // ---- a wave per row: the row stays in registers, the candidates are a loop ----
        const int64_t row = blk * kQuantWaves + wave;
        if (row >= t.rows) return;
        const int64_t base = row * cols;
        const int n = int(cols);
        float v[kQuantPerLane];
        float amax = 0.0f;
#pragma unroll
        for (int j = 0; j < kQuantPerLane; ++j) {
            const int c = lane + 64 * j;
            v[j] = c < n ? t.w[base + c] : 0.0f;
            amax = fmaxf(amax, finite_abs(v[j]));
        }
        amax = qwave_max(amax);
        double best = 0.0;
        float best_scale = 0.0f;
        int best_c = 0;
#pragma unroll 1
        for (int c = 0; c < kClipSteps; ++c) {
            const float scale = scale_of(amax, clip_fraction(c), qmax);
            double se = 0.0;
#pragma unroll
            for (int j = 0; j < kQuantPerLane; ++j)
                if (lane + 64 * j < n) se = add_sq_err(v[j], scale, qmax, se);
            se = qwave_sum(se);                             // the same value in every lane
            if (lane == 0 && t.cand_err) t.cand_err[row * kClipSteps + c] = se;
            if (c == 0 || se < best) { best = se; best_scale = scale; best_c = c; }     // strictly smaller: the first minimum stays
        }
        if (lane == 0) { t.clip[row] = uint8_t(best_c); t.scale[row] = best_scale; }
        return;
    }

    // ---- a workgroup per row: amax, then ONE pass with a float64 sum per candidate and thread ----
    const int64_t row = blk;
    const float* __restrict__ w = t.w + row * cols;
    const bool w_wide = (reinterpret_cast<uintptr_t>(w) & 15) == 0;
    float amax = 0.0f;
#pragma unroll 4
    for (int64_t e0 = 4 * int64_t(tid); e0 < cols; e0 += 4 * kQuantThreads) {
        if (w_wide && e0 + 4 <= cols) {
            const float4 x = *reinterpret_cast<const float4*>(w + e0);
            amax = fmaxf(fmaxf(amax, finite_abs(x.x)), fmaxf(finite_abs(x.y), fmaxf(finite_abs(x.z), finite_abs(x.w))));
        } else {
            for (int i = 0; i < 4; ++i)
                if (e0 + i < cols) amax = fmaxf(amax, finite_abs(w[e0 + i]));
        }
    }
    amax = qwave_max(amax);
    if (lane == 0) red_amax[wave] = amax;
    __syncthreads();
    amax = red_amax[0];
#pragma unroll
    for (int j = 1; j < kQuantWaves; ++j) amax = fmaxf(amax, red_amax[j]);
    if (tid < kClipSteps) cand_scale[tid] = scale_of(amax, clip_fraction(tid), qmax);
    __syncthreads();
    double se[kClipSteps];
#pragma unroll
    for (int c = 0; c < kClipSteps; ++c) se[c] = 0.0;
    for (int64_t e0 = 4 * int64_t(tid); e0 < cols; e0 += 4 * kQuantThreads) {
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (w_wide && e0 + 4 <= cols) {
            const float4 f = *reinterpret_cast<const float4*>(w + e0);
            x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e0 + i < cols) x[i] = w[e0 + i];
        }
#pragma unroll
        for (int c = 0; c < kClipSteps; ++c) {              // unrolled: se[] stays in registers
            const float scale = cand_scale[c];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e0 + i < cols) se[c] = add_sq_err(x[i], scale, qmax, se[c]);         // rising element order within the thread
            __builtin_amdgcn_sched_barrier(0);              // one candidate at a time: 48 interleaved division chains would spill
        }
    }
#pragma unroll
    for (int c = 0; c < kClipSteps; ++c) {
        const double s = qwave_sum(se[c]);
        if (lane == 0) red_c[c][wave] = s;
    }
    __syncthreads();
    if (wave == 0) {                                        // lane c folds candidate c in wave order; lanes past the last hold +inf
        double a = HUGE_VAL;
        if (lane < kClipSteps) {
            a = red_c[lane][0];
            for (int j = 1; j < kQuantWaves; ++j) a += red_c[lane][j];
            if (t.cand_err) t.cand_err[row * kClipSteps + lane] = a;
        }
        int c = lane;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {            // the smallest error; among equal ones the smallest index
            const double oa = __shfl_xor(a, off);
            const int oc = __shfl_xor(c, off);
            if (oa < a || (oa == a && oc < c)) { a = oa; c = oc; }
        }
        c = min(c, kClipSteps - 1);                         // lanes past the last candidate never win: finite sums are below +inf
        if (lane == 0) { t.clip[row] = uint8_t(c); t.scale[row] = cand_scale[c]; }
    }
}

// The clamp of the stored scale moved this element: its gradient is cut.  A non-finite w quantises to 0 and is never moved.
__device__ __forceinline__ bool clamp_moved(float w, float scale, float qmax) { return isfinite(w) && fabsf(rintf(__fdiv_rn(w, scale))) > qmax; }

__global__ __launch_bounds__(kQuantThreads) void ste_kernel(const SteTable tab) {
    const int k = tensor_of(tab, int(blockIdx.x));
    const ww_quant_ste_tensor t = tab.t[k];
    const float qmax = tab.qmax;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = int64_t(int(blockIdx.x) - tab.first_block[k]);
    const int64_t cols = t.cols;
    if (cols <= kQuantWaveCols) {
        const int64_t row = blk * kQuantWaves + wave;
        if (row >= t.rows) return;
        const int64_t base = row * cols;
        const float scale = t.scale[row];
        for (int c = lane; c < int(cols); c += 64)
            if (clamp_moved(t.w[base + c], scale, qmax)) t.g[base + c] = 0.0f;
        return;
    }
    const int64_t row = blk;
    const float* __restrict__ w = t.w + row * cols;
    float* __restrict__ g = t.g + row * cols;
    const bool w_wide = (reinterpret_cast<uintptr_t>(w) & 15) == 0;
    const float scale = t.scale[row];
    for (int64_t e0 = 4 * int64_t(tid); e0 < cols; e0 += 4 * kQuantThreads) {
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};            // a zero is never moved
        if (w_wide && e0 + 4 <= cols) {
            const float4 f = *reinterpret_cast<const float4*>(w + e0);
            x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e0 + i < cols) x[i] = w[e0 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e0 + i < cols && clamp_moved(x[i], scale, qmax)) g[e0 + i] = 0.0f;
    }
}

// Host checks, before any HIP call.
bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int check_call(const void* tensors, int64_t n_tensors, int bits) {
    if (n_tensors < 1 || n_tensors > kQuantMax) return fail(WW_EINVAL, "n_tensors %lld: expected 1..%d", (long long)n_tensors, kQuantMax);
    if (bits < 2 || bits > 8) return fail(WW_EINVAL, "bits %d: expected 2..8", bits);
    if (!tensors) return fail(WW_EINVAL, "null tensors pointer");
    return WW_OK;
}

int check_shape(int k, int64_t rows, int64_t cols) {
    if (rows < 1 || rows > (int64_t(1) << 30)) return fail(WW_EINVAL, "tensors[%d].rows %lld: expected 1..2^30", k, (long long)rows);
    if (cols < 1 || cols > (int64_t(1) << 30)) return fail(WW_EINVAL, "tensors[%d].cols %lld: expected 1..2^30", k, (long long)cols);
    if (rows * cols > (int64_t(1) << 40)) return fail(WW_EINVAL, "tensors[%d]: rows x cols %lld: expected at most 2^40", k, (long long)(rows * cols));
    return WW_OK;
}

int check_disjoint(int k, const float* w, const float* other, int64_t n, const char* name) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(w), b0 = reinterpret_cast<uintptr_t>(other), len = uintptr_t(n) * 4;
    if (a0 < b0 + len && b0 < a0 + len) return fail(WW_EINVAL, "tensors[%d]: the w and %s ranges overlap", k, name);
    return WW_OK;
}

// The fields ww_quant_tensor and ww_quant_clip_tensor share; with kClip the clip tensor's own fields after them.
template <class Tensor>
int check_quant(const Tensor* tensors, int64_t n_tensors, int bits) {
    if (int rc = check_call(tensors, n_tensors, bits)) return rc;
    for (int k = 0; k < int(n_tensors); ++k) {
        const Tensor& t = tensors[k];
        if (int rc = check_shape(k, t.rows, t.cols)) return rc;
        if (!t.w || !t.scale) return fail(WW_EINVAL, "tensors[%d]: null w / scale pointer", k);
        if (misaligned(t.w, 3) || misaligned(t.scale, 3) || misaligned(t.deq, 3) || misaligned(t.bad, 3))
            return fail(WW_EINVAL, "tensors[%d]: w / scale / deq / bad must be 4-byte aligned", k);
        if (misaligned(t.err, 7)) return fail(WW_EINVAL, "tensors[%d]: err must be 8-byte aligned", k);
        if (t.deq)                                          // out of place: a row is read twice
            if (int rc = check_disjoint(k, t.w, t.deq, t.rows * t.cols, "deq")) return rc;
        if constexpr (std::is_same_v<Tensor, ww_quant_clip_tensor>) {
            if (!t.clip) return fail(WW_EINVAL, "tensors[%d]: null clip pointer", k);
            if (misaligned(t.sat, 3)) return fail(WW_EINVAL, "tensors[%d]: sat must be 4-byte aligned", k);
            if (misaligned(t.cand_err, 7)) return fail(WW_EINVAL, "tensors[%d]: cand_err must be 8-byte aligned", k);
        }
    }
    return WW_OK;
}

int check_ste(const ww_quant_ste_tensor* tensors, int64_t n_tensors, int bits) {
    if (int rc = check_call(tensors, n_tensors, bits)) return rc;
    for (int k = 0; k < int(n_tensors); ++k) {
        const ww_quant_ste_tensor& t = tensors[k];
        if (int rc = check_shape(k, t.rows, t.cols)) return rc;
        if (!t.w || !t.scale || !t.g) return fail(WW_EINVAL, "tensors[%d]: null w / scale / g pointer", k);
        if (misaligned(t.w, 3) || misaligned(t.scale, 3) || misaligned(t.g, 3)) return fail(WW_EINVAL, "tensors[%d]: w / scale / g must be 4-byte aligned", k);
        if (int rc = check_disjoint(k, t.w, t.g, t.rows * t.cols, "g")) return rc;
    }
    return WW_OK;
}

// The table of one launch: the tensors, the prefix sums of their block counts (a block is 16 short rows or one long row) and qmax.
template <class Table, class Tensor>
int fill_table(Table& tab, const Tensor* tensors, int n_tensors, int bits, unsigned* grid) {
    int64_t blocks = 0;
    for (int k = 0; k < n_tensors; ++k) {
        tab.t[k] = tensors[k];
        tab.first_block[k] = int32_t(blocks);
        blocks += tensors[k].cols <= kQuantWaveCols ? (tensors[k].rows + kQuantWaves - 1) / kQuantWaves : tensors[k].rows;
        if (blocks > (int64_t(1) << 30)) return fail(WW_EUNSUPPORTED, "tensors[%d]: the table needs more than 2^30 blocks", k);
    }
    for (int k = n_tensors; k <= kQuantMax; ++k) tab.first_block[k] = int32_t(blocks);
    for (int k = n_tensors; k < kQuantMax; ++k) tab.t[k] = Tensor{};
    tab.n_tensors = n_tensors;
    tab.qmax = float((1 << (bits - 1)) - 1);
    *grid = unsigned(blocks);
    return WW_OK;
}

template <auto Kernel, class Table, class Tensor>
int launch_table(const Tensor* tensors, int64_t n_tensors, int bits, ww_stream_t stream) {
    Table tab;
    unsigned grid = 0;
    if (int rc = fill_table(tab, tensors, int(n_tensors), bits, &grid)) return rc;
    return launch<Kernel>(dim3(grid), dim3(kQuantThreads), 0, static_cast<hipStream_t>(stream), tab);
}

}  // namespace
}  // namespace ww

using namespace ww;

extern "C" {

int ww_quant_weights_f32(const ww_quant_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream) {
    if (int rc = check_quant(tensors_host, n_tensors, bits)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_table<quant_kernel<false>, QuantTable>(tensors_host, n_tensors, bits, stream);
}

int ww_quant_weights_clip_f32(const ww_quant_clip_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream) {
    if (int rc = check_quant(tensors_host, n_tensors, bits)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_table<quant_kernel<true>, ClipTable>(tensors_host, n_tensors, bits, stream);
}

int ww_quant_clip_search_f32(const ww_quant_clip_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream) {
    if (int rc = check_quant(tensors_host, n_tensors, bits)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_table<search_kernel, ClipTable>(tensors_host, n_tensors, bits, stream);
}

int ww_quant_ste_f32(const ww_quant_ste_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream) {
    if (int rc = check_ste(tensors_host, n_tensors, bits)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_table<ste_kernel, SteTable>(tensors_host, n_tensors, bits, stream);
}

}  // extern "C"
