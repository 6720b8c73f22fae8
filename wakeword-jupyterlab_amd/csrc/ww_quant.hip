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
// Memory- and latency-bound; the models' weights are 0.6 M and 1.0 M floats.  Not on a per-step path.
#include "ww_internal.h"

namespace ww {
namespace {

constexpr int kQuantThreads = 1024;
constexpr int kQuantWaves = kQuantThreads / 64;
constexpr int kQuantWaveCols = 1024;                         // the longest row a wave takes
constexpr int kQuantPerLane = kQuantWaveCols / 64;
constexpr int kQuantMax = WW_QUANT_MAX_TENSORS;

struct QuantTable {
    ww_quant_tensor t[kQuantMax];
    int32_t first_block[kQuantMax + 1];                     // prefix sums of the tensors' block counts
    int32_t n_tensors;
    float qmax;                                             // 2^(bits - 1) - 1
};

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

// What one lane gathers over its elements: the float64 sums of w^2 and (w - deq)^2, the largest |w - deq|, the non-finite count.
struct QuantAcc {
    double sw = 0.0, se = 0.0, emax = 0.0;
    int bad = 0;
};

// One element.  A non-finite w quantises to 0, is counted, and enters no sum.
__device__ __forceinline__ void quant_one(float w, float scale, float qmax, int& q, float& deq, QuantAcc& acc) {
    const bool fin = isfinite(w);
    float r = rintf(__fdiv_rn(fin ? w : 0.0f, scale));     // ties to even
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

__device__ __forceinline__ int tensor_of(const QuantTable& tab, int block) {
    int k = 0;
    for (int j = 1; j < tab.n_tensors; ++j) k = tab.first_block[j] <= block ? j : k;
    return k;
}

__global__ __launch_bounds__(kQuantThreads) void quant_kernel(const QuantTable tab) {
    __shared__ float red_amax[kQuantWaves];
    __shared__ double red_d[3][kQuantWaves];
    __shared__ int red_bad[kQuantWaves];
    const int k = tensor_of(tab, int(blockIdx.x));
    const ww_quant_tensor t = tab.t[k];
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
        const float scale = scale_of(amax, qmax);
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
    const float scale = scale_of(amax, qmax);
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
    __syncthreads();
    if (tid == 0) {
        double a = red_d[0][0], b = red_d[1][0], c = red_d[2][0];
        int nb = red_bad[0];
        for (int j = 1; j < kQuantWaves; ++j) { a += red_d[0][j]; b += red_d[1][j]; c = fmax(c, red_d[2][j]); nb += red_bad[j]; }   // wave order
        t.scale[row] = scale;
        if (t.err) { t.err[3 * row] = a; t.err[3 * row + 1] = b; t.err[3 * row + 2] = c; }
        if (t.bad) t.bad[row] = nb;
    }
}

// Host checks, before any HIP call.
int check_quant(const ww_quant_tensor* tensors, int64_t n_tensors, int bits) {
    const auto off = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (n_tensors < 1 || n_tensors > kQuantMax) return fail(WW_EINVAL, "n_tensors %lld: expected 1..%d", (long long)n_tensors, kQuantMax);
    if (bits < 2 || bits > 8) return fail(WW_EINVAL, "bits %d: expected 2..8", bits);
    if (!tensors) return fail(WW_EINVAL, "null tensors pointer");
    for (int k = 0; k < int(n_tensors); ++k) {
        const ww_quant_tensor& t = tensors[k];
        if (t.rows < 1 || t.rows > (int64_t(1) << 30)) return fail(WW_EINVAL, "tensors[%d].rows %lld: expected 1..2^30", k, (long long)t.rows);
        if (t.cols < 1 || t.cols > (int64_t(1) << 30)) return fail(WW_EINVAL, "tensors[%d].cols %lld: expected 1..2^30", k, (long long)t.cols);
        if (t.rows * t.cols > (int64_t(1) << 40)) return fail(WW_EINVAL, "tensors[%d]: rows x cols %lld: expected at most 2^40", k, (long long)(t.rows * t.cols));
        if (!t.w || !t.scale) return fail(WW_EINVAL, "tensors[%d]: null w / scale pointer", k);
        if (off(t.w, 3) || off(t.scale, 3) || off(t.deq, 3) || off(t.bad, 3)) return fail(WW_EINVAL, "tensors[%d]: w / scale / deq / bad must be 4-byte aligned", k);
        if (off(t.err, 7)) return fail(WW_EINVAL, "tensors[%d]: err must be 8-byte aligned", k);
        if (t.deq) {                                        // out of place: a row is read twice
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(t.w), b0 = reinterpret_cast<uintptr_t>(t.deq), len = uintptr_t(t.rows * t.cols) * 4;
            if (a0 < b0 + len && b0 < a0 + len) return fail(WW_EINVAL, "tensors[%d]: the w and deq ranges overlap", k);
        }
    }
    return WW_OK;
}

int launch_quant(const ww_quant_tensor* tensors, int n_tensors, int bits, hipStream_t stream) {
    QuantTable tab;
    int64_t blocks = 0;
    for (int k = 0; k < n_tensors; ++k) {
        tab.t[k] = tensors[k];
        tab.first_block[k] = int32_t(blocks);
        blocks += tensors[k].cols <= kQuantWaveCols ? (tensors[k].rows + kQuantWaves - 1) / kQuantWaves : tensors[k].rows;
        if (blocks > (int64_t(1) << 30)) return fail(WW_EUNSUPPORTED, "tensors[%d]: the table needs more than 2^30 blocks", k);
    }
    for (int k = n_tensors; k <= kQuantMax; ++k) tab.first_block[k] = int32_t(blocks);
    for (int k = n_tensors; k < kQuantMax; ++k) tab.t[k] = ww_quant_tensor{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    tab.n_tensors = n_tensors;
    tab.qmax = float((1 << (bits - 1)) - 1);
    return launch<quant_kernel>(dim3(unsigned(blocks)), dim3(kQuantThreads), 0, stream, tab);
}

}  // namespace
}  // namespace ww

using namespace ww;

extern "C" {

int ww_quant_weights_f32(const ww_quant_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream) {
    if (int rc = check_quant(tensors_host, n_tensors, bits)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_quant(tensors_host, int(n_tensors), bits, static_cast<hipStream_t>(stream));
}

}  // extern "C"
