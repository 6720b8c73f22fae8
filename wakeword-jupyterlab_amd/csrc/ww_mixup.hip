// Mixup on log-mel batches: row i of the batch becomes lam_i * row i + (1 - lam_i) * row partner_i, and the
// row's target becomes the same mix of the two one-hot labels -- class probabilities, what ww_ce_loss_soft_f32 takes.
//   mixup_kernel   grid (chunks of a row, rows): a workgroup owns 256 float4 of one row; the first lane of a row's first chunk writes
//                  the row's target
// mel [B][80][T] float32, T = 1 .. 63: a row is 320 T bytes = 20 T float4, so a 16-byte-aligned base gives 16-byte-aligned rows; a view
// 4 bytes off the grid takes the same element mapping one float at a time.  Out of place.  Memory-bound: per row 320 T bytes read and
// written, plus 320 T bytes of the partner row when the row is mixed.  lambda, partner and labels of a row are uniform over a workgroup.
#include <cmath>

#include "ww_internal.h"

namespace ww {

constexpr int kMixThreads = 256;
constexpr int kMixChunk = kMixThreads * 4;              // floats of a row per workgroup: one 16-byte vector per thread
constexpr int kMixMaxGridRows = 65535;                  // grid.y; a larger batch strides over it

// out = fmaf(lam, a, (1 - lam) * b) with `oml` = 1 - lam, one float32 subtraction made by the caller: the product is rounded once, then
// one fused multiply-add -- written with the rounding intrinsics so that no contraction can move a rounding.
__device__ __forceinline__ float mix_one(float lam, float oml, float a, float b) { return fmaf(lam, a, __fmul_rn(oml, b)); }

// The kernel clamps nothing and trusts no device value for an address: a partner outside [0, B) leaves the row unmixed (its target NaN),
// and labels[partner] / mel[partner] are formed only from an index that passed that test against the B ARGUMENT.
template <bool kWide>
__global__ __launch_bounds__(kMixThreads) void mixup_kernel(const float* __restrict__ mel, float* __restrict__ out, int64_t B, int row_floats,
                                                            const int64_t* __restrict__ labels, const int32_t* __restrict__ partner,
                                                            const float* __restrict__ lambda, float* __restrict__ targets) {
    const int e0 = 4 * (int(blockIdx.x) * kMixThreads + int(threadIdx.x));       // row_floats is a multiple of 4: a vector lies inside or outside
    for (int64_t i = blockIdx.y; i < B; i += gridDim.y) {
        const float lam = lambda[i];
        const int64_t p = int64_t(partner[i]);
        const bool in_range = p >= 0 && p < B;
        const bool mixed = lam != 1.0f && in_range;
        const float oml = __fsub_rn(1.0f, lam);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const int64_t yi = labels[i];
            bool ok = in_range && (yi == 0 || yi == 1);
            int64_t yp = yi;
            if (ok && mixed) {
                yp = labels[p];
                ok = yp == 0 || yp == 1;
            }
            float t0 = __builtin_nanf(""), t1 = __builtin_nanf("");                // the loss counts such a row as a bad label
            if (ok && (!mixed || yp == yi)) {
                t0 = yi == 0 ? 1.0f : 0.0f; t1 = yi == 1 ? 1.0f : 0.0f;             // the exact one-hot
            } else if (ok) {
                t0 = yi == 0 ? lam : oml; t1 = yi == 1 ? lam : oml;
            }
            targets[2 * i] = t0; targets[2 * i + 1] = t1;
        }
        if (e0 >= row_floats) continue;
        const float* __restrict__ a = mel + i * int64_t(row_floats) + e0;
        float* __restrict__ o = out + i * int64_t(row_floats) + e0;
        if (!mixed) {                                                                // a bit-exact copy; the partner row is not read
            if (kWide) {
                *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(a);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = a[j];
            }
            continue;
        }
        const float* __restrict__ b = mel + p * int64_t(row_floats) + e0;
        if (kWide) {
            const float4 x = *reinterpret_cast<const float4*>(a), y = *reinterpret_cast<const float4*>(b);
            *reinterpret_cast<float4*>(o) = make_float4(mix_one(lam, oml, x.x, y.x), mix_one(lam, oml, x.y, y.y), mix_one(lam, oml, x.z, y.z),
                                                        mix_one(lam, oml, x.w, y.w));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = mix_one(lam, oml, a[j], b[j]);
        }
    }
}

int launch_mixup(const float* mel, float* out, int64_t B, int T, const int64_t* labels, const int32_t* partner, const float* lambda,
                 float* targets, hipStream_t stream) {
    const int row_floats = kMels * T;
    const dim3 grid(unsigned((row_floats + kMixChunk - 1) / kMixChunk), unsigned(B < kMixMaxGridRows ? B : kMixMaxGridRows)), block(kMixThreads);
    const bool wide = ((reinterpret_cast<uintptr_t>(mel) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    if (wide)
        return launch<mixup_kernel<true>>(grid, block, 0, stream, mel, out, B, row_floats, labels, partner, lambda, targets);
    return launch<mixup_kernel<false>>(grid, block, 0, stream, mel, out, B, row_floats, labels, partner, lambda, targets);
}

}  // namespace ww

using namespace ww;

extern "C" {

int ww_mixup_f32(const float* mel_dev, float* out_dev, int64_t B, int32_t T, const int64_t* labels_dev, const int32_t* partner_dev,
                 const float* lambda_dev, float* targets_dev, ww_stream_t stream) {
    if (B < 1 || B > (int64_t(1) << 30)) return fail(WW_EINVAL, "B %lld: expected 1..2^30", (long long)B);
    if (T < 1 || T > WW_MAX_FRAMES) return fail(WW_EINVAL, "T %d: mel images of 1..%d frames", int(T), WW_MAX_FRAMES);
    if (!mel_dev || !out_dev) return fail(WW_EINVAL, "null mel / out pointer");
    if (!labels_dev || !partner_dev || !lambda_dev || !targets_dev) return fail(WW_EINVAL, "null labels / partner / lambda / targets pointer");
    const uintptr_t a = reinterpret_cast<uintptr_t>(mel_dev), b = reinterpret_cast<uintptr_t>(out_dev);
    if ((a & 3) || (b & 3) || (reinterpret_cast<uintptr_t>(partner_dev) & 3) || (reinterpret_cast<uintptr_t>(lambda_dev) & 3) ||
        (reinterpret_cast<uintptr_t>(targets_dev) & 3))
        return fail(WW_EINVAL, "mel_dev / out_dev / partner_dev / lambda_dev / targets_dev must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(labels_dev) & 7) return fail(WW_EINVAL, "labels_dev must be 8-byte aligned");
    const uintptr_t bytes = uintptr_t(B) * WW_N_MELS * uintptr_t(T) * sizeof(float);
    if (a < b + bytes && b < a + bytes) return fail(WW_EINVAL, "mel_dev and out_dev overlap: the kernel works out of place");
    if (int rc = require_gfx950()) return rc;
    return launch_mixup(mel_dev, out_dev, B, T, labels_dev, partner_dev, lambda_dev, targets_dev, static_cast<hipStream_t>(stream));
}

}  // extern "C"
