// The per-clip rules of the two-class cross-entropy (INTEGRATION.md sections 3h, 3k, 3n), shared by the loss kernels (ww_optim.hip) and
// by the loss-ranked selection (ww_select.hip): one clip's loss and gradient in float64, NOT yet divided by the mean's denominator.
// A policy supplies the target type, the per-clip formula and the mean's denominator; the kernels own the walk over the clips.
#pragma once
#include <cmath>

#include "ww_internal.h"

namespace ww {

// One clip in float64, NOT yet divided by the mean's denominator.
struct LossClip { double loss, d0, d1; int correct, bad, nonfinite; };

// The softmax and the log-sum-exp of one clip in float64, lse = max + log(exp(z0 - max) + exp(z1 - max)): what the three rules share.
struct Softmax2 { double z0, z1, lse, p0, p1; };

__device__ __forceinline__ Softmax2 softmax2(double z0, double z1) {
    Softmax2 r;
    r.z0 = z0; r.z1 = z1;
    const double m = r.z0 > r.z1 ? r.z0 : r.z1;
    const double e0 = exp(r.z0 - m), e1 = exp(r.z1 - m), s = e0 + e1;
    r.lse = m + log(s);
    r.p0 = e0 / s; r.p1 = e1 / s;
    return r;
}

// What a clip adds to the stats record whatever the rule: a tie in the logits predicts class 0, as torch.max(output, 1) does.
__device__ __forceinline__ void clip_counts(LossClip& r, float z0f, float z1f, bool valid, bool ignored, int target_class) {
    r.correct = valid && (z1f > z0f ? 1 : 0) == target_class;
    r.bad = !ignored && !valid;
    r.nonfinite = !(isfinite(z0f) && isfinite(z1f));
}

// Integer labels, the mean over n: loss = lse - z[y], d = softmax - onehot.  A label outside {0, 1} is a bad label (-100 included).
struct PlainLabels {
    using Target = int64_t;
    static constexpr int kPer = 1, kCounts = 0;             // no counting pass: the denominator is n, and a batch is never empty
    __device__ __forceinline__ LossClip clip(float z0f, float z1f, const int64_t* t) const {
        LossClip r;
        const int64_t y = *t;
        const Softmax2 sm = softmax2(z0f, z1f);
        const bool valid = y == 0 || y == 1;
        r.loss = valid ? sm.lse - (y == 1 ? sm.z1 : sm.z0) : 0.0;
        r.d0 = valid ? sm.p0 - (y == 0 ? 1.0 : 0.0) : 0.0;
        r.d1 = valid ? sm.p1 - (y == 1 ? 1.0 : 0.0) : 0.0;
        clip_counts(r, z0f, z1f, valid, false, int(y));
        return r;
    }
};

// Integer labels with class weights, label smoothing and ignore_index, and the focal loss.  A clip counts
// (`valid`) with a label in {0, 1} that is not ignore_index (the ignore test comes first, so ignore_index may be 0 or 1).  The weighted
// mean divides every gradient by W = n0 w0 + n1 w1 (the focal mean by n0 + n1): two integer counts give it exactly before the first
// gradient is written.  With unit weights, no smoothing and the cross-entropy kind loss and gradient have PlainLabels' bits.
struct OptLabels {
    using Target = int64_t;
    static constexpr int kPer = 1, kCounts = 2;
    ww_loss_opts o;
    __device__ __forceinline__ bool counts_first() const { return o.reduction == WW_REDUCE_MEAN; }
    __device__ __forceinline__ void tally(const int64_t* t, int* c) const {
        const bool counted = *t != o.ignore_index;
        c[0] += counted && *t == 0;
        c[1] += counted && *t == 1;
    }
    __device__ __forceinline__ double denominator(const int64_t* totals) const {
        return o.kind == WW_LOSS_FOCAL ? double(totals[0] + totals[1]) : double(totals[0]) * o.class_weight[0] + double(totals[1]) * o.class_weight[1];
    }
    __device__ __forceinline__ LossClip clip(float z0f, float z1f, const int64_t* t) const {
        LossClip r;
        const int64_t y = *t;
        const Softmax2 sm = softmax2(z0f, z1f);
        const double z0 = sm.z0, z1 = sm.z1, lse = sm.lse, p0 = sm.p0, p1 = sm.p1;
        const bool ignored = y == o.ignore_index;
        const bool valid = !ignored && (y == 0 || y == 1);
        const double w0 = o.class_weight[0], w1 = o.class_weight[1];
        const double wy = y == 1 ? w1 : w0;
        const double nly = lse - (y == 1 ? z1 : z0);            // -log p_y
        double loss, d0, d1;
        if (o.kind == WW_LOSS_FOCAL) {
            const double py = y == 1 ? p1 : p0, q = y == 1 ? p0 : p1;      // q = the OTHER class's softmax term, never 1 - p_y
            const double qg = exp(-o.focal_gamma * (lse - (y == 1 ? z0 : z1)));    // q^gamma from log q = z_other - lse: one exp, and 1 at gamma = 0
            loss = wy * qg * nly;
            const double dy = wy * (-o.focal_gamma * py * qg * nly - qg * q);
            d0 = y == 0 ? dy : -dy;
            d1 = y == 1 ? dy : -dy;
        } else {
            const double eps = o.label_smoothing, keep = (1.0 - eps) * wy, half = 0.5 * eps;
            loss = keep * nly + half * (w0 * (lse - z0) + w1 * (lse - z1));
            d0 = keep * (p0 - (y == 0 ? 1.0 : 0.0)) + half * ((w0 + w1) * p0 - w0);
            d1 = keep * (p1 - (y == 1 ? 1.0 : 0.0)) + half * ((w0 + w1) * p1 - w1);
        }
        r.loss = valid ? loss : 0.0;
        r.d0 = valid ? d0 : 0.0;
        r.d1 = valid ? d1 : 0.0;
        clip_counts(r, z0f, z1f, valid, ignored, int(y));
        return r;
    }
};

// Class probabilities [n][2] float32: mixup, soft relabelling, a teacher's softmax (distillation proper, with
// a temperature and a hard term beside the teacher's, is distill_loss_kernel in ww_optim.hip).  t' = (1 - eps) t + eps / 2;
// l = sum_c w_c t'_c (lse - z_c); dl/dz_k = p_k (w0 t'_0 + w1 t'_1) - w_k t'_k.  A row counts iff both targets are finite and >= 0, and
// the mean's denominator is the NUMBER of such rows (torch divides by n), not the weighted sum of the integer-label form.  With a
// one-hot row, unit weights and eps = 0 every product is by 1 or by 0, so loss and gradient have the bits of the label rules.
struct Probs {
    using Target = float;
    static constexpr int kPer = 2, kCounts = 1;
    ww_loss_opts o;
    static __device__ __forceinline__ bool counted(const float* t) { return isfinite(t[0]) && isfinite(t[1]) && t[0] >= 0.f && t[1] >= 0.f; }
    __device__ __forceinline__ bool counts_first() const { return o.reduction == WW_REDUCE_MEAN; }
    __device__ __forceinline__ void tally(const float* t, int* c) const { c[0] += counted(t); }
    __device__ __forceinline__ double denominator(const int64_t* totals) const { return double(totals[0]); }
    __device__ __forceinline__ LossClip clip(float z0f, float z1f, const float* t) const {
        LossClip r;
        const Softmax2 sm = softmax2(z0f, z1f);
        const float t0f = t[0], t1f = t[1];
        const bool valid = counted(t);
        const double eps = o.label_smoothing, half = 0.5 * eps;
        const double a0 = o.class_weight[0] * ((1.0 - eps) * double(t0f) + half);
        const double a1 = o.class_weight[1] * ((1.0 - eps) * double(t1f) + half);
        const double loss = a0 * (sm.lse - sm.z0) + a1 * (sm.lse - sm.z1);
        const double wsum = a0 + a1;
        const double d0 = sm.p0 * wsum - a0, d1 = sm.p1 * wsum - a1;
        r.loss = valid ? loss : 0.0;
        r.d0 = valid ? d0 : 0.0;
        r.d1 = valid ? d1 : 0.0;
        clip_counts(r, z0f, z1f, valid, false, t1f > t0f ? 1 : 0);      // a tie in the target gives class 0: the prediction's rule
        return r;
    }
};

// Host checks of the loss options, before any HIP call (ww_optim.hip): what every entry point that takes a ww_loss_opts shares.
int check_loss_opts(const ww_loss_opts& o);

}  // namespace ww
