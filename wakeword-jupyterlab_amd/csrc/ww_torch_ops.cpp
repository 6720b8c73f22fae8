// torch.ops.wakeword_amd.* as COMPILED operators: schema, CUDA (= HIP on ROCm) kernels over the C ABI, Meta (shape-only) kernels, and a
// CPU kernel that refuses -- SURVEY.md section 7 step 2 / section 8 boundary B1-B3.  Rounds 1-3 registered Python functions through
// torch.library (no Meta kernel: FakeTensor tracing / torch.compile of the drop-in modules could not work, and every call paid Python
// dispatch); this translation unit replaces them.  It is host code only: it validates tensors, allocates outputs with ATen and calls
//   ww_logmel_f32 / ww_cnn_pool_f32 / ww_lstm_fc_f32 / ww_model_forward_f32 / ww_forward_pcm_f32      (include/wakeword_amd.h)
// and, for clips of 0.25 s to 2 s, ww_logmel_frames_f32 / ww_cnn_pool_wide_f32 / ww_forward_pcm_frames_f32, and ww_spec_augment_f32 and
// ww_channel_f32
// on torch's current HIP stream.  The ww_* functions are neither linked nor looked up by name: the Python package hands their ADDRESSES in
// (ww_torch_bind, from the ctypes handle of libwakeword_amd.so or of the build named by WW_LIB_OVERRIDE), so nothing enters the global
// symbol scope -- several builds of the library can live in one process (scripts/ab_kernels.py) without interposing each other's kernels.
//
// Reference call sites these operators stand behind: AudioProcessor.audio_to_mel (wakeword_training_script.py:85-101) -> logmel;
// SimpleWakewordModel.forward (wakeword_training/train_wakeword.py:38-49) / WakewordModel.forward (wakeword_training_script.py:167-184)
// -> cnn_lstm_forward (= cnn_pool + lstm_fc); the batched inference loop (notebook cell 17) on raw clips -> forward_pcm.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "wakeword_amd.h"

namespace {

constexpr int64_t kClip = WW_CLIP_SAMPLES, kMels = WW_N_MELS, kFrames = WW_N_FRAMES;
constexpr int64_t kMinSamples = WW_MIN_CLIP_SAMPLES, kMaxSamples = WW_MAX_CLIP_SAMPLES, kMaxFrames = WW_MAX_FRAMES;

// the C ABI entry points this library calls, bound once by ww_torch_bind (order = ops.py::_TORCH_BIND_ORDER)
struct Abi {
    decltype(&::ww_last_error) last_error = nullptr;
    decltype(&::ww_packed_weights_floats) packed_weights_floats = nullptr;
    decltype(&::ww_cnn_scratch_bytes) cnn_scratch_bytes = nullptr;
    decltype(&::ww_workspace_bytes) workspace_bytes = nullptr;
    decltype(&::ww_logmel_f32) logmel_f32 = nullptr;
    decltype(&::ww_cnn_pool_f32) cnn_pool_f32 = nullptr;
    decltype(&::ww_lstm_fc_f32) lstm_fc_f32 = nullptr;
    decltype(&::ww_model_forward_f32) model_forward_f32 = nullptr;
    decltype(&::ww_forward_pcm_f32) forward_pcm_f32 = nullptr;
    decltype(&::ww_logmel_frames_f32) logmel_frames_f32 = nullptr;
    decltype(&::ww_cnn_wide_scratch_bytes) cnn_wide_scratch_bytes = nullptr;
    decltype(&::ww_cnn_pool_wide_f32) cnn_pool_wide_f32 = nullptr;
    decltype(&::ww_workspace_frames_bytes) workspace_frames_bytes = nullptr;
    decltype(&::ww_forward_pcm_frames_f32) forward_pcm_frames_f32 = nullptr;
    decltype(&::ww_spec_augment_f32) spec_augment_f32 = nullptr;
    decltype(&::ww_channel_f32) channel_f32 = nullptr;
} abi;
constexpr int kAbiEntries = 16;
const Abi& bound() {
    TORCH_CHECK(abi.forward_pcm_f32 != nullptr, "wakeword_amd: the operators are not bound to libwakeword_amd.so (import wakeword_jupyterlab_amd does it)");
    return abi;
}
#define ww_last_error bound().last_error
#define ww_packed_weights_floats bound().packed_weights_floats
#define ww_cnn_scratch_bytes bound().cnn_scratch_bytes
#define ww_workspace_bytes bound().workspace_bytes
#define ww_logmel_f32 bound().logmel_f32
#define ww_cnn_pool_f32 bound().cnn_pool_f32
#define ww_lstm_fc_f32 bound().lstm_fc_f32
#define ww_model_forward_f32 bound().model_forward_f32
#define ww_forward_pcm_f32 bound().forward_pcm_f32
#define ww_logmel_frames_f32 bound().logmel_frames_f32
#define ww_cnn_wide_scratch_bytes bound().cnn_wide_scratch_bytes
#define ww_cnn_pool_wide_f32 bound().cnn_pool_wide_f32
#define ww_workspace_frames_bytes bound().workspace_frames_bytes
#define ww_forward_pcm_frames_f32 bound().forward_pcm_frames_f32
#define ww_spec_augment_f32 bound().spec_augment_f32
#define ww_channel_f32 bound().channel_f32

void* stream_of(const at::Tensor& t) { return static_cast<void*>(c10::hip::getCurrentHIPStream(t.device().index()).stream()); }

void check_rc(int64_t rc, const char* what) {
    TORCH_CHECK(rc >= 0, "wakeword_amd::", what, ": ", ww_last_error() ? ww_last_error() : "native call failed", " (code ", rc, ")");
}

void require_cuda_f32(const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.device().is_cuda(), name, " is on ", t.device(), ": this path has no CPU implementation; move it to the MI355X (`.cuda()`)");
    TORCH_CHECK(t.scalar_type() == at::kFloat, name, ": expected float32, got ", t.scalar_type());
}

int64_t c_last(int64_t n_conv) {
    TORCH_CHECK(n_conv == 2 || n_conv == 3, "n_conv must be 2 or 3, got ", n_conv);
    return n_conv == 2 ? 64 : 128;
}

// [B, n <= 16000] float32 with unit sample stride, row stride a multiple of 4 floats and a 16-byte aligned base, copying only if needed
// (max_samples: the clip length of the *_frames ops, n_samples; the 1 s ops take 16000)
at::Tensor checked_pcm(const at::Tensor& pcm, int64_t max_samples = kClip) {
    require_cuda_f32(pcm, "pcm");
    TORCH_CHECK(pcm.dim() == 2, "pcm: expected [B, samples], got ", pcm.sizes());
    const int64_t B = pcm.size(0), n = pcm.size(1);
    TORCH_CHECK(n >= 1 && n <= max_samples, "pcm: ", n, " samples per clip; the front-end takes 1..", max_samples,
                " (crop longer clips on the host, pad_or_truncate wakeword_training_script.py:78-83)");
    if (pcm.stride(1) == 1 && (B <= 1 || pcm.stride(0) % 4 == 0) && reinterpret_cast<uintptr_t>(pcm.data_ptr()) % 16 == 0) return pcm;
    at::Tensor p = pcm.contiguous();
    if (n % 4 && B > 1) {
        at::Tensor pad = at::zeros({B, (n + 3) / 4 * 4}, pcm.options());
        pad.narrow(1, 0, n).copy_(p);
        p = pad.narrow(1, 0, n);
    }
    return p;
}

at::Tensor checked_x(const at::Tensor& x) {
    require_cuda_f32(x, "x");
    TORCH_CHECK(x.dim() == 4 && x.size(1) == 1 && x.size(2) == kMels, "x: expected [B, 1, ", kMels, ", T], got ", x.sizes());
    TORCH_CHECK_NOT_IMPLEMENTED(x.size(3) >= 1 && x.size(3) <= 32, "x: T = ", x.size(3), " frames; the conv kernels are built for 1..32 (1 s clips give 32)");
    return x.contiguous();
}

at::Tensor checked_x_wide(const at::Tensor& x) {
    require_cuda_f32(x, "x");
    TORCH_CHECK(x.dim() == 4 && x.size(1) == 1 && x.size(2) == kMels, "x: expected [B, 1, ", kMels, ", T], got ", x.sizes());
    TORCH_CHECK(x.size(3) >= 1 && x.size(3) <= kMaxFrames, "x: T = ", x.size(3), " frames; the wide conv stack takes 1..", kMaxFrames, " (2 s clips give 63)");
    return x.contiguous();
}

int64_t frames_of(int64_t n_samples) {
    TORCH_CHECK(n_samples >= kMinSamples && n_samples <= kMaxSamples, "n_samples = ", n_samples, ": clips of ", kMinSamples, "..", kMaxSamples,
                " samples (0.25 s .. 2 s)");
    return 1 + n_samples / WW_HOP;
}

void check_packed(const at::Tensor& packed, int64_t n_conv, const at::Tensor& like) {
    require_cuda_f32(packed, "packed weights");
    TORCH_CHECK(packed.device() == like.device(), "packed weights on ", packed.device(), ", input on ", like.device());
    TORCH_CHECK((n_conv == 2 || n_conv == 3) && packed.is_contiguous() && packed.numel() == ww_packed_weights_floats(int32_t(n_conv)),
                "packed weights do not match n_conv (use ops.pack_state_dict)");
}

// ---------------------------------------------------------------- CUDA (HIP) kernels
at::Tensor logmel_cuda(const at::Tensor& pcm_in, bool normalize) {
    const at::Tensor pcm = checked_pcm(pcm_in);
    const int64_t B = pcm.size(0), n = pcm.size(1);
    at::Tensor out = at::empty({B, 1, kMels, kFrames}, pcm.options());
    c10::DeviceGuard guard(pcm.device());
    check_rc(ww_logmel_f32(pcm.data_ptr<float>(), B, B > 1 ? pcm.stride(0) : n, n, normalize ? 1 : 0, out.data_ptr<float>(), stream_of(pcm)), "logmel");
    return out;
}

at::Tensor cnn_pool_cuda(const at::Tensor& x_in, const at::Tensor& packed, int64_t n_conv) {
    const at::Tensor x = checked_x(x_in);
    check_packed(packed, n_conv, x);
    const int64_t B = x.size(0), T = x.size(3);
    at::Tensor pooled = at::empty({B, c_last(n_conv)}, x.options());
    const int64_t nbytes = ww_cnn_scratch_bytes(B, int32_t(n_conv));
    check_rc(nbytes, "cnn_pool");
    at::Tensor scratch = at::empty({nbytes > 0 ? nbytes : 1}, x.options().dtype(at::kByte));
    c10::DeviceGuard guard(x.device());
    check_rc(ww_cnn_pool_f32(x.data_ptr<float>(), B, int32_t(T), packed.data_ptr<float>(), int32_t(n_conv), nbytes > 0 ? scratch.data_ptr() : nullptr,
                             pooled.data_ptr<float>(), stream_of(x)), "cnn_pool");
    return pooled;
}

at::Tensor lstm_fc_cuda(const at::Tensor& pooled_in, const at::Tensor& packed, int64_t n_conv) {
    require_cuda_f32(pooled_in, "pooled");
    check_packed(packed, n_conv, pooled_in);
    TORCH_CHECK(pooled_in.dim() == 2 && pooled_in.size(1) == c_last(n_conv), "pooled: expected [B, ", c_last(n_conv), "], got ", pooled_in.sizes());
    const at::Tensor pooled = pooled_in.contiguous();
    at::Tensor logits = at::empty({pooled.size(0), 2}, pooled.options());
    c10::DeviceGuard guard(pooled.device());
    check_rc(ww_lstm_fc_f32(pooled.data_ptr<float>(), pooled.size(0), packed.data_ptr<float>(), int32_t(n_conv), logits.data_ptr<float>(),
                            stream_of(pooled)), "lstm_fc");
    return logits;
}

at::Tensor workspace(int64_t n, int64_t n_conv, const at::Tensor& like) {
    const int64_t nbytes = ww_workspace_bytes(n, int32_t(n_conv));
    check_rc(nbytes, "workspace");
    return at::empty({nbytes > 0 ? nbytes : 1}, like.options().dtype(at::kByte));
}

at::Tensor cnn_lstm_forward_cuda(const at::Tensor& x_in, const at::Tensor& packed, int64_t n_conv) {
    const at::Tensor x = checked_x(x_in);
    check_packed(packed, n_conv, x);
    const int64_t B = x.size(0), T = x.size(3);
    at::Tensor logits = at::empty({B, 2}, x.options());
    at::Tensor ws = workspace(B, n_conv, x);
    c10::DeviceGuard guard(x.device());
    check_rc(ww_model_forward_f32(x.data_ptr<float>(), B, int32_t(T), packed.data_ptr<float>(), int32_t(n_conv), ws.data_ptr(), logits.data_ptr<float>(),
                                  stream_of(x)), "cnn_lstm_forward");
    return logits;
}

at::Tensor forward_pcm_cuda(const at::Tensor& pcm_in, const at::Tensor& packed, int64_t n_conv, bool normalize) {
    const at::Tensor pcm = checked_pcm(pcm_in);
    check_packed(packed, n_conv, pcm);
    const int64_t B = pcm.size(0), n = pcm.size(1);
    at::Tensor logits = at::empty({B, 2}, pcm.options());
    at::Tensor ws = workspace(B, n_conv, pcm);
    c10::DeviceGuard guard(pcm.device());
    check_rc(ww_forward_pcm_f32(pcm.data_ptr<float>(), B, B > 1 ? pcm.stride(0) : n, n, normalize ? 1 : 0, packed.data_ptr<float>(), int32_t(n_conv),
                                ws.data_ptr(), logits.data_ptr<float>(), stream_of(pcm)), "forward_pcm");
    return logits;
}

// clips of n_samples (0.25 s .. 2 s): [B, n <= n_samples] -> [B, 1, 80, T], T = 1 + n_samples / 512
at::Tensor logmel_frames_cuda(const at::Tensor& pcm_in, int64_t n_samples, bool normalize) {
    const int64_t T = frames_of(n_samples);
    const at::Tensor pcm = checked_pcm(pcm_in, n_samples);
    const int64_t B = pcm.size(0), n = pcm.size(1);
    at::Tensor out = at::empty({B, 1, kMels, T}, pcm.options());
    c10::DeviceGuard guard(pcm.device());
    check_rc(ww_logmel_frames_f32(pcm.data_ptr<float>(), B, B > 1 ? pcm.stride(0) : n, n, n_samples, normalize ? 1 : 0, out.data_ptr<float>(),
                                  stream_of(pcm)), "logmel_frames");
    return out;
}

at::Tensor cnn_pool_wide_cuda(const at::Tensor& x_in, const at::Tensor& packed, int64_t n_conv) {
    const at::Tensor x = checked_x_wide(x_in);
    check_packed(packed, n_conv, x);
    const int64_t B = x.size(0), T = x.size(3);
    at::Tensor pooled = at::empty({B, c_last(n_conv)}, x.options());
    const int64_t nbytes = ww_cnn_wide_scratch_bytes(B, int32_t(T), int32_t(n_conv));
    check_rc(nbytes, "cnn_pool_wide");
    at::Tensor scratch = at::empty({nbytes > 0 ? nbytes : 1}, x.options().dtype(at::kByte));
    c10::DeviceGuard guard(x.device());
    check_rc(ww_cnn_pool_wide_f32(x.data_ptr<float>(), B, int32_t(T), packed.data_ptr<float>(), int32_t(n_conv), nbytes > 0 ? scratch.data_ptr() : nullptr,
                                  pooled.data_ptr<float>(), stream_of(x)), "cnn_pool_wide");
    return pooled;
}

at::Tensor forward_pcm_frames_cuda(const at::Tensor& pcm_in, const at::Tensor& packed, int64_t n_conv, int64_t n_samples, bool normalize) {
    (void)frames_of(n_samples);
    const at::Tensor pcm = checked_pcm(pcm_in, n_samples);
    check_packed(packed, n_conv, pcm);
    const int64_t B = pcm.size(0), n = pcm.size(1);
    at::Tensor logits = at::empty({B, 2}, pcm.options());
    const int64_t nbytes = ww_workspace_frames_bytes(B, n_samples, int32_t(n_conv));
    check_rc(nbytes, "forward_pcm_frames");
    at::Tensor ws = at::empty({nbytes > 0 ? nbytes : 1}, pcm.options().dtype(at::kByte));
    c10::DeviceGuard guard(pcm.device());
    check_rc(ww_forward_pcm_frames_f32(pcm.data_ptr<float>(), B, B > 1 ? pcm.stride(0) : n, n, n_samples, normalize ? 1 : 0, packed.data_ptr<float>(),
                                       int32_t(n_conv), ws.data_ptr(), logits.data_ptr<float>(), stream_of(pcm)), "forward_pcm_frames");
    return logits;
}

// SpecAugment, out of place: mel [B, 1, 80, T] or [B, 80, T], records int16 [B, 16] on the same device
void check_spec_shapes(const at::Tensor& mel, const at::Tensor& records) {
    TORCH_CHECK(mel.scalar_type() == at::kFloat, "mel: expected float32, got ", mel.scalar_type());
    TORCH_CHECK((mel.dim() == 4 && mel.size(1) == 1 && mel.size(2) == kMels) || (mel.dim() == 3 && mel.size(1) == kMels),
                "mel: expected [B, 1, ", kMels, ", T] or [B, ", kMels, ", T], got ", mel.sizes());
    const int64_t T = mel.size(mel.dim() - 1);
    TORCH_CHECK_NOT_IMPLEMENTED(T >= 1 && T <= kMaxFrames, "mel: T = ", T, " frames; the masking kernel takes 1..", kMaxFrames);
    TORCH_CHECK(records.scalar_type() == at::kShort && records.dim() == 2 && records.size(0) == mel.size(0) && records.size(1) == WW_SPEC_RECORD_INT16,
                "records: expected int16 [", mel.size(0), ", ", WW_SPEC_RECORD_INT16, "], got ", records.scalar_type(), " ", records.sizes());
    TORCH_CHECK(records.device() == mel.device(), "records on ", records.device(), ", mel on ", mel.device());
}

at::Tensor spec_augment_cuda(const at::Tensor& mel_in, const at::Tensor& records_in, int64_t fill_mode, double fill_value) {
    require_cuda_f32(mel_in, "mel");
    check_spec_shapes(mel_in, records_in);
    TORCH_CHECK(fill_mode >= WW_SPEC_FILL_MEAN && fill_mode <= WW_SPEC_FILL_VALUE, "fill_mode ", fill_mode, ": 0 = mean, 1 = min, 2 = fill_value");
    const at::Tensor mel = mel_in.contiguous();
    at::Tensor records = records_in.contiguous();
    if (reinterpret_cast<uintptr_t>(records.data_ptr()) % 16) records = records.clone();
    at::Tensor out = at::empty_like(mel);
    c10::DeviceGuard guard(mel.device());
    check_rc(ww_spec_augment_f32(mel.data_ptr<float>(), out.data_ptr<float>(), mel.size(0), int32_t(mel.size(mel.dim() - 1)), records.data_ptr<int16_t>(),
                                 0, 0.f, 0, 0, 0, 0, int32_t(fill_mode), float(fill_value), stream_of(mel)), "spec_augment");
    return out;
}

// Microphone-channel augmentation, out of place: pcm [B, N] float32, records float32 [B, 48] on the same device
void check_channel_shapes(const at::Tensor& pcm, const at::Tensor& records) {
    TORCH_CHECK(pcm.scalar_type() == at::kFloat, "pcm: expected float32, got ", pcm.scalar_type());
    TORCH_CHECK(pcm.dim() == 2, "pcm: expected [B, samples], got ", pcm.sizes());
    const int64_t n = pcm.size(1);
    TORCH_CHECK_NOT_IMPLEMENTED(n >= kMinSamples && n <= WW_AUG_MAX_SAMPLES, "pcm: ", n, " samples per clip; the channel stage takes ", kMinSamples,
                                "..", WW_AUG_MAX_SAMPLES);
    TORCH_CHECK(records.scalar_type() == at::kFloat && records.dim() == 2 && records.size(0) == pcm.size(0) && records.size(1) == WW_CHANNEL_RECORD_F32,
                "records: expected float32 [", pcm.size(0), ", ", WW_CHANNEL_RECORD_F32, "], got ", records.scalar_type(), " ", records.sizes());
    TORCH_CHECK(records.device() == pcm.device(), "records on ", records.device(), ", pcm on ", pcm.device());
}

at::Tensor channel_effects_cuda(const at::Tensor& pcm_in, const at::Tensor& records_in) {
    require_cuda_f32(pcm_in, "pcm");
    check_channel_shapes(pcm_in, records_in);
    const at::Tensor pcm = pcm_in.contiguous();
    at::Tensor records = records_in.contiguous();
    if (reinterpret_cast<uintptr_t>(records.data_ptr()) % 16) records = records.clone();
    at::Tensor out = at::empty_like(pcm);
    c10::DeviceGuard guard(pcm.device());
    check_rc(ww_channel_f32(pcm.data_ptr<float>(), out.data_ptr<float>(), pcm.size(0), pcm.size(1), pcm.size(1), records.data_ptr<float>(), 0, nullptr,
                            stream_of(pcm)), "channel_effects");
    return out;
}

// ---------------------------------------------------------------- Meta kernels: shapes only (FakeTensor / torch.compile tracing)
at::Tensor logmel_meta(const at::Tensor& pcm, bool) {
    TORCH_CHECK(pcm.dim() == 2 && pcm.size(1) >= 1 && pcm.size(1) <= kClip, "pcm: expected [B, 1..", kClip, "], got ", pcm.sizes());
    return at::empty({pcm.size(0), 1, kMels, kFrames}, pcm.options().dtype(at::kFloat));
}
at::Tensor cnn_pool_meta(const at::Tensor& x, const at::Tensor&, int64_t n_conv) {
    TORCH_CHECK(x.dim() == 4 && x.size(1) == 1 && x.size(2) == kMels && x.size(3) >= 1 && x.size(3) <= 32, "x: expected [B, 1, ", kMels, ", 1..32], got ", x.sizes());
    return at::empty({x.size(0), c_last(n_conv)}, x.options().dtype(at::kFloat));
}
at::Tensor lstm_fc_meta(const at::Tensor& pooled, const at::Tensor&, int64_t n_conv) {
    TORCH_CHECK(pooled.dim() == 2 && pooled.size(1) == c_last(n_conv), "pooled: expected [B, ", c_last(n_conv), "], got ", pooled.sizes());
    return at::empty({pooled.size(0), 2}, pooled.options().dtype(at::kFloat));
}
at::Tensor cnn_lstm_forward_meta(const at::Tensor& x, const at::Tensor&, int64_t n_conv) {
    TORCH_CHECK(x.dim() == 4 && x.size(1) == 1 && x.size(2) == kMels && x.size(3) >= 1 && x.size(3) <= 32, "x: expected [B, 1, ", kMels, ", 1..32], got ", x.sizes());
    (void)c_last(n_conv);
    return at::empty({x.size(0), 2}, x.options().dtype(at::kFloat));
}
at::Tensor forward_pcm_meta(const at::Tensor& pcm, const at::Tensor&, int64_t n_conv, bool) {
    TORCH_CHECK(pcm.dim() == 2 && pcm.size(1) >= 1 && pcm.size(1) <= kClip, "pcm: expected [B, 1..", kClip, "], got ", pcm.sizes());
    (void)c_last(n_conv);
    return at::empty({pcm.size(0), 2}, pcm.options().dtype(at::kFloat));
}

at::Tensor logmel_frames_meta(const at::Tensor& pcm, int64_t n_samples, bool) {
    const int64_t T = frames_of(n_samples);
    TORCH_CHECK(pcm.dim() == 2 && pcm.size(1) >= 1 && pcm.size(1) <= n_samples, "pcm: expected [B, 1..", n_samples, "], got ", pcm.sizes());
    return at::empty({pcm.size(0), 1, kMels, T}, pcm.options().dtype(at::kFloat));
}
at::Tensor cnn_pool_wide_meta(const at::Tensor& x, const at::Tensor&, int64_t n_conv) {
    TORCH_CHECK(x.dim() == 4 && x.size(1) == 1 && x.size(2) == kMels && x.size(3) >= 1 && x.size(3) <= kMaxFrames, "x: expected [B, 1, ", kMels,
                ", 1..", kMaxFrames, "], got ", x.sizes());
    return at::empty({x.size(0), c_last(n_conv)}, x.options().dtype(at::kFloat));
}
at::Tensor forward_pcm_frames_meta(const at::Tensor& pcm, const at::Tensor&, int64_t n_conv, int64_t n_samples, bool) {
    (void)frames_of(n_samples);
    TORCH_CHECK(pcm.dim() == 2 && pcm.size(1) >= 1 && pcm.size(1) <= n_samples, "pcm: expected [B, 1..", n_samples, "], got ", pcm.sizes());
    (void)c_last(n_conv);
    return at::empty({pcm.size(0), 2}, pcm.options().dtype(at::kFloat));
}

at::Tensor spec_augment_meta(const at::Tensor& mel, const at::Tensor& records, int64_t fill_mode, double) {
    check_spec_shapes(mel, records);
    TORCH_CHECK(fill_mode >= WW_SPEC_FILL_MEAN && fill_mode <= WW_SPEC_FILL_VALUE, "fill_mode ", fill_mode, ": 0 = mean, 1 = min, 2 = fill_value");
    return at::empty(mel.sizes(), mel.options());
}

at::Tensor channel_effects_meta(const at::Tensor& pcm, const at::Tensor& records) {
    check_channel_shapes(pcm, records);
    return at::empty(pcm.sizes(), pcm.options());
}

// ---------------------------------------------------------------- CPU: there is none
[[noreturn]] void no_cpu(const char* name) {
    TORCH_CHECK(false, "wakeword_amd::", name, ": no CPU implementation exists (HIP/gfx950 only); move the tensors to the GPU");
}
at::Tensor logmel_cpu(const at::Tensor&, bool) { no_cpu("logmel"); }
at::Tensor cnn_pool_cpu(const at::Tensor&, const at::Tensor&, int64_t) { no_cpu("cnn_pool"); }
at::Tensor lstm_fc_cpu(const at::Tensor&, const at::Tensor&, int64_t) { no_cpu("lstm_fc"); }
at::Tensor cnn_lstm_forward_cpu(const at::Tensor&, const at::Tensor&, int64_t) { no_cpu("cnn_lstm_forward"); }
at::Tensor forward_pcm_cpu(const at::Tensor&, const at::Tensor&, int64_t, bool) { no_cpu("forward_pcm"); }
at::Tensor logmel_frames_cpu(const at::Tensor&, int64_t, bool) { no_cpu("logmel_frames"); }
at::Tensor cnn_pool_wide_cpu(const at::Tensor&, const at::Tensor&, int64_t) { no_cpu("cnn_pool_wide"); }
at::Tensor forward_pcm_frames_cpu(const at::Tensor&, const at::Tensor&, int64_t, int64_t, bool) { no_cpu("forward_pcm_frames"); }
at::Tensor spec_augment_cpu(const at::Tensor&, const at::Tensor&, int64_t, double) { no_cpu("spec_augment"); }
at::Tensor channel_effects_cpu(const at::Tensor&, const at::Tensor&) { no_cpu("channel_effects"); }

}  // namespace

#undef ww_last_error
#undef ww_packed_weights_floats
#undef ww_cnn_scratch_bytes
#undef ww_workspace_bytes
#undef ww_logmel_f32
#undef ww_cnn_pool_f32
#undef ww_lstm_fc_f32
#undef ww_model_forward_f32
#undef ww_forward_pcm_f32
#undef ww_logmel_frames_f32
#undef ww_cnn_wide_scratch_bytes
#undef ww_cnn_pool_wide_f32
#undef ww_workspace_frames_bytes
#undef ww_forward_pcm_frames_f32
#undef ww_spec_augment_f32
#undef ww_channel_f32

// fns[kAbiEntries]: addresses of ww_last_error, ww_packed_weights_floats, ww_cnn_scratch_bytes, ww_workspace_bytes, ww_logmel_f32,
// ww_cnn_pool_f32, ww_lstm_fc_f32, ww_model_forward_f32, ww_forward_pcm_f32, ww_logmel_frames_f32, ww_cnn_wide_scratch_bytes, ww_cnn_pool_wide_f32,
// ww_workspace_frames_bytes, ww_forward_pcm_frames_f32, ww_spec_augment_f32, ww_channel_f32 of ONE build of libwakeword_amd.so.  Returns 0, or -1 on a bad table.
extern "C" __attribute__((visibility("default"))) int ww_torch_bind(const void* const* fns, int n) {
    if (!fns || n != kAbiEntries) return -1;
    for (int i = 0; i < n; ++i)
        if (!fns[i]) return -1;
    abi.last_error = reinterpret_cast<decltype(abi.last_error)>(const_cast<void*>(fns[0]));
    abi.packed_weights_floats = reinterpret_cast<decltype(abi.packed_weights_floats)>(const_cast<void*>(fns[1]));
    abi.cnn_scratch_bytes = reinterpret_cast<decltype(abi.cnn_scratch_bytes)>(const_cast<void*>(fns[2]));
    abi.workspace_bytes = reinterpret_cast<decltype(abi.workspace_bytes)>(const_cast<void*>(fns[3]));
    abi.logmel_f32 = reinterpret_cast<decltype(abi.logmel_f32)>(const_cast<void*>(fns[4]));
    abi.cnn_pool_f32 = reinterpret_cast<decltype(abi.cnn_pool_f32)>(const_cast<void*>(fns[5]));
    abi.lstm_fc_f32 = reinterpret_cast<decltype(abi.lstm_fc_f32)>(const_cast<void*>(fns[6]));
    abi.model_forward_f32 = reinterpret_cast<decltype(abi.model_forward_f32)>(const_cast<void*>(fns[7]));
    abi.forward_pcm_f32 = reinterpret_cast<decltype(abi.forward_pcm_f32)>(const_cast<void*>(fns[8]));
    abi.logmel_frames_f32 = reinterpret_cast<decltype(abi.logmel_frames_f32)>(const_cast<void*>(fns[9]));
    abi.cnn_wide_scratch_bytes = reinterpret_cast<decltype(abi.cnn_wide_scratch_bytes)>(const_cast<void*>(fns[10]));
    abi.cnn_pool_wide_f32 = reinterpret_cast<decltype(abi.cnn_pool_wide_f32)>(const_cast<void*>(fns[11]));
    abi.workspace_frames_bytes = reinterpret_cast<decltype(abi.workspace_frames_bytes)>(const_cast<void*>(fns[12]));
    abi.forward_pcm_frames_f32 = reinterpret_cast<decltype(abi.forward_pcm_frames_f32)>(const_cast<void*>(fns[13]));
    abi.spec_augment_f32 = reinterpret_cast<decltype(abi.spec_augment_f32)>(const_cast<void*>(fns[14]));
    abi.channel_f32 = reinterpret_cast<decltype(abi.channel_f32)>(const_cast<void*>(fns[15]));
    return 0;
}

TORCH_LIBRARY(wakeword_amd, m) {
    m.def("logmel(Tensor pcm, bool normalize=True) -> Tensor");
    m.def("cnn_pool(Tensor x, Tensor packed, int n_conv) -> Tensor");
    m.def("lstm_fc(Tensor pooled, Tensor packed, int n_conv) -> Tensor");
    m.def("cnn_lstm_forward(Tensor x, Tensor packed, int n_conv) -> Tensor");
    m.def("forward_pcm(Tensor pcm, Tensor packed, int n_conv, bool normalize=True) -> Tensor");
    m.def("logmel_frames(Tensor pcm, int n_samples, bool normalize=True) -> Tensor");
    m.def("cnn_pool_wide(Tensor x, Tensor packed, int n_conv) -> Tensor");
    m.def("forward_pcm_frames(Tensor pcm, Tensor packed, int n_conv, int n_samples, bool normalize=True) -> Tensor");
    m.def("spec_augment(Tensor mel, Tensor records, int fill_mode, float fill_value) -> Tensor");
    m.def("channel_effects(Tensor pcm, Tensor records) -> Tensor");
}
TORCH_LIBRARY_IMPL(wakeword_amd, CUDA, m) {
    m.impl("logmel", &logmel_cuda);
    m.impl("cnn_pool", &cnn_pool_cuda);
    m.impl("lstm_fc", &lstm_fc_cuda);
    m.impl("cnn_lstm_forward", &cnn_lstm_forward_cuda);
    m.impl("forward_pcm", &forward_pcm_cuda);
    m.impl("logmel_frames", &logmel_frames_cuda);
    m.impl("cnn_pool_wide", &cnn_pool_wide_cuda);
    m.impl("forward_pcm_frames", &forward_pcm_frames_cuda);
    m.impl("spec_augment", &spec_augment_cuda);
    m.impl("channel_effects", &channel_effects_cuda);
}
TORCH_LIBRARY_IMPL(wakeword_amd, Meta, m) {
    m.impl("logmel", &logmel_meta);
    m.impl("cnn_pool", &cnn_pool_meta);
    m.impl("lstm_fc", &lstm_fc_meta);
    m.impl("cnn_lstm_forward", &cnn_lstm_forward_meta);
    m.impl("forward_pcm", &forward_pcm_meta);
    m.impl("logmel_frames", &logmel_frames_meta);
    m.impl("cnn_pool_wide", &cnn_pool_wide_meta);
    m.impl("forward_pcm_frames", &forward_pcm_frames_meta);
    m.impl("spec_augment", &spec_augment_meta);
    m.impl("channel_effects", &channel_effects_meta);
}
TORCH_LIBRARY_IMPL(wakeword_amd, CPU, m) {
    m.impl("logmel", &logmel_cpu);
    m.impl("cnn_pool", &cnn_pool_cpu);
    m.impl("lstm_fc", &lstm_fc_cpu);
    m.impl("cnn_lstm_forward", &cnn_lstm_forward_cpu);
    m.impl("forward_pcm", &forward_pcm_cpu);
    m.impl("logmel_frames", &logmel_frames_cpu);
    m.impl("cnn_pool_wide", &cnn_pool_wide_cpu);
    m.impl("forward_pcm_frames", &forward_pcm_frames_cpu);
    m.impl("spec_augment", &spec_augment_cpu);
    m.impl("channel_effects", &channel_effects_cpu);
}
