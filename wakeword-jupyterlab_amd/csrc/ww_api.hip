// C ABI entry points of libwakeword_amd.so: argument checking, per-device table cache, the composed
// PCM -> logits path and the hipGraph-captured streaming step.  Declared in include/wakeword_amd.h.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include <atomic>

#include "ww_internal.h"

namespace ww {

constexpr int kMaxDevices = 16;
static std::mutex g_mu;
static LogmelTables* g_tables[kMaxDevices] = {};
static int g_cu[kMaxDevices] = {};
static int g_checked[kMaxDevices] = {};   // 0 unknown, 1 gfx950, -1 refused

static int current_device(int* dev) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(WW_ENODEVICE, "no HIP device visible: the HIP kernels are the only implementation of this path");
    }
    WW_HIP(hipGetDevice(dev));
    if (*dev < 0 || *dev >= kMaxDevices) return fail(WW_EUNSUPPORTED, "device ordinal %d out of range", *dev);
    return WW_OK;
}

int require_gfx950() {
    int dev = 0;
    if (int rc = current_device(&dev)) return rc;
    std::lock_guard<std::mutex> lock(g_mu);
    if (g_checked[dev] == 0) {
        hipDeviceProp_t prop;
        WW_HIP(hipGetDeviceProperties(&prop, dev));
        g_cu[dev] = prop.multiProcessorCount;
        g_checked[dev] = std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : -1;
    }
    if (g_checked[dev] < 0) return fail(WW_ENODEVICE, "device %d is not gfx950 (MI355X): this library carries gfx950 code only", dev);
    return WW_OK;
}

int device_cu_count() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
    return g_cu[dev] > 0 ? g_cu[dev] : 256;
}

const LogmelTables* device_tables() {
    int dev = 0;
    if (require_gfx950() != WW_OK) return nullptr;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(g_mu);
    if (g_tables[dev]) return g_tables[dev];
    LogmelTables* host = new (std::nothrow) LogmelTables;
    if (!host) { fail(WW_EHIP, "out of host memory"); return nullptr; }
    const int pieces = build_logmel_tables(host);
    if (pieces < 0) { delete host; return nullptr; }
    LogmelTables* devp = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&devp), sizeof(LogmelTables));
    if (e == hipSuccess) e = hipMemcpy(devp, host, sizeof(LogmelTables), hipMemcpyHostToDevice);
    delete host;
    if (e != hipSuccess) {
        fail(WW_EHIP, "uploading the log-mel tables failed: %s", hipGetErrorString(e));
        return nullptr;
    }
    g_tables[dev] = devp;
    return devp;
}

// Process-wide defaults (atomics: set from any thread) and per-thread overrides (WW_MATH_INHERIT = none): a launch reads its mode ONCE,
// the calling thread's override first -- two host threads (a streamer and a batch job) can use different arithmetics safely.
static std::atomic<int> g_conv_math{WW_CONV_MATH_F16X3};
static thread_local int t_conv_math = WW_MATH_INHERIT, t_logmel_math = WW_MATH_INHERIT;
static int g_train_math = WW_TRAIN_MATH_F16X3;
int train_math_mode() { return g_train_math; }
int conv_math_mode() { return t_conv_math != WW_MATH_INHERIT ? t_conv_math : g_conv_math.load(std::memory_order_relaxed); }
void set_conv_math_mode(int mode) { g_conv_math.store(mode, std::memory_order_relaxed); }

static std::atomic<int> g_logmel_math{WW_LOGMEL_MATH_AUTO};
int logmel_math_mode() { return t_logmel_math != WW_MATH_INHERIT ? t_logmel_math : g_logmel_math.load(std::memory_order_relaxed); }
void set_logmel_math_mode(int mode) { g_logmel_math.store(mode, std::memory_order_relaxed); }

static int64_t wide_scratch_bytes(int64_t n, int32_t width, int32_t n_conv) {
    return width <= WW_MAX_WIDTH ? cnn_scratch_bytes(n, n_conv) : cnn_wide_scratch_bytes(n, width, n_conv);
}

// THE layout of the forward path's workspace: n log-mel images of T frames, n pooled rows, the conv stack's scratch.  Every size query
// (base == nullptr) and every entry point that walks the workspace goes through here.
struct ForwardWorkspace {
    float* logmel;
    float* pooled;
    void* scratch;
    int64_t total;
};
static ForwardWorkspace forward_workspace(void* base, int64_t n, int T, int n_conv) {
    ForwardWorkspace w{};
    char* p = static_cast<char*>(base);
    int64_t o = 0;
    w.logmel = reinterpret_cast<float*>(p + o); o += up256(n * kMels * T * int64_t(sizeof(float)));
    w.pooled = reinterpret_cast<float*>(p + o); o += up256(n * 128 * int64_t(sizeof(float)));
    w.scratch = p + o; o += up256(wide_scratch_bytes(n, T, n_conv));
    w.total = o;
    return w;
}
static int frames_of(int64_t n_samples) { return int(1 + n_samples / kHop); }

static int cnn_pool_any(const float* mel, int64_t n, int width, const float* packed, int n_conv, void* scratch, float* pooled,
                        hipStream_t st) {
    if (width <= WW_MAX_WIDTH) return launch_cnn_pool(mel, n, width, packed, n_conv, scratch, pooled, st);
    return launch_cnn_pool_wide(mel, n, width, packed, n_conv, scratch, pooled, st);
}
// THE launch chain, mel -> logits (and prob where asked for): what ww_model_forward_f32 runs on the caller's mel images
static int model_chain(const float* mel, int64_t n, int T, const float* packed, int n_conv, const ForwardWorkspace& w, float* logits,
                       float* prob, hipStream_t st) {
    if (int rc = cnn_pool_any(mel, n, T, packed, n_conv, w.scratch, w.pooled, st)) return rc;
    return launch_lstm_fc(w.pooled, n, packed, n_conv, logits, prob, st);
}
// ... and pcm -> logits, rows of n_samples with clip_len valid samples: at n_samples = kClip launch for launch the 1 s chain
// (launch_logmel_frames hands T = 32 to launch_logmel, cnn_pool_any T <= 32 to launch_cnn_pool).  ring_pos: the streamer's window start.
static int forward_chain(const float* pcm, int64_t n, int64_t stride, int64_t clip_len, int64_t n_samples, int normalize,
                         const int32_t* ring_pos, int64_t ring_len, const float* packed, int n_conv, const ForwardWorkspace& w,
                         float* logits, float* prob, hipStream_t st) {
    if (int rc = launch_logmel_frames(pcm, n, stride, clip_len, n_samples, normalize, ring_pos, ring_len, w.logmel, st)) return rc;
    return model_chain(w.logmel, n, frames_of(n_samples), packed, n_conv, w, logits, prob, st);
}

// The pcm rows of every entry point that takes some.  The kinds of call differ in what they allow and in how they word a refusal:
struct RowRule {
    int align;                    // of the pcm base in bytes: 16 where rows are loaded as float4 (then clip_stride % 4 == 0 too), else 4
    int64_t n_max, lo, hi;        // rows; samples per row (n_samples of the augmentation calls, the valid clip_len of the log-mel ones)
    bool len_first;               // a length outside lo..hi is refused before n is looked at, else after the null check
    const char* range;            // that refusal: printf form taking (long long samples, int lo, int hi)
    const char* null;             // a missing pointer
    const char* misaligned;       // pcm or clip_stride: printf form taking (const void* pcm, long long clip_stride)
    const char* out_misaligned;   // out_dev or workspace_dev of the calls that write rows; nullptr for the calls that have none
};
constexpr RowRule kClipRows = {16, int64_t(1) << 30, 1, kClip, false,
                               "clip_len %lld: expected %d..%d samples (longer clips are cropped by the host, pad_or_truncate "
                               "wakeword_training_script.py:78-83)",
                               "null pcm pointer", "pcm must be 16-byte aligned with clip_stride %% 4 == 0 (got %p, %lld)", nullptr};
constexpr RowRule kFrameRows = {16, int64_t(1) << 30, 1, WW_MAX_CLIP_SAMPLES, false, "clip_len %lld: expected >= %d",
                                "null pcm / output pointer", "pcm must be 16-byte aligned with clip_stride %% 4 == 0", nullptr};
constexpr RowRule kAugRows = {16, int64_t(1) << 24, WW_MIN_CLIP_SAMPLES, WW_AUG_MAX_SAMPLES, true,
                              "n_samples %lld: augmentation takes %d..%d samples (0.25 s .. 32 frames at 16 kHz)",
                              "null pcm / plan / output / workspace pointer",
                              "pcm must be 16-byte aligned with clip_stride %% 4 == 0 (got %p, %lld)",
                              "out_dev must be 4-byte and workspace_dev 256-byte aligned"};
// the standalone mix and reverb: rows of every inference length, 4-byte aligned (`range` names the call)
constexpr RowRule rows_4(const char* range) {
    return {4, int64_t(1) << 24, WW_MIN_CLIP_SAMPLES, WW_MAX_CLIP_SAMPLES, true, range, "null pcm / output / workspace pointer",
            "pcm_dev / out_dev must be 4-byte and workspace_dev 256-byte aligned",
            "pcm_dev / out_dev must be 4-byte and workspace_dev 256-byte aligned"};
}
constexpr RowRule kMixRows = rows_4("n_samples %lld: the mix takes %d..%d samples (0.25 .. 2 s at 16 kHz)");
constexpr RowRule kReverbRows = rows_4("n_samples %lld: the reverb takes %d..%d samples (0.25 .. 2 s at 16 kHz)");

// `c`: pcm, n, stride and n_samples (the length the rule bounds), and out / out_stride / workspace where the rule has output rows;
// `others`: the call's remaining pointers are all there.  A single row has no second one: its stride is never looked at.
static int check_rows(const RowRule& k, const AugCall& c, bool others = true) {
    const bool bad_len = c.n_samples < k.lo || c.n_samples > k.hi;
    if (k.len_first && bad_len) return fail(WW_EINVAL, k.range, (long long)c.n_samples, int(k.lo), int(k.hi));
    if (c.n < 0 || c.n > k.n_max) return fail(WW_EINVAL, "n_clips %lld out of range", (long long)c.n);
    if (c.n == 0) return WW_OK;
    if (!c.pcm || !others || (k.out_misaligned && (!c.out || !c.workspace))) return fail(WW_EINVAL, "%s", k.null);
    if (bad_len) return fail(WW_EINVAL, k.range, (long long)c.n_samples, int(k.lo), int(k.hi));
    if (k.out_misaligned) {
        if (c.n > 1 && (c.stride < c.n_samples || c.out_stride < c.n_samples))
            return fail(WW_EINVAL, "clip_stride %lld / out_stride %lld < n_samples %lld", (long long)c.stride, (long long)c.out_stride,
                        (long long)c.n_samples);
    } else if (c.n > 1 && c.stride < c.n_samples) {
        return fail(WW_EINVAL, "clip_stride %lld < clip_len %lld", (long long)c.stride, (long long)c.n_samples);
    }
    if ((reinterpret_cast<uintptr_t>(c.pcm) & (k.align - 1)) || (k.align == 16 && c.n > 1 && (c.stride & 3)))
        return fail(WW_EINVAL, k.misaligned, (const void*)c.pcm, (long long)c.stride);
    if (k.out_misaligned && ((reinterpret_cast<uintptr_t>(c.out) & 3) || (reinterpret_cast<uintptr_t>(c.workspace) & 255)))
        return fail(WW_EINVAL, "%s", k.out_misaligned);
    return WW_OK;
}

static int check_model(int64_t n, int32_t width, const float* packed, int32_t n_conv) {
    if (n < 0 || n > (int64_t(1) << 30)) return fail(WW_EINVAL, "batch %lld out of range", (long long)n);
    if (n_conv != 2 && n_conv != 3) return fail(WW_EINVAL, "n_conv must be 2 or 3, got %d", n_conv);
    if (width < 1 || width > WW_MAX_WIDTH) return fail(WW_EUNSUPPORTED, "mel width %d: the conv kernels take 1..%d frames", width, WW_MAX_WIDTH);
    if (n > 0 && (!packed || (reinterpret_cast<uintptr_t>(packed) & 15))) return fail(WW_EINVAL, "packed weights must be a 16-byte aligned device pointer");
    return WW_OK;
}

}  // namespace ww

using namespace ww;

// --------------------------------------------------------------------------------------------------
// streaming
// --------------------------------------------------------------------------------------------------
struct ww_streamer {
    int n_mics, hop, n_conv;
    int n_samples, n_frames;   // window N (16000 at 1 s) and its T = 1 + N / 512 mel frames
    const float* packed;
    hipStream_t stream;
    float* ring;         // [n_mics][n_samples]
    int32_t* pos;        // device: [0] index of the oldest sample (== next write position), [1] append-kernel ticket,
                         // [2], [3] the input-format kernel's history parity and hop count
    bool input;          // hops in the microphone's own format (ww_streamer_create_input other than 16 kHz float32 mono)
    StreamInput in;      // its rate, format, channels, filter table and history
    void* workspace;
    hipGraph_t graph;
    hipGraphExec_t exec;
    const void* cap_hop;
    float* cap_prob;
    float* cap_logits;
    float* own_logits;   // used when the caller passes logits_dev == NULL
};

// Append one hop to every microphone's ring and THEN advance the shared ring position, in one launch: every workgroup
// reads `pos` before it writes samples and takes a ticket after; the workgroup that draws the last ticket knows all
// others are past their read of `pos` and publishes pos + hop for the kernels that follow in the graph.
__global__ void ring_append_kernel(float* __restrict__ ring, int32_t* __restrict__ pos_p, uint32_t* __restrict__ ticket,
                                   const float* __restrict__ hop, int n_mics, int hop_len, int ring_len) {
    const int pos = *reinterpret_cast<volatile int32_t*>(pos_p);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_mics * hop_len; i += gridDim.x * blockDim.x) {
        const int m = i / hop_len, k = i - m * hop_len;
        int at = pos + k;
        if (at >= ring_len) at -= ring_len;
        ring[int64_t(m) * ring_len + at] = hop[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicInc(ticket, gridDim.x - 1) == gridDim.x - 1) {     // wraps to 0: ready for the next replay
            const int p = pos + hop_len;
            *pos_p = p >= ring_len ? p - ring_len : p;
        }
    }
}
__global__ void ring_unroll_kernel(const float* __restrict__ ring, const int32_t* __restrict__ pos_p,
                                   float* __restrict__ out, int n_mics, int ring_len) {
    const int pos = *pos_p;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < int64_t(n_mics) * ring_len;
         i += int64_t(gridDim.x) * blockDim.x) {
        const int m = int(i / ring_len), k = int(i - int64_t(m) * ring_len);
        int at = pos + k;
        if (at >= ring_len) at -= ring_len;
        out[i] = ring[int64_t(m) * ring_len + at];
    }
}

static int streamer_enqueue(ww_streamer* s, const void* hop_dev, float* prob_dev, float* logits_dev) {
    if (s->input) {
        // convert + resample the hop into the ring (ww_decode.hip), in place of the float32 16 kHz append
        if (int rc = launch_stream_input(s->in, hop_dev, s->n_mics, s->ring, s->pos, s->n_samples, s->stream)) return rc;
    } else {
        const int threads = 256;
        const int blocks = (s->n_mics * s->hop + threads - 1) / threads;
        if (int rc = launch<ring_append_kernel>(dim3(blocks), dim3(threads), 0, s->stream, s->ring, s->pos, reinterpret_cast<uint32_t*>(s->pos + 1),
                                                static_cast<const float*>(hop_dev), s->n_mics, s->hop, s->n_samples)) return rc;
    }
    // N = 16000 (T = 32) is launch_logmel's 1 s ring kernel with the same arguments as ever; other N the 64-frame tile in ring form
    const int N = s->n_samples;
    return forward_chain(s->ring, s->n_mics, N, N, N, 1, s->pos, N, s->packed, s->n_conv,
                         forward_workspace(s->workspace, s->n_mics, s->n_frames, s->n_conv), logits_dev, prob_dev, s->stream);
}

extern "C" {

int ww_set_conv_math(int mode) {
    if (mode != WW_CONV_MATH_F32 && mode != WW_CONV_MATH_F16X3 && mode != WW_CONV_MATH_F16X3_DIRECT)
        return fail(WW_EINVAL, "unknown conv math mode %d", mode);
    set_conv_math_mode(mode);
    return WW_OK;
}
int ww_get_conv_math(void) { return conv_math_mode(); }
int ww_set_conv_math_thread(int mode) {
    if (mode != WW_MATH_INHERIT && mode != WW_CONV_MATH_F32 && mode != WW_CONV_MATH_F16X3 && mode != WW_CONV_MATH_F16X3_DIRECT)
        return fail(WW_EINVAL, "unknown conv math mode %d", mode);
    t_conv_math = mode;
    return WW_OK;
}
int ww_set_train_math(int mode) {
    if (mode != WW_TRAIN_MATH_F32 && mode != WW_TRAIN_MATH_F16X3) return fail(WW_EINVAL, "train math %d: expected WW_TRAIN_MATH_F32 or WW_TRAIN_MATH_F16X3", mode);
    g_train_math = mode;
    return WW_OK;
}
int ww_get_train_math(void) { return g_train_math; }

int ww_set_logmel_math(int mode) {
    if (mode != WW_LOGMEL_MATH_F32 && mode != WW_LOGMEL_MATH_F64 && mode != WW_LOGMEL_MATH_AUTO)
        return fail(WW_EINVAL, "unknown log-mel math mode %d", mode);
    set_logmel_math_mode(mode);
    return WW_OK;
}
int ww_get_logmel_math(void) { return logmel_math_mode(); }
int ww_set_logmel_math_thread(int mode) {
    if (mode != WW_MATH_INHERIT && mode != WW_LOGMEL_MATH_F32 && mode != WW_LOGMEL_MATH_F64 && mode != WW_LOGMEL_MATH_AUTO)
        return fail(WW_EINVAL, "unknown log-mel math mode %d", mode);
    t_logmel_math = mode;
    return WW_OK;
}

int ww_init(void) {
    if (int rc = require_gfx950()) return rc;
    return device_tables() ? WW_OK : WW_EHIP;
}

int ww_sync_timeouts(void) {
    if (int rc = require_gfx950()) return rc;
    unsigned int c = 0;
    if (int rc = sync_timeouts(&c)) return rc;
    return int(c > 0x7fffffffu ? 0x7fffffffu : c);
}

int ww_flac_errors(void) {
    if (int rc = require_gfx950()) return rc;
    WW_HIP(hipDeviceSynchronize());
    unsigned int c = 0;
    if (int rc = flac_errors(&c)) return rc;
    return int(c > 0x7fffffffu ? 0x7fffffffu : c);
}

int ww_device_info(int* n_cu, int* clock_khz, char* name, int name_len) {
    if (int rc = require_gfx950()) return rc;
    int dev = 0;
    WW_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    WW_HIP(hipGetDeviceProperties(&prop, dev));
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (clock_khz) *clock_khz = prop.clockRate;
    if (name && name_len > 0) std::snprintf(name, size_t(name_len), "%s (%s)", prop.name, prop.gcnArchName);
    return WW_OK;
}

int ww_logmel_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t clip_len, int normalize,
                  float* logmel_dev, ww_stream_t stream) {
    if (int rc = check_rows(kClipRows, {pcm_dev, n_clips, clip_stride, clip_len})) return rc;
    if (n_clips > 0 && !logmel_dev) return fail(WW_EINVAL, "null output pointer");
    if (int rc = require_gfx950()) return rc;
    return launch_logmel(pcm_dev, n_clips, clip_stride, clip_len, normalize, nullptr, 0, logmel_dev,
                         static_cast<hipStream_t>(stream));
}

static int check_n_clips(int64_t n_clips) {
    if (n_clips < 0 || n_clips > (int64_t(1) << 24)) return fail(WW_EINVAL, "n_clips %lld out of range", (long long)n_clips);
    return WW_OK;
}

// Every direct augmentation call after its argument checks: the records prepared once (every refusal before the device check and any
// launch), then staged and launched
static int augment_direct(const AugCall& call, unsigned parts, const ww_augment_plan* plans_host, const ww_augment_bg* bg_host,
                          const ww_augment_rir* rir_host) {
    std::vector<char> rec(size_t(call.n * augment_record_bytes(parts)));
    AugStages st;
    if (int rc = augment_prepare(plans_host, bg_host, rir_host, call.n, call.n_samples, call.bank_len, call.n_rirs, parts, rec.data(), &st))
        return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_augment(call, rec.data(), parts, st);
}

int64_t ww_augment_workspace_bytes(int64_t n_clips) {
    if (int rc = check_n_clips(n_clips)) return rc;
    return augment_workspace_bytes(n_clips, kClip, 0);
}

int ww_augment_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, const ww_augment_plan* plans_host,
                   float* out_dev, void* workspace_dev, ww_stream_t stream) {
    if (int rc = check_n_clips(n_clips)) return rc;
    if (int rc = check_rows(kClipRows, {pcm_dev, n_clips, clip_stride, kClip})) return rc;
    if (n_clips == 0) return WW_OK;
    if (!plans_host || !out_dev || !workspace_dev) return fail(WW_EINVAL, "null plan / output / workspace pointer");
    if ((reinterpret_cast<uintptr_t>(out_dev) & 15) || (reinterpret_cast<uintptr_t>(workspace_dev) & 255))
        return fail(WW_EINVAL, "out_dev must be 16-byte and workspace_dev 256-byte aligned");
    return augment_direct({pcm_dev, n_clips, clip_stride, kClip, out_dev, kClip, workspace_dev, static_cast<hipStream_t>(stream)}, 0, plans_host,
                          nullptr, nullptr);
}

int64_t ww_augment_record_bytes(void) { return augment_record_bytes(0); }

int ww_augment_plans_prepare(const ww_augment_plan* plans_host, int64_t n_clips, void* records_host) {
    if (int rc = check_n_clips(n_clips)) return rc;
    if (n_clips == 0) return WW_OK;
    if (!plans_host || !records_host) return fail(WW_EINVAL, "null plan / record pointer");
    return augment_prepare(plans_host, nullptr, nullptr, n_clips, kClip, 0, 0, 0, records_host, nullptr);
}

int ww_augment_records_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, const void* records_dev, float* out_dev,
                           void* workspace_dev, ww_stream_t stream) {
    if (int rc = check_n_clips(n_clips)) return rc;
    if (int rc = check_rows(kClipRows, {pcm_dev, n_clips, clip_stride, kClip})) return rc;
    if (n_clips == 0) return WW_OK;
    if (!records_dev || !out_dev || !workspace_dev) return fail(WW_EINVAL, "null record / output / workspace pointer");
    if ((reinterpret_cast<uintptr_t>(out_dev) & 15) || (reinterpret_cast<uintptr_t>(workspace_dev) & 255) || (reinterpret_cast<uintptr_t>(records_dev) & 7))
        return fail(WW_EINVAL, "out_dev must be 16-byte, workspace_dev 256-byte and records_dev 8-byte aligned");
    if (int rc = require_gfx950()) return rc;
    return launch_augment_records({pcm_dev, n_clips, clip_stride, kClip, out_dev, kClip, workspace_dev, static_cast<hipStream_t>(stream)},
                                  records_dev, 0);
}

// ---- augmentation of clips of n_samples in [WW_MIN_CLIP_SAMPLES, WW_AUG_MAX_SAMPLES] (the 1 s entry points above are unchanged) ----
static int check_aug_samples(int64_t n_samples) {
    if (n_samples < WW_MIN_CLIP_SAMPLES || n_samples > WW_AUG_MAX_SAMPLES)
        return fail(WW_EINVAL, kAugRows.range, (long long)n_samples, WW_MIN_CLIP_SAMPLES, WW_AUG_MAX_SAMPLES);
    return WW_OK;
}
static int check_aug_sizes(int64_t n_clips, int64_t n_samples) {
    if (int rc = check_aug_samples(n_samples)) return rc;
    return check_n_clips(n_clips);
}
// The *_records calls of the lengths above: the checks, then nothing but launches
static int augment_records(const AugCall& c, const void* records_dev, unsigned parts) {
    if (int rc = check_rows(kAugRows, c, records_dev != nullptr)) return rc;
    if (c.n == 0) return WW_OK;
    if (reinterpret_cast<uintptr_t>(records_dev) & 7) return fail(WW_EINVAL, "records_dev must be 8-byte aligned");
    if ((parts & kAugBg) && (c.bank_len < 0 || (c.bank_len > 0 && !c.bank)))
        return fail(WW_EINVAL, "bank: null pointer or bank_len %lld < 0", (long long)c.bank_len);
    if ((parts & kAugRir) && (c.n_rirs < 0 || (c.n_rirs > 0 && !c.spectra) || (reinterpret_cast<uintptr_t>(c.spectra) & 7)))
        return fail(WW_EINVAL, "spectra: null or unaligned pointer, or n_rirs %lld < 0", (long long)c.n_rirs);
    if (int rc = require_gfx950()) return rc;
    return launch_augment_records(c, records_dev, parts);
}

int64_t ww_augment_n_workspace_bytes(int64_t n_clips, int64_t n_samples) {
    if (int rc = check_aug_sizes(n_clips, n_samples)) return rc;
    return augment_workspace_bytes(n_clips, n_samples, 0);
}

int ww_augment_workspace_layout(int64_t n_clips, int64_t n_samples, ww_augment_layout* layout_out) {
    if (n_samples != kClip)
        if (int rc = check_aug_samples(n_samples)) return rc;
    if (int rc = check_n_clips(n_clips)) return rc;
    if (!layout_out) return fail(WW_EINVAL, "null layout pointer");
    *layout_out = augment_workspace_layout(n_clips, n_samples);
    return WW_OK;
}

int ww_augment_n_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_plan* plans_host,
                     float* out_dev, int64_t out_stride, void* workspace_dev, ww_stream_t stream) {
    const AugCall c = {pcm_dev, n_clips, clip_stride, n_samples, out_dev, out_stride, workspace_dev, static_cast<hipStream_t>(stream)};
    if (int rc = check_rows(kAugRows, c, plans_host != nullptr)) return rc;
    if (n_clips == 0) return WW_OK;
    return augment_direct(c, 0, plans_host, nullptr, nullptr);
}

int ww_augment_plans_prepare_n(const ww_augment_plan* plans_host, int64_t n_clips, int64_t n_samples, void* records_host) {
    if (int rc = check_aug_sizes(n_clips, n_samples)) return rc;
    if (n_clips == 0) return WW_OK;
    if (!plans_host || !records_host) return fail(WW_EINVAL, "null plan / record pointer");
    return augment_prepare(plans_host, nullptr, nullptr, n_clips, n_samples, 0, 0, 0, records_host, nullptr);
}

int ww_augment_records_n_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const void* records_dev,
                             float* out_dev, int64_t out_stride, void* workspace_dev, ww_stream_t stream) {
    return augment_records({pcm_dev, n_clips, clip_stride, n_samples, out_dev, out_stride, workspace_dev, static_cast<hipStream_t>(stream)},
                           records_dev, 0);
}

// ---- background noise (the augmentation lengths above; the standalone mix at every inference length) ----
static int check_bg_args(int64_t n_clips, const ww_augment_bg* bg_host, const float* bank_dev, int64_t bank_len) {
    if (n_clips == 0) return WW_OK;
    if (!bg_host) return fail(WW_EINVAL, "null bg pointer");
    if (bank_len < 0) return fail(WW_EINVAL, "bank_len %lld < 0", (long long)bank_len);
    bool any = false;
    for (int64_t c = 0; c < n_clips && !any; ++c) any = bg_host[c].enabled != 0;
    if (any && !bank_dev) return fail(WW_EINVAL, "null bank pointer");
    return WW_OK;
}

int64_t ww_augment_bg_workspace_bytes(int64_t n_clips, int64_t n_samples) {
    if (int rc = check_aug_sizes(n_clips, n_samples)) return rc;
    return augment_workspace_bytes(n_clips, n_samples, kAugBg);
}

int ww_augment_bg_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_plan* plans_host,
                      const ww_augment_bg* bg_host, const float* bank_dev, int64_t bank_len, float* out_dev, int64_t out_stride,
                      void* workspace_dev, ww_stream_t stream) {
    const AugCall c = {pcm_dev, n_clips, clip_stride, n_samples, out_dev, out_stride, workspace_dev, static_cast<hipStream_t>(stream), bank_dev,
                       bank_len};
    if (int rc = check_rows(kAugRows, c, plans_host != nullptr)) return rc;
    if (n_clips == 0) return WW_OK;
    if (int rc = check_bg_args(n_clips, bg_host, bank_dev, bank_len)) return rc;
    return augment_direct(c, kAugBg, plans_host, bg_host, nullptr);
}

int64_t ww_augment_bg_record_bytes(void) { return augment_record_bytes(kAugBg); }

int ww_augment_bg_prepare(const ww_augment_plan* plans_host, const ww_augment_bg* bg_host, int64_t n_clips, int64_t n_samples,
                          int64_t bank_len, void* records_host) {
    if (int rc = check_aug_sizes(n_clips, n_samples)) return rc;
    if (n_clips == 0) return WW_OK;
    if (!plans_host || !bg_host || !records_host) return fail(WW_EINVAL, "null plan / bg / record pointer");
    if (bank_len < 0) return fail(WW_EINVAL, "bank_len %lld < 0", (long long)bank_len);
    return augment_prepare(plans_host, bg_host, nullptr, n_clips, n_samples, bank_len, 0, kAugBg, records_host, nullptr);
}

int ww_augment_bg_records_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const void* records_dev,
                              const float* bank_dev, int64_t bank_len, float* out_dev, int64_t out_stride, void* workspace_dev,
                              ww_stream_t stream) {
    return augment_records({pcm_dev, n_clips, clip_stride, n_samples, out_dev, out_stride, workspace_dev, static_cast<hipStream_t>(stream), bank_dev,
                            bank_len},
                           records_dev, kAugBg);
}

int64_t ww_mix_background_workspace_bytes(int64_t n_clips) {
    if (int rc = check_n_clips(n_clips)) return rc;
    return mix_background_workspace_bytes(n_clips);
}

int ww_mix_background_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_bg* bg_host,
                          const float* bank_dev, int64_t bank_len, float* out_dev, int64_t out_stride, void* workspace_dev,
                          ww_stream_t stream) {
    const AugCall c = {pcm_dev, n_clips, clip_stride, n_samples, out_dev, out_stride, workspace_dev, static_cast<hipStream_t>(stream), bank_dev,
                       bank_len};
    if (int rc = check_rows(kMixRows, c)) return rc;
    if (n_clips == 0) return WW_OK;
    if (int rc = check_bg_args(n_clips, bg_host, bank_dev, bank_len)) return rc;
    std::vector<char> rec(size_t(mix_background_workspace_bytes(n_clips)));
    if (int rc = background_prepare(bg_host, n_clips, bank_len, rec.data(), nullptr)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_mix_background(c, rec.data());
}

// ---- reverberation (the augmentation lengths above; the standalone reverb at every inference length) ----
static int check_rir_args(int64_t n_clips, const ww_augment_rir* rir_host, const float* spectra_dev, int64_t n_rirs) {
    if (n_clips == 0) return WW_OK;
    if (!rir_host) return fail(WW_EINVAL, "null rir pointer");
    if (n_rirs < 0) return fail(WW_EINVAL, "n_rirs %lld < 0", (long long)n_rirs);
    bool any = false;
    for (int64_t c = 0; c < n_clips && !any; ++c) any = rir_host[c].enabled != 0;
    if (any && !spectra_dev) return fail(WW_EINVAL, "null spectra pointer");
    if (reinterpret_cast<uintptr_t>(spectra_dev) & 7) return fail(WW_EINVAL, "spectra_dev must be 8-byte aligned");
    return WW_OK;
}

int64_t ww_rir_spectra_workspace_bytes(int64_t n_rirs) {
    if (n_rirs < 0 || n_rirs > (int64_t(1) << 24)) return fail(WW_EINVAL, "n_rirs %lld out of range", (long long)n_rirs);
    return rir_spectra_workspace_bytes(n_rirs);
}

int ww_rir_spectra_f32(const float* taps_dev, int64_t taps_len, const int64_t* offsets_host, const int32_t* lengths_host, int64_t n_rirs,
                       float* spectra_dev, void* workspace_dev, ww_stream_t stream) {
    if (n_rirs < 0 || n_rirs > (int64_t(1) << 24)) return fail(WW_EINVAL, "n_rirs %lld out of range", (long long)n_rirs);
    if (n_rirs == 0) return WW_OK;
    if (!taps_dev || !offsets_host || !lengths_host || !spectra_dev || !workspace_dev)
        return fail(WW_EINVAL, "null taps / offsets / lengths / spectra / workspace pointer");
    if ((reinterpret_cast<uintptr_t>(taps_dev) & 3) || (reinterpret_cast<uintptr_t>(spectra_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(workspace_dev) & 255))
        return fail(WW_EINVAL, "taps_dev must be 4-byte, spectra_dev 8-byte and workspace_dev 256-byte aligned");
    if (taps_len < 0) return fail(WW_EINVAL, "taps_len %lld < 0", (long long)taps_len);
    for (int64_t r = 0; r < n_rirs; ++r)      // every refusal before anything is launched (the launcher checks the same again)
        if (lengths_host[r] < 1 || lengths_host[r] > WW_RIR_MAX_TAPS || offsets_host[r] < 0 || offsets_host[r] > taps_len - lengths_host[r])
            return fail(WW_EINVAL, "rir %lld: taps [%lld, +%d) outside the buffer of %lld or not 1..%d", (long long)r, (long long)offsets_host[r],
                        lengths_host[r], (long long)taps_len, WW_RIR_MAX_TAPS);
    if (int rc = require_gfx950()) return rc;
    return launch_rir_spectra(taps_dev, taps_len, offsets_host, lengths_host, n_rirs, spectra_dev, workspace_dev,
                              static_cast<hipStream_t>(stream));
}

int64_t ww_augment_rir_workspace_bytes(int64_t n_clips, int64_t n_samples) {
    if (int rc = check_aug_sizes(n_clips, n_samples)) return rc;
    return augment_workspace_bytes(n_clips, n_samples, kAugBg | kAugRir);
}

int ww_augment_rir_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_plan* plans_host,
                       const ww_augment_bg* bg_host, const float* bank_dev, int64_t bank_len, const ww_augment_rir* rir_host,
                       const float* spectra_dev, int64_t n_rirs, float* out_dev, int64_t out_stride, void* workspace_dev,
                       ww_stream_t stream) {
    const AugCall c = {pcm_dev, n_clips, clip_stride, n_samples, out_dev, out_stride, workspace_dev, static_cast<hipStream_t>(stream), bank_dev,
                       bank_len, spectra_dev, n_rirs};
    if (int rc = check_rows(kAugRows, c, plans_host != nullptr)) return rc;
    if (n_clips == 0) return WW_OK;
    if (bg_host)
        if (int rc = check_bg_args(n_clips, bg_host, bank_dev, bank_len)) return rc;
    if (int rc = check_rir_args(n_clips, rir_host, spectra_dev, n_rirs)) return rc;
    return augment_direct(c, kAugBg | kAugRir, plans_host, bg_host, rir_host);
}

int64_t ww_augment_rir_record_bytes(void) { return augment_record_bytes(kAugBg | kAugRir); }

int ww_augment_rir_prepare(const ww_augment_plan* plans_host, const ww_augment_bg* bg_host, const ww_augment_rir* rir_host, int64_t n_clips,
                           int64_t n_samples, int64_t bank_len, int64_t n_rirs, void* records_host) {
    if (int rc = check_aug_sizes(n_clips, n_samples)) return rc;
    if (n_clips == 0) return WW_OK;
    if (!plans_host || !rir_host || !records_host) return fail(WW_EINVAL, "null plan / rir / record pointer");
    if (bank_len < 0 || n_rirs < 0) return fail(WW_EINVAL, "bank_len %lld / n_rirs %lld < 0", (long long)bank_len, (long long)n_rirs);
    return augment_prepare(plans_host, bg_host, rir_host, n_clips, n_samples, bank_len, n_rirs, kAugBg | kAugRir, records_host, nullptr);
}

int ww_augment_rir_records_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const void* records_dev,
                               const float* bank_dev, int64_t bank_len, const float* spectra_dev, int64_t n_rirs, float* out_dev,
                               int64_t out_stride, void* workspace_dev, ww_stream_t stream) {
    return augment_records({pcm_dev, n_clips, clip_stride, n_samples, out_dev, out_stride, workspace_dev, static_cast<hipStream_t>(stream), bank_dev,
                            bank_len, spectra_dev, n_rirs},
                           records_dev, kAugBg | kAugRir);
}

int64_t ww_reverb_workspace_bytes(int64_t n_clips) {
    if (int rc = check_n_clips(n_clips)) return rc;
    return reverb_workspace_bytes(n_clips);
}

int ww_reverb_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_rir* rir_host,
                  const float* spectra_dev, int64_t n_rirs, float* out_dev, int64_t out_stride, void* workspace_dev, ww_stream_t stream) {
    const AugCall c = {pcm_dev, n_clips, clip_stride, n_samples, out_dev, out_stride, workspace_dev, static_cast<hipStream_t>(stream), nullptr, 0,
                       spectra_dev, n_rirs};
    if (int rc = check_rows(kReverbRows, c)) return rc;
    if (n_clips == 0) return WW_OK;
    if (int rc = check_rir_args(n_clips, rir_host, spectra_dev, n_rirs)) return rc;
    std::vector<char> rec(size_t(reverb_workspace_bytes(n_clips)));
    if (int rc = rir_prepare(rir_host, n_clips, n_rirs, rec.data(), nullptr)) return rc;
    if (int rc = require_gfx950()) return rc;
    return launch_reverb(c, rec.data());
}

// SpecAugment: what the draw and the masking call share, all of it before any HIP call
static int check_spec(int64_t n, int32_t width, float prob, int32_t n_freq, int32_t freq_max, int32_t n_time, int32_t time_max) {
    if (width < 1 || width > WW_MAX_FRAMES) return fail(WW_EUNSUPPORTED, "width %d: mel images of 1..%d frames", width, WW_MAX_FRAMES);
    if (n < 0 || n > (int64_t(1) << 30)) return fail(WW_EINVAL, "n %lld out of range", (long long)n);
    if (!(prob >= 0.f && prob <= 1.f)) return fail(WW_EINVAL, "prob %g outside [0, 1]", double(prob));
    if (n_freq < 0 || n_freq > WW_SPEC_MAX_MASKS || n_time < 0 || n_time > WW_SPEC_MAX_MASKS)
        return fail(WW_EINVAL, "n_freq %d / n_time %d: 0..%d masks per axis", n_freq, n_time, WW_SPEC_MAX_MASKS);
    if (freq_max < 0 || freq_max > WW_N_MELS) return fail(WW_EINVAL, "freq_max %d outside 0..%d", freq_max, WW_N_MELS);
    if (time_max < 0 || time_max > width) return fail(WW_EINVAL, "time_max %d outside 0..width = %d", time_max, width);
    return WW_OK;
}

int64_t ww_spec_augment_record_bytes(void) { return WW_SPEC_RECORD_INT16 * int64_t(sizeof(int16_t)); }

int ww_spec_augment_draw(uint64_t seed, int64_t n, int32_t width, float prob, int32_t n_freq, int32_t freq_max, int32_t n_time,
                         int32_t time_max, int16_t* records_dev, ww_stream_t stream) {
    if (int rc = check_spec(n, width, prob, n_freq, freq_max, n_time, time_max)) return rc;
    if (n == 0) return WW_OK;
    if (!records_dev) return fail(WW_EINVAL, "null records pointer");
    if (reinterpret_cast<uintptr_t>(records_dev) & 15) return fail(WW_EINVAL, "records_dev must be 16-byte aligned");
    if (int rc = require_gfx950()) return rc;
    const SpecDraw d = {seed, prob, n_freq, freq_max, n_time, time_max};
    return launch_spec_draw(d, n, width, records_dev, static_cast<hipStream_t>(stream));
}

int ww_spec_augment_f32(const float* mel_in, float* mel_out, int64_t n, int32_t width, const int16_t* records_dev, uint64_t seed, float prob,
                        int32_t n_freq, int32_t freq_max, int32_t n_time, int32_t time_max, int32_t fill_mode, float fill_value,
                        ww_stream_t stream) {
    if (int rc = check_spec(n, width, prob, n_freq, freq_max, n_time, time_max)) return rc;
    if (fill_mode != WW_SPEC_FILL_MEAN && fill_mode != WW_SPEC_FILL_MIN && fill_mode != WW_SPEC_FILL_VALUE)
        return fail(WW_EINVAL, "unknown fill mode %d", fill_mode);
    if (n == 0) return WW_OK;
    if (!mel_in || !mel_out) return fail(WW_EINVAL, "null mel pointer");
    const uintptr_t a = reinterpret_cast<uintptr_t>(mel_in), b = reinterpret_cast<uintptr_t>(mel_out);
    if ((a & 15) || (b & 15) || (reinterpret_cast<uintptr_t>(records_dev) & 15))
        return fail(WW_EINVAL, "mel_in, mel_out and records_dev must be 16-byte aligned");
    const uintptr_t bytes = uintptr_t(n) * WW_N_MELS * uintptr_t(width) * sizeof(float);
    if (a != b && a < b + bytes && b < a + bytes) return fail(WW_EINVAL, "mel_in and mel_out overlap partially: pass the same buffer or disjoint ones");
    if (int rc = require_gfx950()) return rc;
    const SpecDraw d = {seed, prob, n_freq, freq_max, n_time, time_max};
    return launch_spec_augment(mel_in, mel_out, n, width, records_dev, d, fill_mode, fill_value, static_cast<hipStream_t>(stream));
}

// Microphone-channel augmentation: what the draw and the filter call share, all of it before any HIP call
static int check_channel_config(const ww_channel_config* g) {
    if (!g) return fail(WW_EINVAL, "null config pointer");
    const float probs[] = {g->prob, g->highpass_prob, g->low_shelf_prob, g->high_shelf_prob, g->peak_prob, g->lowpass_prob, g->drive_prob};
    for (float p : probs)
        if (!(p >= 0.f && p <= 1.f)) return fail(WW_EINVAL, "probability %g outside [0, 1]", double(p));
    const float hz[][2] = {{g->highpass_lo, g->highpass_hi}, {g->low_shelf_lo, g->low_shelf_hi}, {g->high_shelf_lo, g->high_shelf_hi},
                           {g->peak_lo, g->peak_hi}, {g->lowpass_lo, g->lowpass_hi}};
    for (const auto& r : hz)
        if (!(r[0] > 0.f && r[0] <= r[1] && r[1] <= 7600.f))
            return fail(WW_EINVAL, "frequency range (%g, %g): expected 0 < lo <= hi <= 7600 Hz", double(r[0]), double(r[1]));
    if (!(g->peak_q_lo > 0.f && g->peak_q_lo <= g->peak_q_hi && g->peak_q_hi <= 1e6f))
        return fail(WW_EINVAL, "Q range (%g, %g): expected 0 < lo <= hi", double(g->peak_q_lo), double(g->peak_q_hi));
    if (!(g->shelf_db >= 0.f && g->shelf_db <= 40.f && g->peak_db >= 0.f && g->peak_db <= 40.f))
        return fail(WW_EINVAL, "shelf_db %g / peak_db %g outside [0, 40]", double(g->shelf_db), double(g->peak_db));
    if (g->peaks < 0 || g->peaks > WW_CHANNEL_MAX_PEAKS) return fail(WW_EINVAL, "peaks %d outside 0..%d", g->peaks, WW_CHANNEL_MAX_PEAKS);
    if (!(g->drive_lo >= 0.f && g->drive_lo <= g->drive_hi && g->drive_hi <= 8.f))
        return fail(WW_EINVAL, "drive range (%g, %g): expected 0 <= lo <= hi <= 8", double(g->drive_lo), double(g->drive_hi));
    return WW_OK;
}

int64_t ww_channel_record_bytes(void) { return WW_CHANNEL_RECORD_F32 * int64_t(sizeof(float)); }

int ww_channel_draw(uint64_t seed, int64_t n, const ww_channel_config* cfg, float* records_dev, ww_stream_t stream) {
    if (n < 0 || n > (int64_t(1) << 30)) return fail(WW_EINVAL, "n %lld out of range", (long long)n);
    if (int rc = check_channel_config(cfg)) return rc;
    if (n == 0) return WW_OK;
    if (!records_dev) return fail(WW_EINVAL, "null records pointer");
    if (reinterpret_cast<uintptr_t>(records_dev) & 15) return fail(WW_EINVAL, "records_dev must be 16-byte aligned");
    if (int rc = require_gfx950()) return rc;
    return launch_channel_draw(*cfg, seed, n, records_dev, static_cast<hipStream_t>(stream));
}

int ww_channel_f32(const float* pcm_in, float* pcm_out, int64_t n, int64_t n_samples, int64_t row_stride, const float* records_dev,
                   uint64_t seed, const ww_channel_config* cfg, ww_stream_t stream) {
    if (n_samples < WW_MIN_CLIP_SAMPLES || n_samples > WW_AUG_MAX_SAMPLES)
        return fail(WW_EUNSUPPORTED, "n_samples %lld: the channel stage takes clips of %d..%d samples", (long long)n_samples, WW_MIN_CLIP_SAMPLES,
                    WW_AUG_MAX_SAMPLES);
    if (n < 0 || n > (int64_t(1) << 30)) return fail(WW_EINVAL, "n %lld out of range", (long long)n);
    if (!records_dev || cfg)
        if (int rc = check_channel_config(cfg)) return rc;
    if (n == 0) return WW_OK;
    if (!pcm_in || !pcm_out) return fail(WW_EINVAL, "null pcm pointer");
    if (row_stride < n_samples || row_stride > (int64_t(1) << 31)) return fail(WW_EINVAL, "row_stride %lld < n_samples %lld", (long long)row_stride, (long long)n_samples);
    const uintptr_t a = reinterpret_cast<uintptr_t>(pcm_in), b = reinterpret_cast<uintptr_t>(pcm_out);
    if ((a & 3) || (b & 3) || (reinterpret_cast<uintptr_t>(records_dev) & 15))
        return fail(WW_EINVAL, "pcm_in and pcm_out must be 4-byte and records_dev 16-byte aligned");
    const uintptr_t bytes = (uintptr_t(n - 1) * uintptr_t(row_stride) + uintptr_t(n_samples)) * sizeof(float);
    if (a != b && a < b + bytes && b < a + bytes) return fail(WW_EINVAL, "pcm_in and pcm_out overlap partially: pass the same buffer or disjoint ones");
    if (int rc = require_gfx950()) return rc;
    static const ww_channel_config none = {};
    return launch_channel(pcm_in, pcm_out, n, int(n_samples), row_stride, records_dev, seed, cfg ? *cfg : none, static_cast<hipStream_t>(stream));
}

int64_t ww_cnn_scratch_bytes(int64_t n, int32_t n_conv) { return cnn_scratch_bytes(n, n_conv); }

int ww_cnn_pool_f32(const float* mel_dev, int64_t n, int32_t width, const float* packed_dev, int32_t n_conv,
                    void* scratch_dev, float* pooled_dev, ww_stream_t stream) {
    if (int rc = check_model(n, width, packed_dev, n_conv)) return rc;
    if (n > 0 && (!mel_dev || !pooled_dev)) return fail(WW_EINVAL, "null tensor pointer");
    if (int rc = require_gfx950()) return rc;
    return launch_cnn_pool(mel_dev, n, width, packed_dev, n_conv, scratch_dev, pooled_dev, static_cast<hipStream_t>(stream));
}

int ww_lstm_fc_f32(const float* pooled_dev, int64_t n, const float* packed_dev, int32_t n_conv, float* logits_dev,
                   ww_stream_t stream) {
    if (int rc = check_model(n, 1, packed_dev, n_conv)) return rc;
    if (n > 0 && (!pooled_dev || !logits_dev)) return fail(WW_EINVAL, "null tensor pointer");
    if (int rc = require_gfx950()) return rc;
    return launch_lstm_fc(pooled_dev, n, packed_dev, n_conv, logits_dev, nullptr, static_cast<hipStream_t>(stream));
}

int64_t ww_workspace_bytes(int64_t n, int32_t n_conv) {
    if (n < 0 || (n_conv != 2 && n_conv != 3)) return fail(WW_EINVAL, "bad workspace query");
    return forward_workspace(nullptr, n, kFrames, n_conv).total;
}

int ww_model_forward_f32(const float* mel_dev, int64_t n, int32_t width, const float* packed_dev, int32_t n_conv,
                         void* workspace_dev, float* logits_dev, ww_stream_t stream) {
    if (int rc = check_model(n, width, packed_dev, n_conv)) return rc;
    if (n == 0) return WW_OK;
    if (!mel_dev || !logits_dev || !workspace_dev) return fail(WW_EINVAL, "null tensor / workspace pointer");
    if (int rc = require_gfx950()) return rc;
    // the workspace of ww_workspace_bytes(): laid out for kFrames whatever the width
    return model_chain(mel_dev, n, width, packed_dev, n_conv, forward_workspace(workspace_dev, n, kFrames, n_conv), logits_dev, nullptr,
                       static_cast<hipStream_t>(stream));
}

int ww_forward_pcm_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t clip_len, int normalize,
                       const float* packed_dev, int32_t n_conv, void* workspace_dev, float* logits_dev,
                       ww_stream_t stream) {
    if (int rc = check_rows(kClipRows, {pcm_dev, n_clips, clip_stride, clip_len})) return rc;
    if (int rc = check_model(n_clips, kFrames, packed_dev, n_conv)) return rc;
    if (n_clips == 0) return WW_OK;
    if (!logits_dev || !workspace_dev) return fail(WW_EINVAL, "null logits / workspace pointer");
    if (int rc = require_gfx950()) return rc;
    return forward_chain(pcm_dev, n_clips, clip_stride, clip_len, kClip, normalize, nullptr, 0, packed_dev, n_conv,
                         forward_workspace(workspace_dev, n_clips, kFrames, n_conv), logits_dev, nullptr, static_cast<hipStream_t>(stream));
}

// ---- any clip length in [0.25 s, 2 s] (the 1 s entry points above are unchanged) ----
static int check_samples(int64_t clip_len, int64_t n_samples) {
    if (n_samples < WW_MIN_CLIP_SAMPLES || n_samples > WW_MAX_CLIP_SAMPLES)
        return fail(WW_EINVAL, "n_samples %lld: expected %d..%d (0.25 s .. 2 s at 16 kHz)", (long long)n_samples, WW_MIN_CLIP_SAMPLES,
                    WW_MAX_CLIP_SAMPLES);
    if (clip_len > n_samples) return fail(WW_EINVAL, "clip_len %lld > n_samples %lld", (long long)clip_len, (long long)n_samples);
    return WW_OK;
}
static int check_wide(int64_t n, int32_t width, const float* packed, int32_t n_conv) {
    if (width < 1 || width > WW_MAX_FRAMES) return fail(WW_EINVAL, "mel width %d: the wide conv stack takes 1..%d frames", width, WW_MAX_FRAMES);
    if (n > (int64_t(1) << 24)) return fail(WW_EINVAL, "batch %lld out of range", (long long)n);
    return check_model(n, width <= WW_MAX_WIDTH ? width : 1, packed, n_conv);
}

int ww_logmel_frames_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t clip_len, int64_t n_samples, int normalize,
                         float* logmel_dev, ww_stream_t stream) {
    if (int rc = check_samples(clip_len, n_samples)) return rc;
    if (int rc = check_rows(kFrameRows, {pcm_dev, n_clips, clip_stride, clip_len}, logmel_dev != nullptr)) return rc;
    if (n_clips == 0) return WW_OK;
    if (int rc = require_gfx950()) return rc;
    return launch_logmel_frames(pcm_dev, n_clips, clip_stride, clip_len, n_samples, normalize, logmel_dev, static_cast<hipStream_t>(stream));
}

int64_t ww_cnn_wide_scratch_bytes(int64_t n, int32_t width, int32_t n_conv) {
    if (n < 0 || width < 1 || width > WW_MAX_FRAMES || (n_conv != 2 && n_conv != 3)) return fail(WW_EINVAL, "bad wide scratch query");
    return wide_scratch_bytes(n, width, n_conv);
}

int ww_cnn_pool_wide_f32(const float* mel_dev, int64_t n, int32_t width, const float* packed_dev, int32_t n_conv, void* scratch_dev,
                         float* pooled_dev, ww_stream_t stream) {
    if (int rc = check_wide(n, width, packed_dev, n_conv)) return rc;
    if (n == 0) return WW_OK;
    if (!mel_dev || !pooled_dev) return fail(WW_EINVAL, "null tensor pointer");
    if (width > WW_MAX_WIDTH && (!scratch_dev || (reinterpret_cast<uintptr_t>(scratch_dev) & 255)))
        return fail(WW_EINVAL, "widths > %d need ww_cnn_wide_scratch_bytes() of 256-byte aligned scratch", WW_MAX_WIDTH);
    if (int rc = require_gfx950()) return rc;
    return cnn_pool_any(mel_dev, n, width, packed_dev, n_conv, scratch_dev, pooled_dev, static_cast<hipStream_t>(stream));
}

int64_t ww_workspace_frames_bytes(int64_t n, int64_t n_samples, int32_t n_conv) {
    if (n < 0 || (n_conv != 2 && n_conv != 3) || n_samples < WW_MIN_CLIP_SAMPLES || n_samples > WW_MAX_CLIP_SAMPLES)
        return fail(WW_EINVAL, "bad workspace query");
    return forward_workspace(nullptr, n, frames_of(n_samples), n_conv).total;
}

int ww_forward_pcm_frames_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t clip_len, int64_t n_samples, int normalize,
                              const float* packed_dev, int32_t n_conv, void* workspace_dev, float* logits_dev, ww_stream_t stream) {
    if (int rc = check_samples(clip_len, n_samples)) return rc;
    const int T = frames_of(n_samples);
    if (int rc = check_wide(n_clips, T, packed_dev, n_conv)) return rc;
    if (n_clips == 0) return WW_OK;
    if (!logits_dev || !workspace_dev || (reinterpret_cast<uintptr_t>(workspace_dev) & 255))
        return fail(WW_EINVAL, "null logits pointer, or workspace not a 256-byte aligned pointer");
    if (int rc = check_rows(kFrameRows, {pcm_dev, n_clips, clip_stride, clip_len})) return rc;
    if (int rc = require_gfx950()) return rc;
    return forward_chain(pcm_dev, n_clips, clip_stride, clip_len, n_samples, normalize, nullptr, 0, packed_dev, n_conv,
                         forward_workspace(workspace_dev, n_clips, T, n_conv), logits_dev, nullptr, static_cast<hipStream_t>(stream));
}

// ---- long recordings: overlapping windows of one signal, and events over their scores ----
// The log-mel kernels (logmel_kernel, logmel64_kernel in all three arithmetics) only read the input, each clip through a buffer
// descriptor of its own at pcm + c * clip_stride; every write goes to the workspace, indexed by clip.  So rows may overlap here, and
// the chain is the one ww_forward_pcm_frames_f32 runs (at N = 16000 the 1 s kernels, as ww_forward_pcm_f32 does).
int64_t ww_forward_windows_workspace_bytes(int64_t n_windows, int64_t n_samples, int32_t n_conv) {
    if (n_windows < 0 || n_windows > (int64_t(1) << 24)) return fail(WW_EINVAL, "n_windows %lld out of range", (long long)n_windows);
    if (n_conv != 2 && n_conv != 3) return fail(WW_EINVAL, "n_conv must be 2 or 3, got %d", n_conv);
    if (n_samples != kClip && (n_samples < WW_MIN_CLIP_SAMPLES || n_samples > WW_MAX_CLIP_SAMPLES))
        return fail(WW_EINVAL, "n_samples %lld: expected %d..%d", (long long)n_samples, WW_MIN_CLIP_SAMPLES, WW_MAX_CLIP_SAMPLES);
    return forward_workspace(nullptr, n_windows, frames_of(n_samples), n_conv).total;
}

int ww_forward_windows_f32(const float* signal_dev, int64_t n_windows, int64_t hop, int64_t n_samples, int normalize,
                           const float* packed_dev, int32_t n_conv, void* workspace_dev, int64_t workspace_bytes, float* logits_dev,
                           float* prob_dev, ww_stream_t stream) {
    if (n_windows < 0 || n_windows > (int64_t(1) << 24)) return fail(WW_EINVAL, "n_windows %lld: expected 0..%d", (long long)n_windows, 1 << 24);
    if (n_samples < WW_MIN_CLIP_SAMPLES || n_samples > WW_MAX_CLIP_SAMPLES)
        return fail(WW_EINVAL, "n_samples %lld: expected %d..%d (0.25 s .. 2 s at 16 kHz)", (long long)n_samples, WW_MIN_CLIP_SAMPLES,
                    WW_MAX_CLIP_SAMPLES);
    if (hop < 4 || hop > n_samples || (hop & 3))
        return fail(WW_EINVAL, "hop %lld: expected a multiple of 4 in 4..n_samples (%lld)", (long long)hop, (long long)n_samples);
    if (n_conv != 2 && n_conv != 3) return fail(WW_EINVAL, "n_conv must be 2 or 3, got %d", n_conv);
    if (n_windows == 0) return WW_OK;
    if (!signal_dev || (reinterpret_cast<uintptr_t>(signal_dev) & 15)) return fail(WW_EINVAL, "signal_dev must be a 16-byte aligned device pointer");
    if (!packed_dev || (reinterpret_cast<uintptr_t>(packed_dev) & 15)) return fail(WW_EINVAL, "packed_dev must be a 16-byte aligned device pointer");
    if (!logits_dev) return fail(WW_EINVAL, "logits_dev is null");
    if (!workspace_dev || (reinterpret_cast<uintptr_t>(workspace_dev) & 255)) return fail(WW_EINVAL, "workspace_dev must be 256-byte aligned");
    const ForwardWorkspace w = forward_workspace(workspace_dev, n_windows, frames_of(n_samples), n_conv);
    if (workspace_bytes < w.total)
        return fail(WW_EINVAL, "workspace_bytes %lld < %lld needed", (long long)workspace_bytes, (long long)w.total);
    if (int rc = require_gfx950()) return rc;
    return forward_chain(signal_dev, n_windows, hop, n_samples, n_samples, normalize, nullptr, 0, packed_dev, n_conv, w, logits_dev, prob_dev,
                         static_cast<hipStream_t>(stream));
}

int64_t ww_events_workspace_bytes(int64_t n_windows) {
    if (n_windows < 0 || n_windows > (int64_t(1) << 40)) return fail(WW_EINVAL, "n_windows %lld out of range", (long long)n_windows);
    return up256(n_windows * int64_t(sizeof(double)));
}

int ww_events_sweep_f32(const float* prob_dev, const int64_t* seg_offsets_dev, int64_t n_segs, int64_t n_windows, int32_t smooth,
                        int64_t refractory, const float* thresholds_dev, int32_t n_thr, int64_t* counts_dev, uint8_t* fired_dev,
                        void* workspace_dev, int64_t workspace_bytes, ww_stream_t stream) {
    if (n_segs < 0 || n_segs > (int64_t(1) << 30)) return fail(WW_EINVAL, "n_segs %lld out of range", (long long)n_segs);
    if (n_windows < 0 || n_windows > (int64_t(1) << 40)) return fail(WW_EINVAL, "n_windows %lld out of range", (long long)n_windows);
    if (smooth < 1 || smooth > 256) return fail(WW_EINVAL, "smooth %d: expected 1..256 windows", smooth);
    if (refractory < 0 || refractory > (int64_t(1) << 30)) return fail(WW_EINVAL, "refractory %lld: expected 0..2^30 windows", (long long)refractory);
    if (n_thr < 1 || n_thr > 65536) return fail(WW_EINVAL, "n_thr %d: expected 1..65536 thresholds", n_thr);
    if (fired_dev && n_thr != 1) return fail(WW_EINVAL, "fired_dev: per-window flags need exactly one threshold (n_thr %d)", n_thr);
    if (n_segs == 0) return WW_OK;
    if (!seg_offsets_dev || (reinterpret_cast<uintptr_t>(seg_offsets_dev) & 7)) return fail(WW_EINVAL, "seg_offsets_dev must be an 8-byte aligned device pointer");
    if (!thresholds_dev || (reinterpret_cast<uintptr_t>(thresholds_dev) & 3)) return fail(WW_EINVAL, "thresholds_dev must be a 4-byte aligned device pointer");
    if (!counts_dev || (reinterpret_cast<uintptr_t>(counts_dev) & 7)) return fail(WW_EINVAL, "counts_dev must be an 8-byte aligned device pointer");
    if (n_windows > 0 && !prob_dev) return fail(WW_EINVAL, "prob_dev is null");
    if (!workspace_dev || (reinterpret_cast<uintptr_t>(workspace_dev) & 15)) return fail(WW_EINVAL, "workspace_dev must be 16-byte aligned");
    if (workspace_bytes < n_windows * int64_t(sizeof(double)))
        return fail(WW_EINVAL, "workspace_bytes %lld < %lld needed", (long long)workspace_bytes, (long long)(n_windows * int64_t(sizeof(double))));
    if (int rc = require_gfx950()) return rc;
    return launch_events_sweep(prob_dev, seg_offsets_dev, int(n_segs), n_windows, smooth, refractory, thresholds_dev, n_thr, counts_dev,
                               fired_dev, static_cast<double*>(workspace_dev), static_cast<hipStream_t>(stream));
}

int64_t ww_events_state_bytes(int32_t n_mics, int32_t smooth) {
    if (n_mics < 1 || n_mics > (1 << 20)) return fail(WW_EINVAL, "n_mics %d out of range", n_mics);
    if (smooth < 1 || smooth > 256) return fail(WW_EINVAL, "smooth %d: expected 1..256 windows", smooth);
    return 16 * int64_t(n_mics) + up256(int64_t(n_mics) * smooth * int64_t(sizeof(float)));
}

int ww_events_step_f32(const float* prob_dev, int32_t n_mics, int32_t smooth, float threshold, int64_t refractory, void* state_dev,
                       uint8_t* fired_dev, ww_stream_t stream) {
    if (n_mics < 1 || n_mics > (1 << 20)) return fail(WW_EINVAL, "n_mics %d out of range", n_mics);
    if (smooth < 1 || smooth > 256) return fail(WW_EINVAL, "smooth %d: expected 1..256 windows", smooth);
    if (refractory < 0 || refractory > (int64_t(1) << 30)) return fail(WW_EINVAL, "refractory %lld: expected 0..2^30 windows", (long long)refractory);
    if (!(threshold > 0.f && threshold <= 1.f)) return fail(WW_EINVAL, "threshold %g: expected 0 < threshold <= 1", double(threshold));
    if (!prob_dev || (reinterpret_cast<uintptr_t>(prob_dev) & 3)) return fail(WW_EINVAL, "prob_dev must be a 4-byte aligned device pointer");
    if (!state_dev || (reinterpret_cast<uintptr_t>(state_dev) & 15)) return fail(WW_EINVAL, "state_dev must be a 16-byte aligned device pointer");
    if (!fired_dev) return fail(WW_EINVAL, "fired_dev is null");
    if (int rc = require_gfx950()) return rc;
    return launch_events_step(prob_dev, n_mics, smooth, threshold, refractory, state_dev, fired_dev, static_cast<hipStream_t>(stream));
}

static int check_train(const float* mel, int64_t n, int32_t width, const ww_train_params* p, const void* ws) {
    if (n < 1 || n > (int64_t(1) << 24)) return fail(WW_EINVAL, "training batch %lld out of range", (long long)n);
    if (width < 1 || width > WW_MAX_WIDTH) return fail(WW_EUNSUPPORTED, "mel width %d: the conv kernels take 1..%d frames", width, WW_MAX_WIDTH);
    if (!p || !mel || !ws) return fail(WW_EINVAL, "null argument");
    if ((p->n_conv != 2 && p->n_conv != 3) || p->hidden != kHidden) return fail(WW_EUNSUPPORTED, "the training step is built for 2 or 3 convs and hidden 256");
    for (int i = 0; i < p->n_conv; ++i)
        if (!p->conv_weight[i] || !p->conv_bias[i]) return fail(WW_EINVAL, "null parameter pointer");
    for (int i = 0; i < 2; ++i)
        if (!p->lstm_weight_ih[i] || !p->lstm_bias_ih[i] || !p->lstm_bias_hh[i]) return fail(WW_EINVAL, "null parameter pointer");
    if (!p->fc_weight || !p->fc_bias) return fail(WW_EINVAL, "null parameter pointer");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(WW_EINVAL, "workspace must be 256-byte aligned");
    return WW_OK;
}

// WW_TRAIN_MATH_DEFAULT -> the process-wide setting, read ONCE per call (the caller should then hand the resolved value to the other half)
static int resolve_train_math(int32_t mode, int* out) {
    if (mode == WW_TRAIN_MATH_DEFAULT) mode = g_train_math;
    if (mode != WW_TRAIN_MATH_F32 && mode != WW_TRAIN_MATH_F16X3)
        return fail(WW_EINVAL, "train math %d: expected WW_TRAIN_MATH_F32, WW_TRAIN_MATH_F16X3 or WW_TRAIN_MATH_DEFAULT", mode);
    *out = mode;
    return WW_OK;
}

int64_t ww_train_workspace_bytes(int64_t n, int32_t n_conv, int32_t train_math) {
    if (n < 0 || n > (int64_t(1) << 24) || (n_conv != 2 && n_conv != 3)) return fail(WW_EINVAL, "bad training workspace query");
    int mode;
    if (int rc = resolve_train_math(train_math, &mode)) return rc;
    return train_workspace_bytes(n, n_conv, mode);
}

int ww_train_forward_f32(const float* mel_dev, int64_t n, int32_t width, const ww_train_params* params, float p_lstm, float p_fc,
                         uint64_t seed, int32_t train_math, void* workspace_dev, int64_t workspace_bytes, float* logits_dev, ww_stream_t stream) {
    int mode;
    if (int rc = resolve_train_math(train_math, &mode)) return rc;
    if (int rc = check_train(mel_dev, n, width, params, workspace_dev)) return rc;
    if (workspace_bytes < train_workspace_bytes(n, params->n_conv, mode))
        return fail(WW_EINVAL, "training workspace of %lld bytes: %lld clips of the %d-conv model under train math %d need %lld",
                    (long long)workspace_bytes, (long long)n, params->n_conv, mode, (long long)train_workspace_bytes(n, params->n_conv, mode));
    if (!logits_dev) return fail(WW_EINVAL, "null logits pointer");
    if (!(p_lstm >= 0.f && p_lstm < 1.f) || !(p_fc >= 0.f && p_fc < 1.f)) return fail(WW_EINVAL, "drop probabilities must lie in [0, 1)");
    if (int rc = require_gfx950()) return rc;
    return train_forward(mel_dev, n, width, params, p_lstm, p_fc, seed, mode, workspace_dev, workspace_bytes, logits_dev, static_cast<hipStream_t>(stream));
}

int ww_train_masks(const void* workspace_dev, int64_t n, int32_t n_conv, float* mask0_dev, float* mask1_dev, ww_stream_t stream) {
    if (!workspace_dev || !mask0_dev || !mask1_dev || n < 1 || (n_conv != 2 && n_conv != 3)) return fail(WW_EINVAL, "bad argument");
    if (int rc = require_gfx950()) return rc;
    return train_masks(workspace_dev, n, n_conv, mask0_dev, mask1_dev, static_cast<hipStream_t>(stream));
}

int ww_train_packed_image(const void* workspace_dev, int64_t n, int32_t n_conv, float* img_dev, ww_stream_t stream) {
    if (!workspace_dev || !img_dev || n < 1 || (n_conv != 2 && n_conv != 3)) return fail(WW_EINVAL, "ww_train_packed_image: bad arguments");
    return train_packed_image(workspace_dev, n, n_conv, img_dev, static_cast<hipStream_t>(stream));
}

int ww_train_bit_images(const void* workspace_dev, int64_t n, int32_t n_conv, uint8_t* mask_last_dev, uint32_t* sign1_dev, ww_stream_t stream) {
    if (!workspace_dev || !mask_last_dev || !sign1_dev || n < 1 || (n_conv != 2 && n_conv != 3)) return fail(WW_EINVAL, "ww_train_bit_images: bad arguments");
    return train_bit_images(workspace_dev, n, n_conv, mask_last_dev, sign1_dev, static_cast<hipStream_t>(stream));
}

int ww_train_stage(const void* workspace_dev, int64_t n, int32_t n_conv, int32_t train_math, int32_t stage, float* out_dev, int64_t out_floats,
                   ww_stream_t stream) {
    if (!workspace_dev || !out_dev || n < 1 || n > (int64_t(1) << 24) || (n_conv != 2 && n_conv != 3)) return fail(WW_EINVAL, "ww_train_stage: bad arguments");
    int mode;
    if (int rc = resolve_train_math(train_math, &mode)) return rc;
    if (int rc = train_stage_mode_check(workspace_dev, mode)) return rc;
    const int64_t floats = train_stage_floats(n, n_conv, mode, stage);
    if (floats < 0) return fail(WW_EINVAL, "ww_train_stage: unknown stage %d", stage);
    if (floats == 0) return fail(WW_EINVAL, "ww_train_stage: stage %d is not kept by the %d-conv model under train math %d", stage, n_conv, mode);
    if (out_floats != floats) return fail(WW_EINVAL, "ww_train_stage: stage %d holds %lld floats, the output has %lld", stage, (long long)floats, (long long)out_floats);
    if (int rc = require_gfx950()) return rc;
    return train_stage(workspace_dev, n, n_conv, mode, stage, out_dev, static_cast<hipStream_t>(stream));
}

int ww_train_backward_f32(const float* mel_dev, int64_t n, int32_t width, const ww_train_params* params, const float* dlogits_dev,
                          int32_t train_math, void* workspace_dev, int64_t workspace_bytes, const ww_train_grads* grads, ww_stream_t stream) {
    int mode;
    if (int rc = resolve_train_math(train_math, &mode)) return rc;
    if (int rc = check_train(mel_dev, n, width, params, workspace_dev)) return rc;
    if (workspace_bytes < train_workspace_bytes(n, params->n_conv, mode))
        return fail(WW_EINVAL, "training workspace of %lld bytes: %lld clips of the %d-conv model under train math %d need %lld",
                    (long long)workspace_bytes, (long long)n, params->n_conv, mode, (long long)train_workspace_bytes(n, params->n_conv, mode));
    if (!dlogits_dev || !grads) return fail(WW_EINVAL, "null argument");
    for (int i = 0; i < params->n_conv; ++i)
        if (!grads->conv_weight[i] || !grads->conv_bias[i]) return fail(WW_EINVAL, "null gradient pointer");
    for (int i = 0; i < 2; ++i)
        if (!grads->lstm_weight_ih[i] || !grads->lstm_bias[i]) return fail(WW_EINVAL, "null gradient pointer");
    if (!grads->fc_weight || !grads->fc_bias) return fail(WW_EINVAL, "null gradient pointer");
    if (int rc = require_gfx950()) return rc;
    return train_backward(mel_dev, n, width, params, dlogits_dev, mode, workspace_dev, workspace_bytes, grads, static_cast<hipStream_t>(stream));
}

// in: nullptr for float32 16 kHz mono hops (ww_streamer_create_n), else the checked input format
static int streamer_create(int32_t n_mics, int32_t hop_samples, int32_t n_samples, const StreamInput* in, const float* packed_dev,
                           int32_t n_conv, ww_stream_t stream, ww_streamer** out) {
    const int N = n_samples;
    const int T = frames_of(N);
    if (int rc = check_model(n_mics, T, packed_dev, n_conv)) return rc;
    if (!device_tables()) return WW_EHIP;   // also the gfx950 check; must precede graph capture
    ww_streamer* s = new (std::nothrow) ww_streamer();
    if (!s) return fail(WW_EHIP, "out of host memory");
    s->n_mics = n_mics; s->hop = hop_samples; s->n_conv = n_conv; s->packed = packed_dev;
    s->n_samples = N; s->n_frames = T;
    s->stream = static_cast<hipStream_t>(stream);
    if (in) { s->input = true; s->in = *in; }
    const int64_t ws = forward_workspace(nullptr, n_mics, T, n_conv).total;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->ring), sizeof(float) * int64_t(n_mics) * N);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->pos), 16);
    if (e == hipSuccess) e = hipMalloc(&s->workspace, size_t(ws));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->own_logits), sizeof(float) * 2 * n_mics);
    if (e == hipSuccess) e = hipMemsetAsync(s->ring, 0, sizeof(float) * int64_t(n_mics) * N, s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->pos, 0, 16, s->stream);
    if (e != hipSuccess) {
        ww_streamer_destroy(s);
        return fail(WW_EHIP, "streamer allocation failed: %s", hipGetErrorString(e));
    }
    if (in) {
        if (int rc = stream_input_alloc(&s->in, n_mics, s->stream)) {
            ww_streamer_destroy(s);
            return rc;
        }
    }
    *out = s;
    return WW_OK;
}

static int check_streamer_window(int32_t n_mics, int32_t n_samples) {
    if (n_mics < 1 || n_mics > (1 << 20)) return fail(WW_EINVAL, "n_mics %d out of range", n_mics);
    const int N = n_samples;
    if (N != kClip && (N < WW_MIN_CLIP_SAMPLES || N > WW_AUG_MAX_SAMPLES))
        return fail(WW_EUNSUPPORTED, "n_samples %d: streaming windows take %d..%d samples (0.25 .. 1 s, at most 32 frames) or %d", N,
                    WW_MIN_CLIP_SAMPLES, WW_AUG_MAX_SAMPLES, kClip);
    return WW_OK;
}

int ww_streamer_create_n(int32_t n_mics, int32_t hop_samples, int32_t n_samples, const float* packed_dev, int32_t n_conv,
                         ww_stream_t stream, ww_streamer** out) {
    if (!out) return fail(WW_EINVAL, "null out pointer");
    *out = nullptr;
    if (int rc = check_streamer_window(n_mics, n_samples)) return rc;
    const int N = n_samples;
    if (hop_samples < 4 || hop_samples > N || (hop_samples & 3) || (N % hop_samples))
        return fail(WW_EINVAL, "hop_samples %d: must be a multiple of 4 that divides %d", hop_samples, N);
    return streamer_create(n_mics, hop_samples, n_samples, nullptr, packed_dev, n_conv, stream, out);
}

int ww_streamer_create_input(int32_t n_mics, int32_t hop_frames, int32_t sample_rate, int32_t format, int32_t channels, int32_t n_samples,
                             const float* packed_dev, int32_t n_conv, ww_stream_t stream, ww_streamer** out) {
    if (!out) return fail(WW_EINVAL, "null out pointer");
    *out = nullptr;
    if (int rc = check_streamer_window(n_mics, n_samples)) return rc;
    StreamInput in{};
    if (int rc = stream_input_check(sample_rate, format, channels, hop_frames, n_samples, &in)) return rc;
    const bool plain = sample_rate == WW_SAMPLE_RATE && format == WW_FMT_F32 && channels == 1;   // today's streamer, node for node
    return streamer_create(n_mics, in.hop_out, n_samples, plain ? nullptr : &in, packed_dev, n_conv, stream, out);
}

int ww_streamer_create(int32_t n_mics, int32_t hop_samples, const float* packed_dev, int32_t n_conv,
                       ww_stream_t stream, ww_streamer** out) {
    return ww_streamer_create_n(n_mics, hop_samples, kClip, packed_dev, n_conv, stream, out);
}

static int streamer_replay(ww_streamer* s, const void* hop_dev, float* prob_dev, float* logits_dev) {
    float* lg = logits_dev ? logits_dev : s->own_logits;
    if (!s->exec || s->cap_hop != hop_dev || s->cap_prob != prob_dev || s->cap_logits != lg) {
        // (re)capture: the I/O pointers are baked into the graph's kernel nodes
        if (s->exec) { (void)hipGraphExecDestroy(s->exec); s->exec = nullptr; }
        if (s->graph) { (void)hipGraphDestroy(s->graph); s->graph = nullptr; }
        WW_HIP(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
        const int rc = streamer_enqueue(s, hop_dev, prob_dev, lg);
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(s->stream, &g);
        if (rc != WW_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (e != hipSuccess) return fail(WW_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
        s->graph = g;
        WW_HIP(hipGraphInstantiate(&s->exec, s->graph, nullptr, nullptr, 0));
        s->cap_hop = hop_dev; s->cap_prob = prob_dev; s->cap_logits = lg;
    }
    WW_HIP(hipGraphLaunch(s->exec, s->stream));
    return WW_OK;
}

int ww_streamer_step(ww_streamer* s, const float* hop_dev, float* prob_dev, float* logits_dev) {
    if (!s || !hop_dev || !prob_dev) return fail(WW_EINVAL, "null argument");
    if (reinterpret_cast<uintptr_t>(hop_dev) & 3) return fail(WW_EINVAL, "hop_dev must be float-aligned");
    if (s->input) return fail(WW_EINVAL, "this streamer takes hops at %d Hz in format %d: use ww_streamer_step_input", s->in.rate, s->in.format);
    return streamer_replay(s, hop_dev, prob_dev, logits_dev);
}

int ww_streamer_step_input(ww_streamer* s, const void* hop_dev, float* prob_dev, float* logits_dev) {
    if (!s || !hop_dev || !prob_dev) return fail(WW_EINVAL, "null argument");
    const int bytes = s->input ? sample_bytes(s->in.format) : 4;
    const int align = bytes == 3 ? 1 : bytes;                   // S24: packed 3-byte samples, read byte by byte
    if (reinterpret_cast<uintptr_t>(hop_dev) & (align - 1)) return fail(WW_EINVAL, "hop_dev must be aligned to %d bytes", align);
    return streamer_replay(s, hop_dev, prob_dev, logits_dev);
}

int ww_streamer_latency(const ww_streamer* s) {
    if (!s) return fail(WW_EINVAL, "null argument");
    return s->input ? s->in.latency : 0;
}

int ww_streamer_window(ww_streamer* s, float* window_dev) {
    if (!s || !window_dev) return fail(WW_EINVAL, "null argument");
    return launch<ring_unroll_kernel>(dim3(1024), dim3(256), 0, s->stream, s->ring, s->pos, window_dev, s->n_mics, s->n_samples);
}

int ww_streamer_destroy(ww_streamer* s) {
    if (!s) return WW_OK;
    if (s->exec) (void)hipGraphExecDestroy(s->exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    if (s->ring) (void)hipFree(s->ring);
    if (s->pos) (void)hipFree(s->pos);
    if (s->workspace) (void)hipFree(s->workspace);
    if (s->own_logits) (void)hipFree(s->own_logits);
    stream_input_free(&s->in);
    delete s;
    return WW_OK;
}

}  // extern "C"
