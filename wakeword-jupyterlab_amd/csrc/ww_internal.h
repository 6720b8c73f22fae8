// Internal definitions shared by the translation units of libwakeword_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "wakeword_amd.h"

namespace ww {

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
int fail(int code, const char* fmt, ...);
#define WW_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return ::ww::fail(WW_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                              __FILE__, __LINE__);                                           \
    } while (0)

// THE rounding of every workspace region: sizes and offsets are multiples of 256 bytes
inline int64_t up256(int64_t b) { return (b + 255) & ~int64_t(255); }

// ---------------------------------------------------------------------------------------------
// THE kernel launch: LDS opt-in, launch and error check.  Every launch in the library is
//     return launch<kernel<...>>(grid, block, lds_bytes, stream, args...);
// (or `if (int rc = launch<...>(...)) return rc;` where more follows).  The arguments convert to the kernel's parameter types as in a
// plain call, so a null pointer is `nullptr`.  An error carries the call site's file and line, in WW_HIP's form.
// ---------------------------------------------------------------------------------------------
constexpr size_t kLdsNoOptIn = 64 * 1024;   // dynamic LDS a kernel gets without asking; up to 160 KiB per workgroup with an opt-in
constexpr int kLdsOptInDevices = 64;

struct LaunchGrid {        // the grid, with the place it was written at
    dim3 dim;
    const char* file;
    int line;
    LaunchGrid(dim3 d, const char* f = __builtin_FILE(), int l = __builtin_LINE()) : dim(d), file(f), line(l) {}
};

inline int launch_fail(const char* what, hipError_t e, const LaunchGrid& at) {
    return fail(WW_EHIP, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), at.file, at.line);
}

// The slow path of launch(): `granted` is the byte count this kernel instantiation was last opted in to on the current device.
inline int lds_opt_in(const void* kernel, size_t lds_bytes, std::atomic<size_t>& granted, const LaunchGrid& at) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (lds_bytes <= granted.load(std::memory_order_relaxed)) return WW_OK;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
    if (e != hipSuccess) return launch_fail("the opt-in to hipFuncAttributeMaxDynamicSharedMemorySize", e, at);
    granted.store(lds_bytes, std::memory_order_release);
    return WW_OK;
}

template <auto Kernel, class... A>
int launch(LaunchGrid grid, dim3 block, size_t lds_bytes, hipStream_t stream, A&&... args) {
    if (lds_bytes > kLdsNoOptIn) {       // once per (kernel instantiation, device), before its first launch there
        static std::atomic<size_t> granted[kLdsOptInDevices] = {};
        int dev = 0;
        const hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return launch_fail("hipGetDevice(&dev)", e, grid);
        if (dev < 0 || dev >= kLdsOptInDevices) return fail(WW_EINVAL, "device ordinal out of range");
        if (lds_bytes > granted[dev].load(std::memory_order_acquire))
            if (int rc = lds_opt_in(reinterpret_cast<const void*>(Kernel), lds_bytes, granted[dev], grid)) return rc;
    }
    hipLaunchKernelGGL(Kernel, grid.dim, block, lds_bytes, stream, std::forward<A>(args)...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WW_OK : launch_fail("hipGetLastError()", e, grid);
}

// ---------------------------------------------------------------------------------------------
// K1 tables (one image per device, built on the host in double precision)
// ---------------------------------------------------------------------------------------------
constexpr int kClip = WW_CLIP_SAMPLES;
constexpr int kNfft = WW_N_FFT;
constexpr int kHop = WW_HOP;
constexpr int kMels = WW_N_MELS;
constexpr int kFrames = WW_N_FRAMES;
constexpr int kBins = WW_N_BINS;

// The mel matrix (2004 non-zeros, <=2 filters per bin, every filter one contiguous run of 9..75 bins) is cut
// into PIECES: (filter f, aligned window of 8 bins [8m, 8m+8)) with 8 weights (zero outside the filter).
// 317 real pieces -> 5 rounds of 64 lane-slots; every lane of the mel stage runs the same trip count and reads
// its 8 power bins with two aligned ds_read_b128.  Slot order = sorted by window, dealt out so that the 16 lanes
// of one ds_read_b128 hardware group read neighbouring windows (conflict-free, mostly broadcast).
constexpr int kPieceLen = 8;
constexpr int kPieceRounds = 5;             // pieces per lane-slot
constexpr int kPieceSlots = 64;             // lane-slots
constexpr int kPieces = kPieceRounds * kPieceSlots;  // 320 >= number of real pieces (checked on host)

struct LogmelTables {
    float window[kNfft];          // periodic Hann
    float2 tw1[7][128];           // W_1024^(n' * k1),  k1 = 1..7, n' = 0..127
    float2 tw2[7][16];            // W_128^(n'' * k2),  k2 = 1..7, n'' = 0..15
    float2 twp[512];              // W_2048^k, k = 0..511, except twp[0] = W_2048^512 (lane 0 takes bin 512)
    float piece_w[2][kPieces][4]; // [half][slot index c*64+lane][4]: weights of bins 8m+4*half .. +3
    int32_t piece_info[kPieces];  // (8m) | (output position << 16); output positions are filter-major
    int32_t filt_p0[kMels];       // first output position of filter f
    int32_t filt_cnt[kMels];      // number of pieces of filter f
    // augmentation kernels (ww_augment.hip)
    float2 twr[1024];             // W_2048^k, k = 0..1023
    float kaiser_best[32772];     // resampler half-window: 64 zero crossings x 512 + 1 entries (+3 pad)
    // float64 forms for the precise log-mel kernel (logmel64_kernel): the same entries, not rounded to float
    double window_d[kNfft];
    double2 tw1_d[7][128];
    double2 tw2_d[7][16];
    double2 twp_d[512];
    // per mel band: the largest weight of the triangle and its reciprocal (the auto mode's rounding-floor test)
    float band_wmax[kMels];
    float band_bins[kMels];
};

void build_mel_filterbank(float* out /*[80][1025]*/);
void build_hann(double* out /*[2048]*/);
int build_logmel_tables(LogmelTables* t);   // host; returns number of real pieces or <0
const LogmelTables* device_tables();        // lazily uploaded for the current device (nullptr on error)

// ---------------------------------------------------------------------------------------------
// packed weight image (floats).  Offsets for n_conv = 2 | 3.
// ---------------------------------------------------------------------------------------------
constexpr int kHidden = WW_HIDDEN;
constexpr int kGateCols = 3 * kHidden;     // i, g, o (the forget gate is dead with zero state)

struct PackedLayout {
    int n_conv;
    int c_last;        // 64 | 128
    int64_t conv1_w;   // [32][9]
    int64_t conv1_b;   // [32]
    int64_t conv2_w;   // [2 ntile][144][64 lanes]  B-operand order
    int64_t conv2_b;   // [64]
    int64_t conv3_w;   // [4 ntile][288][64 lanes]  (n_conv 3)
    int64_t conv3_b;   // [128]
    int64_t l0_w;      // [c_last][768]  k-major, column = (hb*3 + gate)*32 + u
    int64_t l0_b;      // [768]
    int64_t l1_w;      // [256][768]
    int64_t l1_b;      // [768]
    int64_t fc_w;      // [2][256]
    int64_t fc_b;      // [2] (+2 pad)
    // split-precision images for the f16x3 kernels: W * 2^S = hi + lo (two f16) in MFMA operand order
    int64_t conv2_hs;  // [64]: 2^-S per output channel (descale applied to the f32 accumulator)
    int64_t conv1_h;   // conv1 as a 32x32x16 f16 MFMA A operand: [hi,lo][64 lanes][4 dwords]; k = tap 0..8, rest 0
    int64_t conv1_hs;  // [4]: 2^-S of conv1 (one scale for the tensor), 0, 0, 0
    int64_t conv3_h;   // (n_conv 3) conv3 split-precision B operands for 16x16x32: [8 ntile][18 kstep = (cb*3+dx)*3+dy][hi,lo][64][4]
    int64_t conv3_hs;  // [128]: 2^-S per output channel
    int64_t conv2_h16; // same weights for v_mfma_f32_16x16x32_f16: [4 ntile][9 kstep = dx*3+dy][hi,lo][64 lanes][4 dwords]
    int64_t l0_h;      // W_ih l0 split for v_mfma_f32_16x16x32_f16: [K/32][48 ntile][hi,lo][64 lanes][4 dwords], columns as l0_w
    int64_t l1_h;      // same for layer 1 (K = 256)
    int64_t lstm_hs;   // [2][768]: 2^-S per packed gate column, layer 0 then layer 1
    int64_t conv2_hw;  // conv2 as 1-D Winograd F(2,3) along rows, split precision: [4 ntile][12 kstep = xi*3+dx][hi,lo][64 lanes][4 dwords]
    int64_t conv2_hws; // [64]: 2^-S per output channel of the transformed weights
    int64_t conv3_hw;  // (n_conv 3) conv3 in the same Winograd form: [8 ntile][24 kstep = (xi*3+dx)*2 + cb][hi,lo][64 lanes][4 dwords]
    int64_t conv3_hws; // [128]
    int64_t range;     // [8]: l1 bound of conv1 (max over channels of sum |w|), max |b1|, the same for conv2, 0...
    int64_t total;
};
PackedLayout packed_layout(int n_conv);

// ---------------------------------------------------------------------------------------------
// kernel launchers (defined in the .hip files)
// ---------------------------------------------------------------------------------------------
int launch_logmel(const float* pcm, int64_t n_clips, int64_t clip_stride, int64_t clip_len, int normalize,
                  const int32_t* ring_pos /*nullable: streaming ring start per launch*/, int64_t ring_len,
                  float* logmel, hipStream_t stream);
// any clip length: rows of n_samples (<= 32000; clip_len <= n_samples valid), T = 1 + n_samples / 512 frames in [8, 63] -> [n][80][T]
int launch_logmel_frames(const float* pcm, int64_t n_clips, int64_t clip_stride, int64_t clip_len, int64_t n_samples, int normalize,
                         float* logmel, hipStream_t stream);
// the same over streaming rings of ring_len = clip_len = n_samples samples per row (a multiple of 4), window start *ring_pos (device)
int launch_logmel_frames(const float* pcm, int64_t n_clips, int64_t clip_stride, int64_t clip_len, int64_t n_samples, int normalize,
                         const int32_t* ring_pos, int64_t ring_len, float* logmel, hipStream_t stream);
// events on continuous audio (ww_events.hip): smooth per segment into s_work [n_windows] float64, then count events per (segment,
// threshold) into counts [n_segs][n_thr] (and, with n_thr == 1, one fired byte per window); the per-hop form for the streamer
int launch_events_sweep(const float* prob, const int64_t* offsets, int n_segs, int64_t n_windows, int smooth, int64_t refractory,
                        const float* thresholds, int n_thr, int64_t* counts, uint8_t* fired, double* s_work, hipStream_t stream);
int launch_events_step(const float* prob, int n_mics, int smooth, float threshold, int64_t refractory, void* state, uint8_t* fired,
                       hipStream_t stream);
// log-mel arithmetic: 0 = f32 FFT, 1 = f64 FFT (what the reference's numpy.fft.rfft is), 2 = auto (f32, then the clips whose
// quiet bands sit on the f32 FFT's rounding floor are redone in f64)
int logmel_math_mode();
void set_logmel_math_mode(int mode);
// ---- augmentation host path (ww_augment.hip, ww_reverb.hip): the entry points check N and the pointers, the prepare functions check the
// per-clip entries, both before any launch.  n_samples = 16000 (the 1 s entry points) or 4000 .. 16383 (the *_n, bg and rir ones).
// Which record arrays a call carries.  A records buffer is [n] AugDev, then [n] BgDev with kAugBg, then [n] RirDev with kAugRir, back to
// back; the workspace is the plain workspace followed by a 256-byte-rounded slot for each of the two in the same order.
enum : unsigned { kAugBg = 1, kAugRir = 2 };
int64_t augment_record_bytes(unsigned parts);                                    // per clip
int64_t augment_workspace_bytes(int64_t n, int64_t n_samples, unsigned parts);
ww_augment_layout augment_workspace_layout(int64_t n, int64_t n_samples);
struct AugStages { bool pitch, stretch, bg, rir; };    // the stages that some clip of the batch uses
struct AugCall {           // the device side of one call; bank / spectra stay zero where the call has none
    const float* pcm;
    int64_t n, stride, n_samples;
    float* out;
    int64_t out_stride;
    void* workspace;
    hipStream_t stream;
    const float* bank;
    int64_t bank_len;
    const float* spectra;
    int64_t n_rirs;
};
struct RirDev {            // one per clip, derived on the host from ww_augment_rir
    int64_t index;         // the RIR's spectrum; -1 = no reverb for this clip
    int32_t dpos;          // direct-path position within the kept taps
    int32_t pad_;
};
int background_prepare(const ww_augment_bg* bg_host, int64_t n, int64_t bank_len, void* records_host, bool* any_out);
int rir_prepare(const ww_augment_rir* rir_host, int64_t n, int64_t n_rirs, void* records_host, bool* any_out);
// plans (+ bg with kAugBg, + rir with kAugRir) -> a records buffer of `parts`; bg_host NULL with kAugBg: zero records, no background
int augment_prepare(const ww_augment_plan* plans_host, const ww_augment_bg* bg_host, const ww_augment_rir* rir_host, int64_t n,
                    int64_t n_samples, int64_t bank_len, int64_t n_rirs, unsigned parts, void* records_host, AugStages* stages_out);
// launches only, on a records buffer of `parts` in device memory: both vocoder stages, the reverb with kAugRir, mix_kernel last with kAugBg
int launch_augment_records(const AugCall& c, const void* records_dev, unsigned parts);
// a prepared records buffer in host memory -> the workspace's slots (only the arrays a stage in `st` reads), then the stages in `st`
int launch_augment(const AugCall& c, const void* records_host, unsigned parts, AugStages st);
// pinned staging of host records into device memory (ww_augment.hip): `pieces` byte ranges, each to its own address
int stage_to_device(const void* const* src, const size_t* sizes, void* const* dst, int pieces, hipStream_t stream);
// the standalone mix and reverb on prepared host records ([n] BgDev / [n] RirDev), staged into the workspace
int64_t mix_background_workspace_bytes(int64_t n);
int launch_mix_background(const AugCall& c, const void* records_host);
int launch_reverb_records(const float* in, int64_t in_stride, int64_t n, int n_samples, const RirDev* rir, const float2* spectra,
                          int64_t n_rirs, float* out, int64_t out_stride, hipStream_t stream);
int64_t reverb_workspace_bytes(int64_t n);
int launch_reverb(const AugCall& c, const void* records_host);
int64_t rir_spectra_workspace_bytes(int64_t n_rirs);
int launch_rir_spectra(const float* taps, int64_t taps_len, const int64_t* offsets_host, const int32_t* lengths_host, int64_t n_rirs,
                       float* spectra, void* workspace, hipStream_t stream);
void build_kaiser_best(float* out /*[32769]*/);
// SpecAugment on log-mel batches (ww_specaug.hip): what the generator needs to draw a clip's record
struct SpecDraw {
    uint64_t seed;
    float prob;
    int32_t n_freq, freq_max, n_time, time_max;
};
int launch_spec_draw(const SpecDraw& d, int64_t n, int T, int16_t* records, hipStream_t stream);
// records NULL: drawn from `d` inside the kernel; in == out or disjoint (the entry point checks)
int launch_spec_augment(const float* in, float* out, int64_t n, int T, const int16_t* records, const SpecDraw& d, int mode, float fill_value,
                        hipStream_t stream);
// microphone-channel augmentation (ww_channel.hip): records [n][48] float32 or NULL = drawn from (seed, g) inside the kernel; in == out or
// disjoint, n_samples 4000 .. 16383 (the entry point checks)
int launch_channel_draw(const ww_channel_config& g, uint64_t seed, int64_t n, float* records, hipStream_t stream);
int launch_channel(const float* in, float* out, int64_t n, int n_samples, int64_t row_stride, const float* records, uint64_t seed,
                   const ww_channel_config& g, hipStream_t stream);
// mixup on log-mel batches (ww_mixup.hip): out of place; 16-byte accesses when mel and out are both 16-byte aligned
int launch_mixup(const float* mel, float* out, int64_t B, int T, const int64_t* labels, const int32_t* partner, const float* lambda,
                 float* targets, hipStream_t stream);
int sync_timeouts(unsigned int* count);   // bounded LDS-counter waits that expired (must be 0)
int64_t cnn_scratch_bytes(int64_t n, int n_conv);
int launch_cnn_pool(const float* mel, int64_t n, int width, const float* packed, int n_conv, void* scratch,
                    float* pooled, hipStream_t stream);
// K2 for 33..63 columns: column tiles of 32 run through the kernels above as virtual clips, each pooling the columns it owns (ww_cnn.hip)
int cnn_wide_tiles(int width, int n_conv);
int64_t cnn_wide_scratch_bytes(int64_t n, int width, int n_conv);
int launch_cnn_pool_wide(const float* mel, int64_t n, int width, const float* packed, int n_conv, void* scratch, float* pooled,
                         hipStream_t stream);
// conv math: 0 = exact f32 MFMA (v_mfma_f32_32x32x2_f32), 1 = f16x3 split (3 x v_mfma_f32_16x16x32_f16 per product block; conv2 of
// the 2-conv model as 1-D Winograd), 2 = f16x3 split with every conv in its direct form
int conv_math_mode();
void set_conv_math_mode(int mode);
int launch_lstm_fc(const float* pooled, int64_t n, const float* packed, int n_conv, float* logits,
                   float* prob /*nullable*/, hipStream_t stream);

// training step (ww_train.hip)
int64_t train_workspace_bytes(int64_t n, int n_conv, int mode);
int train_forward(const float* mel, int64_t n, int width, const ww_train_params* p, float p_lstm, float p_fc, uint64_t seed, int mode,
                  void* workspace, int64_t workspace_bytes, float* logits, hipStream_t st);
int train_masks(const void* workspace, int64_t n, int n_conv, float* mask0, float* mask1, hipStream_t st);
int train_packed_image(const void* workspace, int64_t n, int n_conv, float* img, hipStream_t st);
int train_bit_images(const void* workspace, int64_t n, int n_conv, uint8_t* mask_last, uint32_t* sign1, hipStream_t st);
int launch_decode_mask_image(const uint32_t* img, int64_t n, int C, uint8_t* out, hipStream_t st);
int train_stage_mode_check(const void* workspace, int mode);
int64_t train_stage_floats(int64_t n, int n_conv, int mode, int stage);
int train_stage(const void* workspace, int64_t n, int n_conv, int mode, int stage, float* out, hipStream_t st);
int launch_decode_channels_last(const float* src, const float* scale /*nullable*/, int64_t n, float* out, hipStream_t st);
int train_backward(const float* mel, int64_t n, int width, const ww_train_params* p, const float* dlogits, int mode, void* workspace,
                   int64_t workspace_bytes, const ww_train_grads* g, hipStream_t st);

int train_math_mode();   // 0 exact fp32, 1 split-precision conv backward where a kernel exists (ww_train_h.hip)
int launch_pack_conv_h_dev(const ww_train_params* p, float* img, hipStream_t st);
int launch_cnn3w_pool_bits(const float* mel, int64_t n, int width, const float* packed, float* mid2, float* apow2, float* pooled,
                           uint32_t* bits3, uint32_t* bits1, hipStream_t stream);
int launch_cnn2w_pool_bits(const float* mel, int64_t n, int width, const float* packed, float* pooled, uint32_t* bits, uint32_t* bits1,
                           hipStream_t stream);
// the exact-fp32 training forward of the conv stack, on the live parameters (wB: conv2 / conv3 weights in B-operand order)
int launch_cnn2_f32_mid(const float* mel, int64_t n, int width, const float* w1, const float* b1, const float* wB, const float* b2, float* mid,
                        hipStream_t stream);
int launch_cnn3_f32_store(const float* mid2, int64_t n, int width, const float* wB, const float* b3, float* pooled, float* mid3,
                          hipStream_t stream);
int launch_conv2_wgrad_h(const float* mel, const uint32_t* maskbits, const float* gp, int64_t n, int width, const float* packed,
                         float* partial, int grid, hipStream_t st);

int launch_conv3_wgrad_h(const float* act2, const float* apow2, const uint32_t* maskbits, const float* gp, int64_t n, float* partial,
                         float* dw, float* db, int grid, hipStream_t st);
int64_t dgrad_h_scratch_floats(int64_t n, int n_conv);
float* dgrad_h_scratch2(float* scratch, int64_t n);
float* dgrad_h_dzs(float* scratch, int64_t n);
int launch_conv2_wgrad_h_dense(const float* mel, const float* dz2h, const float* dzs, int64_t n, int width, const float* packed, float* partial,
                               int grid, hipStream_t st);
int launch_conv2_dgrad_h_dense(const float* mel, const float* dz2h, const float* dzs, const uint32_t* bits1, const float* w2, float* scratch2,
                               int64_t n, int width, float* partial, int grid, hipStream_t st);
int launch_gp_max(const float* dpooled, float s, int64_t n, int n_conv, float* gp, float* scratch, hipStream_t st);
int launch_conv3_dgrad_h(const float* act2, const uint32_t* maskbits, const float* gp, const float* w3, float* scratch, int64_t n, float* dz2h,
                         float* dzs, int grid, hipStream_t st);
int launch_conv2_dgrad_h(const float* mel, const uint32_t* maskbits, const uint32_t* bits1, const float* gp, const float* w2, float* scratch,
                         int64_t n, int width, float* partial, int grid, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// FLAC (ww_flac_index.h: container walk + frame index on the host, inside ww_files.cpp; ww_flac.hip: sample decode on the device)
// ---------------------------------------------------------------------------------------------
struct FlacHead {                 // STREAMINFO and where the first frame starts
    int channels = 0, bps = 0, sample_rate = 0, min_block = 0, max_block = 0;
    int64_t total_samples = 0, audio_start = 0;
};
// One verified frame of a file.  Byte positions are relative to the file's first frame.
struct FlacFrame {
    int64_t byte_off;             // first byte of the frame header
    int64_t sample_off;           // first sample frame of the block inside the file
    int32_t byte_len;             // header .. CRC-16 inclusive
    int32_t header_len;           // header bytes, CRC-8 included (the subframes start behind it)
    int32_t block_size;
    int32_t chan_assign;          // 0..7 = 1..8 independent channels, 8 left/side, 9 side/right, 10 mid/side
};
static_assert(sizeof(FlacFrame) == 32, "FlacFrame is shared with the device");
// One FLAC file of a batch, as the decode kernel sees it.  Offsets are bytes from the slot's device buffer.
struct FlacClip {
    int64_t comp_off;             // the file's frames (uploaded with the staging)
    int64_t frames_off;           // its FlacFrame records (uploaded with the staging)
    int64_t dec_off;              // float32 interleaved output, n_samples * channels (behind the staging's max_raw bytes)
    int64_t first_frame;          // index of its first frame among all FLAC frames of the batch
    int32_t n_blocks, clip, channels, bps;
    int32_t err, _pad[3];         // err: set by the device when the file's bitstream is inconsistent
};
static_assert(sizeof(FlacClip) == 64, "FlacClip is shared with the device");

// The decode kernel: one lane per frame; writes float32 samples at raw_dev + dec_off; a file with an inconsistent bitstream gets
// n_frames = 0 in its descriptor (K0 then writes a zero row) and is counted in the FLAC error counter.
// (default visibility: ww_files.cpp is also linked on its own against the library, by the reader's ThreadSanitizer test)
__attribute__((visibility("default"))) int launch_flac_decode(uint8_t* raw_dev, FlacClip* clips_dev, int n_flac, int64_t n_frames_total, ww_clip_desc* descs_dev,
                       hipStream_t stream);
int flac_errors(unsigned int* count);

// ---------------------------------------------------------------------------------------------
// streaming at the microphone's rate, format and channel count (ww_decode.hip, beside K0 whose filter and conversion it shares)
// ---------------------------------------------------------------------------------------------
struct StreamInput {
    int rate, format, channels, hop_in, hop_out;
    int up, down, lh;         // K0's filter for `rate` (up == down == 1 at 16 kHz: no filter)
    int latency;              // D: the window lags the input by D samples at 16 kHz
    int hist;                 // P: mono frames before a hop that its outputs still read (kept per mic between hops)
    int block;                // outputs per LDS block (their input span fits kStreamSpan frames)
    int span;                 // the longest such span: LDS frames per workgroup
    const float* taps;        // device, K0's cached filter (not owned)
    int32_t* table;           // device [3][hop_out]: first input frame relative to the hop, first tap, tap count
    float* history;           // device [2][n_mics][hist]: ping-pong by the parity the kernel keeps in pos[2]
};
// Host only, no HIP call: checks rate, format, channels and hop (WW_EINVAL naming the field) and fills the scalar fields.
int stream_input_check(int rate, int format, int channels, int hop_in, int n_samples, StreamInput* si);
// Allocates the table and the zeroed history on `stream` (after stream_input_check).
int stream_input_alloc(StreamInput* si, int n_mics, hipStream_t stream);
void stream_input_free(StreamInput* si);
// One hop: converts and resamples hop [n_mics][hop_in][channels] into the ring and advances pos (the ring_append_kernel protocol:
// pos[0] ring position, pos[1] ticket; plus pos[2] history parity and pos[3] hops so far, saturating).
int launch_stream_input(const StreamInput& si, const void* hop, int n_mics, float* ring, int32_t* pos, int ring_len, hipStream_t stream);
int sample_bytes(int format);   // bytes per sample of a WW_FMT_* PCM format (0 for FLAC and unknown)

int require_gfx950();
int device_cu_count();   // CUs of the current device (256 on MI355X); cached

}  // namespace ww
