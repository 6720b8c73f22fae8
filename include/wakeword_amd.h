/*
 * wakeword_amd.h -- C ABI of libwakeword_amd.so (MI355X / gfx950 native).
 *
 * The reference (sarpel/wakeword-jupyterlab) is pure Python and has no FFI: its boundary for the
 * hot path is three Python call signatures.  Each entry point below names the reference code it
 * replaces (paths relative to the reference repository).  The Python host layer
 * (the .py files of wakeword-jupyterlab_amd) binds these with ctypes and re-exposes the reference signatures;
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every `*_dev` pointer is a DEVICE pointer (HBM) on the current HIP device; every `*_host`
 *     pointer is ordinary host memory.  No torch / C++ types cross this boundary.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  All launch
 *     functions are asynchronous on that stream, allocate nothing, never synchronise and are
 *     therefore capturable into a hipGraph once ww_init() has run on the device (exception, stated
 *     at the function: ww_augment_f32 / ww_augment_n_f32 read their plans from host memory and are not capturable; the two-call
 *     forms ww_augment_plans_prepare(_n) + ww_augment_records(_n)_f32 are).
 *   - a `workspace_dev` / `scratch_dev` buffer is the caller's, of at least the size its query returns; the library writes nothing past
 *     that size.  Unless a function says otherwise (state that must be zeroed or initialised first) its content on entry is unspecified.
 *   - return value: WW_OK (0) or a negative WW_E* code; ww_last_error() gives the message of the
 *     calling thread's most recent failure.  Nothing falls back to a CPU path: without a usable
 *     gfx950 device every launch function fails with WW_ENODEVICE.
 *   - all tensors are float32, C-contiguous in the stated shape unless a stride is a parameter.
 */
#ifndef WAKEWORD_AMD_H
#define WAKEWORD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WW_ABI_VERSION 4 /* 2: ww_set_logmel_math, ww_train_*, third conv-math mode; 3: ww_set_train_math (round 2); 4: ww_wav_reader_*, ww_read_wav_batch_host (round 3) */

#if defined(WW_BUILD)
#define WW_API __attribute__((visibility("default")))
#else
#define WW_API
#endif

#define WW_OK 0
#define WW_EINVAL (-1)    /* bad shape / alignment / argument */
#define WW_ENODEVICE (-2) /* no HIP device, or not gfx950 */
#define WW_EHIP (-3)      /* a HIP runtime call failed */
#define WW_EUNSUPPORTED (-4)
#define WW_ENOSPACE (-5)  /* a caller-sized buffer (the WAV reader's staging) is too small for this request */

/* AudioConfig, wakeword_training_script.py:29-37 (dup wakeword_training.ipynb cell 3);
 * Config, wakeword_training/train_wakeword.py:16-25; ModelConfig, wakeword_training_script.py:39-43 */
#define WW_SAMPLE_RATE 16000
#define WW_CLIP_SAMPLES 16000
#define WW_N_FFT 2048
#define WW_HOP 512
#define WW_N_MELS 80
#define WW_N_FRAMES 32 /* 1 + 16000/512, librosa center=True */
#define WW_N_BINS 1025
#define WW_HIDDEN 256
#define WW_N_CLASSES 2
#define WW_MAX_WIDTH 32 /* widest mel image (frames) the conv kernels take: T in [1, 32] */
/* Any clip length from 0.25 s to 2 s (AudioConfig.DURATION in [0.25, 2.0], inference only): N = int(16000 * DURATION) samples,
 * T = 1 + N / 512 frames.  The *_frames_* / *_wide_* entry points below take these; the 1 s entry points keep their limits. */
#define WW_MIN_CLIP_SAMPLES 4000
#define WW_MAX_CLIP_SAMPLES 32000
#define WW_MAX_FRAMES 63 /* 1 + 32000 / 512 */

typedef void* ww_stream_t;

/* ---- library / device ------------------------------------------------------------------- */
WW_API int ww_abi_version(void);
WW_API const char* ww_last_error(void);
/* Build and upload the front-end tables (window, twiddles, sparse mel pieces) for the current
 * device.  Idempotent.  Must have run once on a device before any launch below is captured into
 * a hipGraph (it allocates and synchronises); the launch functions call it lazily otherwise. */
WW_API int ww_init(void);
/* Device facts used by bench.py for the roofline denominator: number of CUs, max clock (kHz). */
WW_API int ww_device_info(int* n_cu, int* clock_khz, char* name, int name_len);
/* Health check (synchronises the device): how many bounded in-kernel waits of the conv kernel's producer/consumer
 * protocol have expired since the library was loaded.  Always 0 unless the protocol is broken; negative = error code.
 * A workgroup whose wait expired overwrites every output it produced with NaN before it exits, so a broken launch
 * cannot be consumed silently even without this call. */
WW_API int ww_sync_timeouts(void);
/* Health check (synchronises the device): how many FLAC files since the library was loaded had CRCs that verified but a bitstream the
 * decoder could not follow (reserved codes, a negative LPC shift, a residual layout the block does not allow, a sample outside its bit
 * width, subframes running past the frame).  Each such file was decoded to a zero row; its `ok` flag (decided on the host) stays True.
 * 0 for files any conforming encoder writes; negative = error code. */
WW_API int ww_flac_errors(void);

/* Arithmetic of the implicit GEMMs (conv1/conv2/conv3 and the LSTM gate GEMMs: all but ~1 % of the model's flops);
 * process-wide, default F16X3.
 *   WW_CONV_MATH_F32    v_mfma_f32_32x32x2_f32 / 16x16x4_f32: exact fp32 products and accumulation (an fmaf chain)
 *   WW_CONV_MATH_F16X3  each fp32 operand carried as two f16 halves (22 significant bits), every product block as
 *                       three f16 MFMAs (v_mfma_f32_16x16x32_f16) with fp32 accumulation: ~2^-21 relative error per
 *                       product (PyTorch's own default for convolutions on the reference's GPU is TF32, 2^-11), 3/16
 *                       of the matrix-core cycles.  Holds for any finite weights and inputs: weights carry a
 *                       power-of-two scale per output channel, inputs and activations one exponent per clip chosen
 *                       from the clip's max |x| and the layers' l1 bounds, so no f16 half overflows or goes subnormal. */
#define WW_CONV_MATH_F32 0
#define WW_CONV_MATH_F16X3 1
/*   WW_CONV_MATH_F16X3_DIRECT  F16X3 with every convolution in its direct (implicit-GEMM) form.  Under F16X3 conv2 of BOTH models and
 *                       conv3 of the 3-conv model run as a one-dimensional Winograd F(2,3) along the image rows (1.5x fewer
 *                       matrix instructions; the transforms are fp32 adds on the activations and exact-in-double combinations
 *                       of the weights); under F16X3_DIRECT every convolution of both models is direct. */
#define WW_CONV_MATH_F16X3_DIRECT 2
WW_API int ww_set_conv_math(int mode);
WW_API int ww_get_conv_math(void);   /* what a launch from the calling thread would use now (its override, else the process default) */
/* Per-thread override of the process-wide setting: launches issued by the CALLING THREAD use `mode` until it is cleared with
 * WW_MATH_INHERIT; other threads are unaffected.  A launch reads its mode once.  (ww_set_logmel_math_thread: the same for K1.) */
#define WW_MATH_INHERIT (-1)
WW_API int ww_set_conv_math_thread(int mode);

/* Arithmetic of the log-mel front end (K1), process-wide, default AUTO.  The reference's STFT is float64 (librosa forms
 * window * frame in float64 and numpy.fft.rfft runs in double; wakeword_training_script.py:89-98), then everything is
 * float32.  A float32 FFT leaves a rounding floor ~165 dB under a frame's energy: mel bands of noise-free signals that lie
 * 60-80 dB under the clip's peak come out up to 3.4e-4 dB off (clips with a broadband floor above about -60 dB, like the
 * benchmark's sine + noise clips, are unaffected: <= 1.5e-5 dB).
 *   WW_LOGMEL_MATH_F32   float32 FFT for every clip (the throughput kernel)
 *   WW_LOGMEL_MATH_F64   window product, FFT and real-input split in float64 for every clip (~4x the time)
 *   WW_LOGMEL_MATH_AUTO  the float32 kernel, which marks the clips that have a live (unclamped) mel band on its rounding
 *                        floor; a second launch redoes exactly those clips in float64.  MEASURED, not proven: <= 1.5e-5 dB
 *                        against the float64 reference on every noise-free test signal of tests/test_gpu_parity.py (the marking
 *                        threshold, band/frame energy ratio 1e-5, sits 2.7x above the boundary 10^-5.43 found on that sample,
 *                        profiles/r02_diag_floor.log).  Cost: one near-empty launch when no clip is marked; a marked clip costs
 *                        the float64 kernel (~3x): clean-speech / digitally silent data pays up to K1 x3 (bench line:
 *                        stages.K1_logmel.noise_free_batch). */
#define WW_LOGMEL_MATH_F32 0
#define WW_LOGMEL_MATH_F64 1
#define WW_LOGMEL_MATH_AUTO 2
WW_API int ww_set_logmel_math(int mode);
WW_API int ww_get_logmel_math(void);
WW_API int ww_set_logmel_math_thread(int mode);

/* ---- front-end tables, host side (no GPU needed; lets CPU tests check them) ------------------ */
/* librosa.filters.mel(sr=16000, n_fft=2048, n_mels=80, fmin=0, fmax=8000, htk=False,
 * norm='slaney') as used by wakeword_training_script.py:89-98 -> [80][1025] float32. */
WW_API int ww_mel_filterbank_host(float* out_host);
/* periodic Hann window of 2048 points (librosa.stft window='hann') -> [2048] float32. */
WW_API int ww_hann_window_host(float* out_host);

/* ---- K0: decode + mono + resample + normalise + crop/pad ------------------- */
/* Replaces the numeric part of AudioProcessor.load_audio = librosa.load(path, sr=16000)
 * (wakeword_training_script.py:65-71), normalize_audio (:73-76) and pad_or_truncate (:78-83): process_audio_file
 * :125-133 up to the mel call.  The host reads the file and parses the RIFF header; everything on samples runs here.
 * The resampler follows scipy.signal.resample_poly's design; librosa's (soxr_hq) differs: unpinned, see DESIGN.md. */
#define WW_FMT_S16 1
#define WW_FMT_S24 2
#define WW_FMT_S32 3
#define WW_FMT_F32 4
#define WW_FMT_U8 5
#define WW_FMT_F64 6 /* IEEE double samples (WAVE_FORMAT_IEEE_FLOAT, 64 bits): rounded to float32 as soundfile does for dtype float32 */
#define WW_FMT_FLAC 7 /* a FLAC file (RFC 9639, 4..24 bits, 1..8 channels) as the reader and the probe report it; byte_offset = its first
                         frame.  ww_wav_batch_decode decodes it on the device to float32 x * 2^-(bps-1) (what a WAV of the same integers
                         gives) and K0 reads that as WW_FMT_F32.  K0 itself does not decode it: a descriptor that still says
                         WW_FMT_FLAC gives a zero row and no sample byte is read. */
typedef struct ww_clip_desc {
    int64_t byte_offset;  /* start of the interleaved sample data of this file inside raw_dev */
    int64_t n_frames;     /* sample frames in the file */
    int32_t channels;
    int32_t sample_rate;
    int32_t format;       /* WW_FMT_* */
    int32_t crop_start;   /* first 16 kHz output sample of the 1 s window (host draws it: pad_or_truncate's random crop) */
    int32_t up, down, half_len, _pad; /* filled by ww_resampler_prepare */
    const void* taps_dev; /* filled by ww_resampler_prepare (NULL when the file is already 16 kHz) */
} ww_clip_desc;
/* The polyphase taps for `sample_rate` -> 16 kHz on the host (no GPU needed); returns the tap count (0 = no filter),
 * or the count needed when taps_host is NULL. */
WW_API int ww_resample_taps_host(int32_t sample_rate, float* taps_host, int32_t max_taps, int32_t* up, int32_t* down, int32_t* half_len);
/* Fill up/down/half_len/taps_dev of one descriptor; uploads the filter for this rate once per device (allocates). */
WW_API int ww_resampler_prepare(int32_t sample_rate, ww_clip_desc* desc_host);
/* raw_dev: the files' sample bytes; descs_dev: [n_clips] descriptors in device memory; pcm_out_dev [n_clips][16000]. */
WW_API int ww_decode_resample(const uint8_t* raw_dev, const ww_clip_desc* descs_dev, int64_t n_clips, int normalize,
                              float* pcm_out_dev, ww_stream_t stream);
/* The same with rows of n_samples (16000, or WW_MIN_CLIP_SAMPLES..WW_MAX_CLIP_SAMPLES: clips of 0.25 .. 2 s): pcm_out_dev [n_clips][n_samples];
 * crop_start is then the first output sample of the n_samples window (pad_or_truncate against n_samples). */
WW_API int ww_decode_resample_n(const uint8_t* raw_dev, const ww_clip_desc* descs_dev, int64_t n_clips, int normalize, int64_t n_samples,
                                float* pcm_out_dev, ww_stream_t stream);

/* ---- file-fed batches: the host half of load_audio for many files at once ------------------------------------- */
/* Replaces, for a batch of paths, the file access of AudioProcessor.load_audio = librosa.load(path, sr=16000)
 * (wakeword_training_script.py:65-71) as it is driven by WakewordDataset.__getitem__ (:204-216) under
 * DataLoader(batch_size=16, num_workers=2) (:461-463) -- the loop that bounds the reference at 453 clips/s
 * (wakeword_training.ipynb:742).  A reader owns `n_threads` host threads, `n_slots` pinned staging buffers with their
 * device twins, and a copy stream.  Per batch:
 *   ww_read_wav_batch_host  the threads open the files, walk the RIFF chunks and pread the sample bytes straight into
 *                           the slot's pinned staging; one ww_clip_desc per file is filled in (host, pinned; returned so
 *                           that the caller can set crop_start -- pad_or_truncate's random crop (:78-83) stays the
 *                           caller's draw: n_out = ceil(n_frames * up / down) is known now).  status_host[i] = 1, or a
 *                           WW_WAV_E* code for a file that could not be used (the reference prints and substitutes
 *                           zeros, :66-71, :210-211: such a file decodes to a zero clip here).  Blocks until the slot's
 *                           previous upload has left the staging buffer.  A FLAC file (magic "fLaC", an ID3v2 tag may precede
 *                           it) is staged as its frames plus a frame index built here (every CRC-8 and CRC-16 verified, no
 *                           sample decoded); its descriptor says WW_FMT_FLAC, and its decoded float32 samples count against
 *                           the same max_raw_bytes in a device-only region (WW_ENOSPACE reports the larger of the two needs).
 *   ww_wav_batch_decode     H2D copy of the slot on the reader's copy stream, then (only when the slot holds FLAC files) the
 *                           FLAC decode kernel, then K0 (ww_decode_resample) on `stream`
 *                           behind it: pcm_out_dev [n][16000].  Asynchronous; the next ww_read_wav_batch_host on ANOTHER
 *                           slot overlaps with it.  The upload of a slot waits for the K0 that last read its device twin.
 * A reader serves ONE caller at a time (its thread pool runs one batch); use one reader per consumer thread. */
#define WW_WAV_EOPEN (-1)    /* cannot open */
#define WW_WAV_ENOTRIFF (-2) /* neither a RIFF/WAVE nor a FLAC file */
#define WW_WAV_ECHUNK (-3)   /* fmt or data chunk missing / truncated; FLAC: STREAMINFO missing, a frame header or CRC-16 that does not
                                verify, a truncated frame */
#define WW_WAV_EFORMAT (-4)  /* encoding K0 does not take (it takes PCM u8/s16/s24/s32 and float32/float64, FLAC of 4..24 bits), or an
                                absurd rate */
#define WW_WAV_EIO (-5)      /* read error */
#define WW_WAV_ESPACE (-6)   /* the staging buffer was full (the call then returns WW_ENOSPACE with the size needed) */
typedef struct ww_wav_reader ww_wav_reader;
/* flags: WW_READER_HOST_ONLY = staging in ordinary host memory, no device twin, no GPU needed (ww_wav_batch_decode then returns
 * WW_EUNSUPPORTED): the RIFF walk and the threaded reads can be checked -- and run under a sanitizer -- on a CPU-only machine. */
#define WW_READER_HOST_ONLY 1
WW_API int ww_wav_reader_create(int32_t n_threads, int32_t n_slots, int64_t max_clips, int64_t max_raw_bytes, int32_t flags, ww_wav_reader** out);
WW_API int ww_wav_reader_destroy(ww_wav_reader* r);
/* The slot's staging buffer as the last ww_read_wav_batch_host left it (descs[i].byte_offset points into it); for tests. */
WW_API int ww_wav_reader_staging(ww_wav_reader* r, int32_t slot, const uint8_t** raw_host_out, int64_t* raw_bytes_out);
/* One file's header only (no GPU needed): returns 1 and fills n_frames / channels / sample_rate / format / up / down / half_len, with
 * byte_offset = the position of the sample data INSIDE THE FILE; or a WW_WAV_E* code.  A FLAC file is scanned whole (its frame index
 * gives n_frames): format = WW_FMT_FLAC, byte_offset = its first frame. */
WW_API int ww_wav_probe_host(const char* path, ww_clip_desc* desc_host);
/* raw_bytes_out (may be NULL): sample bytes of the batch, 16-byte aligned per file; on WW_ENOSPACE the size to create a reader with. */
WW_API int ww_read_wav_batch_host(ww_wav_reader* r, const char* const* paths, int64_t n, int32_t slot, ww_clip_desc** descs_host_out,
                                  int8_t* status_host, int64_t* raw_bytes_out);
WW_API int ww_wav_batch_decode(ww_wav_reader* r, int32_t slot, int normalize, float* pcm_out_dev, ww_stream_t stream);
/* ww_wav_batch_decode with rows of n_samples (as ww_decode_resample_n): pcm_out_dev [n][n_samples]. */
WW_API int ww_wav_batch_decode_n(ww_wav_reader* r, int32_t slot, int normalize, int64_t n_samples, float* pcm_out_dev, ww_stream_t stream);
/* The upload half of ww_wav_batch_decode, for a caller that runs K0 itself on windows of its own (AudioProcessor.load_audio): the slot's
 * H2D and, when it holds FLAC files, their decode on `stream`; then (synchronous) descs_out [n] receives the slot's descriptors as K0
 * takes them -- a FLAC file as WW_FMT_F32 at its decoded samples, n_frames 0 when its bitstream was inconsistent -- and *raw_dev_out the
 * device buffer their byte_offsets index.  Both stay valid until the next ww_read_wav_batch_host of the slot; whatever the caller
 * launches on them must have finished before the slot's next ww_wav_batch_decode / _stage.  The descriptors ww_read_wav_batch_host
 * returned are not changed by either call (a FLAC file keeps WW_FMT_FLAC and its staging offset there). */
WW_API int ww_wav_batch_stage(ww_wav_reader* r, int32_t slot, ww_stream_t stream, const uint8_t** raw_dev_out, ww_clip_desc* descs_out);

/* ---- KA: training-time augmentation ------------------------------ */
/* Replaces AudioProcessor.augment_audio (wakeword_training_script.py:103-123): np.roll time shift ->
 * librosa.effects.pitch_shift -> librosa.effects.time_stretch + pad_or_truncate -> additive Gaussian noise.
 * The random draws stay with the caller (the reference uses Python's `random`): one plan per clip.
 * librosa's phase vocoder (n_fft 2048, hop 512, Hann) is restated; its resampler (soxr_hq, third party)
 * is replaced by a Kaiser-windowed-sinc interpolator (resampy 'kaiser_best' design) and np.random.normal by
 * the build's counter-based generator: parity against librosa itself is unpinned (oracle/augment_oracle.py). */
typedef struct ww_augment_plan {
    int32_t shift;        /* np.roll shift in samples, any sign; 0 = no shift (:106-108) */
    int32_t crop_start;   /* pad_or_truncate's random crop start after time_stretch, in [0, round(16000/rate) - 16000] (N: see *_n below) */
    double pitch_rate;    /* 2^(-n_steps/12) of pitch_shift (:110-112); 0 = off */
    double stretch_rate;  /* time_stretch rate (:114-117); 0 = off.  Both rates: 32/46 <= rate < 32 */
    float noise_sigma;    /* NOISE_FACTOR (:119-121); 0 = off */
    uint32_t noise_seed;
} ww_augment_plan;
WW_API int64_t ww_augment_workspace_bytes(int64_t n_clips);
/* pcm_dev [n_clips] rows of 16000 samples at pcm_dev + i*clip_stride (16-byte aligned, clip_stride % 4 == 0);
 * plans_host [n_clips] in HOST memory: read before the call returns (staged through pinned memory owned by the library, so
 * the call is asynchronous on `stream`; it is not graph-capturable); out_dev [n_clips][16000], may alias pcm_dev;
 * workspace_dev >= ww_augment_workspace_bytes(n_clips), 256-byte aligned. Its content on entry is unspecified and no result depends on it. */
WW_API int ww_augment_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, const ww_augment_plan* plans_host,
                   float* out_dev, void* workspace_dev, ww_stream_t stream);
/* The same in two halves, for hipGraph capture: ww_augment_plans_prepare turns the plans into the fixed-size records the kernels read
 * (host arithmetic only: [n_clips] x ww_augment_record_bytes() bytes, e.g. into pinned memory), ww_augment_records_f32 is nothing but
 * kernel launches on `stream` reading the records from DEVICE memory -- capturable; both transform stages are always launched (a clip
 * whose plan switches one off is copied through it).  A captured step = {copy records host -> device, ww_augment_records_f32};
 * before every replay: ww_augment_plans_prepare into the host buffer.  Results equal ww_augment_f32's bit for bit. */
WW_API int64_t ww_augment_record_bytes(void);
WW_API int ww_augment_plans_prepare(const ww_augment_plan* plans_host, int64_t n_clips, void* records_host);
WW_API int ww_augment_records_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, const void* records_dev, float* out_dev,
                                  void* workspace_dev, ww_stream_t stream);
/* The four calls above for clips of n_samples = N samples, WW_MIN_CLIP_SAMPLES <= N <= WW_AUG_MAX_SAMPLES (T = 1 + N / 512 <= 32
 * frames, what the training kernels take); any other N is WW_EINVAL before anything is launched.  pcm_dev rows as above (16-byte aligned,
 * clip_stride >= N, clip_stride % 4 == 0); out_dev [n_clips] rows of N samples at out_dev + i*out_stride (out_stride >= N, any value;
 * 4-byte aligned), may alias pcm_dev.  The plan's shift is reduced mod N and crop_start lies in [0, round(N/rate) - N]; the rate bounds
 * are the 1 s ones (32/46 <= rate) at every N, with rate < T.  Records (still ww_augment_record_bytes() each) are valid only for the N
 * they were prepared for.  N = 16000 runs the 1 s kernels: results equal ww_augment_f32's bit for bit. */
#define WW_AUG_MAX_SAMPLES 16383 /* 1 + 16383 / 512 = 32 frames */
WW_API int64_t ww_augment_n_workspace_bytes(int64_t n_clips, int64_t n_samples);
WW_API int ww_augment_n_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_plan* plans_host,
                            float* out_dev, int64_t out_stride, void* workspace_dev, ww_stream_t stream);
WW_API int ww_augment_plans_prepare_n(const ww_augment_plan* plans_host, int64_t n_clips, int64_t n_samples, void* records_host);
WW_API int ww_augment_records_n_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const void* records_dev,
                                    float* out_dev, int64_t out_stride, void* workspace_dev, ww_stream_t stream);
/* Diagnostic: where the calls above leave their intermediates in workspace_dev, for n_clips clips of n_samples (16000 or the *_n range).
 * Byte offsets from workspace_dev and byte strides; the library sizes the workspace and places its buffers from this same function.
 *   records  [n_clips] per-clip records of record_bytes (ww_augment_record_bytes())
 *   buf_a    [n_clips] rows of row_bytes: the rolled input (rows padded with zeros to four floats)
 *   buf_b    [n_clips] rows of row_bytes: the resampled clips after a batch with pitch only, the cropped / zero-padded inverse STFT
 *            after a batch with stretch only (a batch with both: buf_a holds the stretch's output, buf_b its input)
 *   spec     [n_clips][46][1025] complex float32: the phase vocoder's output columns of the LAST vocoder pass that ran
 *   y        [n_clips] rows of y_clip_bytes: the pitch pass's inverse STFT, its first round(N / pitch_rate) samples
 * Nothing else is promised about the workspace's contents. */
typedef struct ww_augment_layout {
    int64_t records, buf_a, buf_b, spec, y;                       /* offsets */
    int64_t record_bytes, row_bytes, spec_clip_bytes, spec_step_bytes, y_clip_bytes;   /* strides */
    int64_t total_bytes;                                          /* = ww_augment_n_workspace_bytes(n_clips, n_samples) */
} ww_augment_layout;
WW_API int ww_augment_workspace_layout(int64_t n_clips, int64_t n_samples, ww_augment_layout* layout_out);
/* Background noise at a random SNR, mixed in after time_stretch + crop and before the Gaussian noise (additions only; no existing call,
 * struct or record changes).  The bank is one float32 device buffer of bank_len samples holding every noise file back to back.  Per clip:
 *   seg[j] = bank[file_offset + (start + j) mod file_len], j < N        (a file shorter than the clip repeats)
 *   Ex = sum x^2 over the clip, En = sum seg^2                           (float64, in a fixed order that depends on N alone)
 *   g = sqrt(Ex / (En * 10^(snr_db / 10))), out = fmaf(g, seg, x)       (nothing is added when Ex or En is 0)
 * -- the SNR as named: 10 log10(Ex / sum (g seg)^2) = snr_db.  Every call below returns WW_EINVAL before any launch for an enabled clip
 * with file_len <= 0, a file or start outside the bank, or a non-finite snr_db; clips with enabled = 0 are not looked at. */
typedef struct ww_augment_bg {
    int64_t file_offset;  /* the file's first sample in the bank */
    int64_t file_len;     /* the file's samples, > 0; file_offset + file_len <= bank_len */
    int64_t start;        /* segment start within the file, [0, file_len) */
    float snr_db;         /* finite */
    int32_t enabled;      /* 0 = no background for this clip */
} ww_augment_bg;
/* ww_augment_n_f32 with background, at N = 16000 or WW_MIN_CLIP_SAMPLES..WW_AUG_MAX_SAMPLES (rows and strides as there); bg_host [n_clips]
 * in host memory; workspace_dev >= ww_augment_bg_workspace_bytes(n_clips, N). Its content on entry is unspecified and no result depends on it.  With every enabled = 0 the results equal
 * ww_augment_n_f32's (and at N = 16000 ww_augment_f32's) bit for bit. */
WW_API int64_t ww_augment_bg_workspace_bytes(int64_t n_clips, int64_t n_samples);
WW_API int ww_augment_bg_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_plan* plans_host,
                             const ww_augment_bg* bg_host, const float* bank_dev, int64_t bank_len, float* out_dev, int64_t out_stride,
                             void* workspace_dev, ww_stream_t stream);
/* The same in two halves, for hipGraph capture (as ww_augment_plans_prepare_n / ww_augment_records_n_f32): records are
 * ww_augment_bg_record_bytes() per clip, laid out as [n_clips] augmentation records followed by [n_clips] background records, valid for
 * the N and the bank length they were prepared for (a background record that does not lie inside bank_len at launch mixes nothing).
 * The launch always ends in the mix kernel.  Results equal ww_augment_bg_f32's bit for bit. */
WW_API int64_t ww_augment_bg_record_bytes(void);
WW_API int ww_augment_bg_prepare(const ww_augment_plan* plans_host, const ww_augment_bg* bg_host, int64_t n_clips, int64_t n_samples,
                                 int64_t bank_len, void* records_host);
WW_API int ww_augment_bg_records_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const void* records_dev,
                                     const float* bank_dev, int64_t bank_len, float* out_dev, int64_t out_stride, void* workspace_dev,
                                     ww_stream_t stream);
/* The mix alone (no other transform, no Gaussian noise), e.g. for noisy evaluation sets at a fixed SNR: clips of N = WW_MIN_CLIP_SAMPLES ..
 * WW_MAX_CLIP_SAMPLES samples, rows at pcm_dev + i*clip_stride and out_dev + i*out_stride (4-byte aligned, strides >= N; out may alias
 * pcm row for row); workspace_dev >= ww_mix_background_workspace_bytes(n_clips), 256-byte aligned. Its content on entry is unspecified and no result depends on it. */
WW_API int64_t ww_mix_background_workspace_bytes(int64_t n_clips);
WW_API int ww_mix_background_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_bg* bg_host,
                                 const float* bank_dev, int64_t bank_len, float* out_dev, int64_t out_stride, void* workspace_dev,
                                 ww_stream_t stream);
/* Reverberation with a room impulse response (RIR), after time_stretch + crop and before the background mix (additions only).  A bank
 * holds each RIR as the spectrum of its kept taps h (at most WW_RIR_MAX_TAPS, direct path at dpos), zero-padded to WW_RIR_FFT_SIZE:
 * WW_RIR_SPECTRUM_BINS complex float32 values (float pairs) per RIR, in the library's own order.  Per clip of N samples:
 *   y[i] = sum_k h[k] x[i + dpos - k], i < N              (x zero outside [0, N): a linear convolution advanced by the direct path)
 *   out = g y, g = sqrt(Ex / Ey)                          (float64 sums of x^2 and y^2 in a fixed order; g = 1 when either is 0)
 * Every call below returns WW_EINVAL before any launch for an enabled clip whose index lies outside [0, n_rirs), whose taps lie outside
 * [1, WW_RIR_MAX_TAPS] or whose dpos lies outside [0, taps); clips with enabled = 0 are not looked at and pass through unchanged. */
#define WW_RIR_MAX_TAPS 16384
#define WW_RIR_FFT_SIZE 32768
#define WW_RIR_SPECTRUM_BINS 16385
typedef struct ww_augment_rir {
    int64_t index;        /* the RIR's spectrum in the bank, [0, n_rirs) */
    int32_t dpos;         /* direct-path position within the kept taps, [0, taps) */
    int32_t taps;         /* kept taps of that RIR, 1 .. WW_RIR_MAX_TAPS */
    int32_t enabled;      /* 0 = no reverb for this clip */
    int32_t reserved;     /* 0 */
} ww_augment_rir;
/* Bank build: spectra_dev [n_rirs][WW_RIR_SPECTRUM_BINS][2] from the taps of RIR r at taps_dev + offsets_host[r], lengths_host[r] of them
 * (1 .. WW_RIR_MAX_TAPS, inside taps_len); workspace_dev >= ww_rir_spectra_workspace_bytes(n_rirs), 256-byte aligned. Its content on entry is unspecified and no result depends on it. */
WW_API int64_t ww_rir_spectra_workspace_bytes(int64_t n_rirs);
WW_API int ww_rir_spectra_f32(const float* taps_dev, int64_t taps_len, const int64_t* offsets_host, const int32_t* lengths_host, int64_t n_rirs,
                              float* spectra_dev, void* workspace_dev, ww_stream_t stream);
/* ww_augment_bg_f32 with reverb (bg_host may be NULL: no background); spectra_dev holds n_rirs spectra; workspace_dev >=
 * ww_augment_rir_workspace_bytes(n_clips, N). Its content on entry is unspecified and no result depends on it.  With every rir enabled = 0 the results equal ww_augment_bg_f32's (bg_host NULL:
 * ww_augment_n_f32's) bit for bit. */
WW_API int64_t ww_augment_rir_workspace_bytes(int64_t n_clips, int64_t n_samples);
WW_API int ww_augment_rir_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_plan* plans_host,
                              const ww_augment_bg* bg_host, const float* bank_dev, int64_t bank_len, const ww_augment_rir* rir_host,
                              const float* spectra_dev, int64_t n_rirs, float* out_dev, int64_t out_stride, void* workspace_dev,
                              ww_stream_t stream);
/* The same in two halves, for hipGraph capture: records are ww_augment_rir_record_bytes() per clip, laid out as [n_clips] augmentation,
 * [n_clips] background and [n_clips] reverb records (bg_host may be NULL), valid for the N, bank length and n_rirs they were prepared
 * for (a reverb record outside n_rirs at launch passes its clip through).  The launch always runs the reverb and the mix kernels.
 * Results equal ww_augment_rir_f32's bit for bit. */
WW_API int64_t ww_augment_rir_record_bytes(void);
WW_API int ww_augment_rir_prepare(const ww_augment_plan* plans_host, const ww_augment_bg* bg_host, const ww_augment_rir* rir_host,
                                  int64_t n_clips, int64_t n_samples, int64_t bank_len, int64_t n_rirs, void* records_host);
WW_API int ww_augment_rir_records_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const void* records_dev,
                                      const float* bank_dev, int64_t bank_len, const float* spectra_dev, int64_t n_rirs, float* out_dev,
                                      int64_t out_stride, void* workspace_dev, ww_stream_t stream);
/* The reverb alone (no other transform), e.g. for reverberant evaluation sets: clips of N = WW_MIN_CLIP_SAMPLES .. WW_MAX_CLIP_SAMPLES
 * samples, rows at pcm_dev + i*clip_stride and out_dev + i*out_stride (4-byte aligned, strides >= N; out may alias pcm row for row);
 * workspace_dev >= ww_reverb_workspace_bytes(n_clips), 256-byte aligned. Its content on entry is unspecified and no result depends on it. */
WW_API int64_t ww_reverb_workspace_bytes(int64_t n_clips);
WW_API int ww_reverb_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t n_samples, const ww_augment_rir* rir_host,
                         const float* spectra_dev, int64_t n_rirs, float* out_dev, int64_t out_stride, void* workspace_dev, ww_stream_t stream);
/* The resampler's half-window (32769 floats: 64 zero crossings x 512 + 1) on the host, for checking on a CPU. */
WW_API int ww_kaiser_best_host(float* out_host);

/* ---- K1: log-mel front-end --------------------------------------------------------------- */
/* Replaces AudioProcessor.normalize_audio (:73-76), the zero-pad branch of pad_or_truncate
 * (:78-83) and AudioProcessor.audio_to_mel (:85-101) =
 * librosa.feature.melspectrogram + librosa.power_to_db(ref=np.max), batched.
 *   pcm_dev      [n_clips] rows of `clip_len` valid samples, row i at pcm_dev + i*clip_stride
 *                (floats; 16-byte aligned base, clip_stride % 4 == 0 -- ignored for a single clip --, 0 < clip_len <= 16000;
 *                shorter rows are right-zero-padded like pad_or_truncate does)
 *   normalize    != 0: divide the clip by max|x| first (process_audio_file order, :131-133);
 *                a silent clip then yields NaN, as the reference does
 *   logmel_dev   [n_clips][80][32]  (== the [B,1,80,32] tensor WakewordDataset.__getitem__ :204-216
 *                returns, batched), dB in [-80, 0] with per-clip max exactly 0
 * Non-finite samples: a clip with a NaN or an Inf among its clip_len samples gives NaN in EVERY output of its row, in all three
 * arithmetics and with either `normalize` -- what x / np.max(np.abs(x)) and power_to_db(ref=np.max) make of it (the per-clip maximum
 * is NaN once any mel power is NaN or Inf).  The other rows of the batch keep their bits; samples past clip_len are never read.
 * Signal level (normalize != 0): a gain of 2^k changes no output bit for |k| <= 31 in any arithmetic (int16 or int32 PCM may be passed
 * unscaled), in float64 mode for |k| <= 60 (tests/test_gpu_logmel_nonfinite.py).  Measured on MI355X (profiles/logmel_levels.json,
 * clips of peak 0.01 .. 1 times 2^k): float64 mode stays within 1e-4 dB of the reference for 2^-100 .. 2^100.  The float32 kernel
 * (float32 and auto mode) squares the raw samples and applies 1 / peak^2 to the mel powers: within 1e-4 dB for 2^-50 .. 2^50; at
 * 2^60 and beyond (powers or peak^2 overflow) and at 2^-70 and below (1 / peak^2 overflows) the row is all NaN; around 2^-60 the
 * powers go subnormal and auto mode gave a finite but wrong image for a noise-free clip.  Scale such material first, or use float64. */
WW_API int ww_logmel_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t clip_len,
                  int normalize, float* logmel_dev, ww_stream_t stream);

/* The same for any clip length (no ABI version bump: additions only):
 *   pcm_dev      rows of clip_len valid samples as above, 0 < clip_len <= n_samples; rows are right-zero-padded to n_samples
 *   n_samples    N in [WW_MIN_CLIP_SAMPLES, WW_MAX_CLIP_SAMPLES]; T = 1 + N / 512 frames
 *   logmel_dev   [n_clips][80][T], dB in [-80, 0], per-clip max (over all T frames) exactly 0
 * Same arithmetic modes (ww_set_logmel_math); N with T = 32 (16,000 samples among them) runs the 1 s kernel, bit for bit.
 * Non-finite samples and signal level: ww_logmel_f32's rules (a NaN or Inf among a row's clip_len samples: the whole row is NaN). */
WW_API int ww_logmel_frames_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t clip_len, int64_t n_samples,
                                int normalize, float* logmel_dev, ww_stream_t stream);

/* ---- SpecAugment: time and frequency masks on log-mel batches ------------- */
/* The one augmentation on the feature side of K1 (the reference has none): blocks of mel bands and blocks of frames of a clip are
 * replaced by one fill value.  mel_in / mel_out [n][80][width] float32 as K1 writes them, width = 1 .. WW_MAX_FRAMES, 16-byte aligned.
 * Each clip has one record of WW_SPEC_RECORD_INT16 int16 (ww_spec_augment_record_bytes() = 32 bytes, 16-byte aligned):
 *   [f_start, f_width] x WW_SPEC_MAX_MASKS, then [t_start, t_width] x WW_SPEC_MAX_MASKS; a width of 0 means no mask.
 * Position (row, col) of a clip is masked iff row lies in any [f_start, f_start + f_width) or col in any [t_start, t_start + t_width).
 * Masks may overlap and may cover the whole clip; what a record names outside the clip masks nothing.
 * Unmasked positions keep the input's bits.  Every masked position of a clip gets the same fill value:
 *   WW_SPEC_FILL_MEAN   the mean over all 80 width values of the clip BEFORE masking: float64 sums in an order that width alone fixes
 *                       (never the clip's place in the batch or n), rounded once to float32 -- within one float32 ulp of the exact mean
 *   WW_SPEC_FILL_MIN    the clip's minimum before masking (an fminf fold: a NaN is passed over)
 *   WW_SPEC_FILL_VALUE  fill_value
 * mel_out == mel_in is allowed: a clip without masks is then neither read nor written, only masked positions are written, and
 * WW_SPEC_FILL_VALUE reads nothing of the clip.  Buffers that overlap in any other way are WW_EINVAL.
 * Records: records_dev [n][16] filled by the caller, or NULL = drawn inside the kernel from a counter-based generator (splitmix64, the
 * stream of the training step's dropout masks), so that a batch costs the host one 64-bit seed.  With uint64 wrapping arithmetic:
 *   r(c, j) = fmix64(seed + 0x9E3779B97F4A7C15 * (32 c + j + 1))     fmix64: x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27,
 *                                                                            x *= 0x94D049BB133111EB, x ^= x >> 31
 *   int_in(r, m) = ((r >> 32) * (m + 1)) >> 32                       an integer in 0 .. m
 *   j = 0           u = float(r >> 40) * 2^-24; the clip is masked at all iff u < prob, otherwise its record is all zeros
 *   j = 1 + 2 i, 2 + 2 i   frequency mask i < n_freq: f_width = int_in(r, freq_max), f_start = int_in(r', 80 - f_width)
 *   j = 9 + 2 i, 10 + 2 i  time mask i < n_time:      t_width = int_in(r, time_max), t_start = int_in(r', width - t_width)
 * c is the clip's index in the batch: clip c's record does not depend on n.  ww_spec_augment_draw writes exactly those records (what a
 * caller or a test reads the plans back through, as ww_train_masks is for dropout).
 * Both launches are asynchronous, allocate and copy nothing and are capturable; n == 0 is WW_OK without a launch.  Checked before any
 * HIP call: width outside 1 .. WW_MAX_FRAMES (WW_EUNSUPPORTED); n outside 0 .. 2^30, a null or misaligned pointer, n_freq or n_time
 * outside 0 .. WW_SPEC_MAX_MASKS, freq_max outside 0 .. 80, time_max outside 0 .. width, prob outside [0, 1], an unknown fill mode,
 * partially overlapping buffers (WW_EINVAL).  The generator's arguments are checked with records_dev given too (pass zeros). */
#define WW_SPEC_MAX_MASKS 4
#define WW_SPEC_RECORD_INT16 16
#define WW_SPEC_FILL_MEAN 0
#define WW_SPEC_FILL_MIN 1
#define WW_SPEC_FILL_VALUE 2
WW_API int64_t ww_spec_augment_record_bytes(void);
WW_API int ww_spec_augment_draw(uint64_t seed, int64_t n, int32_t width, float prob, int32_t n_freq, int32_t freq_max, int32_t n_time,
                                int32_t time_max, int16_t* records_dev, ww_stream_t stream);
WW_API int ww_spec_augment_f32(const float* mel_in, float* mel_out, int64_t n, int32_t width, const int16_t* records_dev, uint64_t seed,
                               float prob, int32_t n_freq, int32_t freq_max, int32_t n_time, int32_t time_max, int32_t fill_mode,
                               float fill_value, ww_stream_t stream);

/* ---- Microphone-channel augmentation: random EQ, band limit, clipping ---- */
/* The waveform stage between the augmentation chain and K1 (the reference has none): a clip of N float32 samples goes through
 * WW_CHANNEL_SECTIONS second-order sections in a fixed order, then an optional saturator.  Section s is
 *   y[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] - a1 y[i-1] - a2 y[i-2]      (zero state before sample 0)
 * and [1, 0, 0, 0, 0] is the identity; slot 0 is a high-pass, 1 a low shelf, 2..5 peaks, 6 a high shelf, 7 a low-pass (RBJ "Audio EQ
 * Cookbook" forms at 16 kHz, normalised by a0; passes and shelves at Q = 1/sqrt(2)).  The saturator with drive d > 0:
 *   p = max |y| over the clip after the cascade (a NaN is passed over); out = p tanh(d y / p) / tanh(d); p == 0: out = y
 * Each clip has one record of WW_CHANNEL_RECORD_F32 float32 (ww_channel_record_bytes() = 192 bytes, 16-byte aligned):
 *   8 x [b0, b1, b2, a1, a2], then d, then 7 zeros.  Eight identity sections and d == 0 mean "off": with pcm_out == pcm_in such a clip
 *   is neither read nor written, otherwise it is copied bit for bit.
 * Records: records_dev [n][48] filled by the caller (cfg may then be NULL), or NULL = drawn inside the kernel from cfg and SpecAugment's
 * generator r(c, j) (above; c the clip's index in the batch, so clip c's record does not depend on n):
 *   on(j, P)  = float(r >> 40) * 2^-24 < P            u(j) = double(r >> 11) * 2^-53
 *   uniform   lo + u (hi - lo)                        log-uniform   lo * pow(hi / lo, u)            (float64; lo, hi the float32 fields)
 *   j = 0  the clip is touched at all (prob)          1, 2  high-pass on, f          3, 4, 5  low shelf on, f, gain dB
 *   6 + 4 i .. 9 + 4 i  peak i < peaks: on, f, gain dB, Q       22, 23, 24  high shelf on, f, gain dB
 *   25, 26  low-pass on, f                            27, 28  saturator on, d
 * Frequencies and Q are log-uniform, gains (within +-shelf_db, +-peak_db) and the drive uniform.  Coefficients are computed in float64 and
 * rounded once to float32.  ww_channel_draw writes exactly the records ww_channel_f32 draws with records_dev NULL.
 * Records the caller fills are trusted, not checked: poles outside the unit circle, NaN coefficients or a negative d give what the
 * recurrence and the saturator give for them (the launch stays in bounds and ends whatever they hold).
 * pcm rows: n rows of n_samples floats, row_stride floats apart (>= n_samples), the same for pcm_in and pcm_out; 4-byte aligned.
 * Both launches are asynchronous, allocate and copy nothing and are capturable; n == 0 is WW_OK without a launch.  Checked before any HIP
 * call: n_samples other than 16000 or 4000 .. 16383 (WW_EUNSUPPORTED); n outside 0 .. 2^30, a null or misaligned pointer, row_stride <
 * n_samples, buffers that overlap without being the same, a probability outside [0, 1], a frequency outside (0, 7600], a Q <= 0 or > 1e6,
 * peaks outside 0 .. 4, a drive outside [0, 8], a negative dB span, a reversed range or a non-finite field (WW_EINVAL). */
#define WW_CHANNEL_SECTIONS 8
#define WW_CHANNEL_MAX_PEAKS 4
#define WW_CHANNEL_RECORD_F32 48
typedef struct ww_channel_config {
    float prob;
    float highpass_prob, highpass_lo, highpass_hi;
    float low_shelf_prob, low_shelf_lo, low_shelf_hi;
    float high_shelf_prob, high_shelf_lo, high_shelf_hi;
    float shelf_db;
    float peak_prob, peak_lo, peak_hi, peak_db, peak_q_lo, peak_q_hi;
    float lowpass_prob, lowpass_lo, lowpass_hi;
    float drive_prob, drive_lo, drive_hi;
    int32_t peaks;
} ww_channel_config;
WW_API int64_t ww_channel_record_bytes(void);
WW_API int ww_channel_draw(uint64_t seed, int64_t n, const ww_channel_config* cfg, float* records_dev, ww_stream_t stream);
WW_API int ww_channel_f32(const float* pcm_in, float* pcm_out, int64_t n, int64_t n_samples, int64_t row_stride, const float* records_dev,
                          uint64_t seed, const ww_channel_config* cfg, ww_stream_t stream);

/* ---- weights ------------------------------------------------------------------------------ */
/* The reference state_dict (train_wakeword.py:28-36 / wakeword_training_script.py:141-165) as
 * host pointers in torch layout.  conv3_* are NULL for SimpleWakewordModel.  weight_hh_l* are not
 * part of the struct: with seq_len 1 and zero initial state they never reach the output. */
typedef struct ww_state_dict {
    int32_t n_conv;            /* 2 (SimpleWakewordModel) or 3 (WakewordModel) */
    int32_t hidden;            /* 256 */
    const float* conv_weight[3]; /* [32,1,3,3], [64,32,3,3], [128,64,3,3] */
    const float* conv_bias[3];   /* [32], [64], [128] */
    const float* lstm_weight_ih[2]; /* [4*hidden, C_last], [4*hidden, hidden]; gate order i,f,g,o */
    const float* lstm_bias_ih[2];   /* [4*hidden] */
    const float* lstm_bias_hh[2];   /* [4*hidden] */
    const float* fc_weight;         /* [2, hidden] */
    const float* fc_bias;           /* [2] */
} ww_state_dict;

/* Number of floats of the packed (kernel-layout) weight image for a model with n_conv convs. */
WW_API int64_t ww_packed_weights_floats(int32_t n_conv);
/* Pack on the host (pure CPU): MFMA B-operand order for the convs, transposed W_ih with the dead
 * forget-gate rows dropped, b_ih + b_hh pre-summed.  The caller uploads `packed_host` to HBM once
 * (model.load_state_dict / .to(device)) and passes the device copy to the functions below. */
WW_API int ww_pack_weights_host(const ww_state_dict* sd, float* packed_host);

/* ---- K2: conv stack + global average pool --------------------------------------------------- */
/* Replaces `x = F.relu(self.conv1(x)); x = F.relu(self.conv2(x)); [conv3]; x = self.pool(x)`
 * (train_wakeword.py:39-41 / wakeword_training_script.py:170-173).
 *   mel_dev    [n][80][width]   (the [B,1,80,T] model input), 1 <= width <= 32
 *   pooled_dev [n][C_last]      C_last = 64 (n_conv 2) or 128 (n_conv 3)
 *   scratch_dev  n_conv 3 only: ww_cnn_scratch_bytes(n, 3) bytes; may be NULL for n_conv 2. Its content on entry is unspecified and no result depends on it. */
WW_API int64_t ww_cnn_scratch_bytes(int64_t n, int32_t n_conv);
WW_API int ww_cnn_pool_f32(const float* mel_dev, int64_t n, int32_t width, const float* packed_dev,
                    int32_t n_conv, void* scratch_dev, float* pooled_dev, ww_stream_t stream);

/* K2 for mel images up to WW_MAX_FRAMES wide: mel_dev [n][80][width], 1 <= width <= 63, n <= 2^24.  Widths <= 32 run ww_cnn_pool_f32 (bit
 * for bit; scratch as there).  Wider images are covered by 32-column tiles that overlap by 2 h columns (h = 2 for n_conv 2, 3 for n_conv 3:
 * the reach of the conv stack); each tile runs the 32-wide kernels and pools only the columns it owns, with scale 1 / (80 width), and a
 * second kernel sums a clip's tiles in a fixed order (results do not depend on the batch).  Arithmetic: ww_set_conv_math (WW_CONV_MATH_F32
 * or WW_CONV_MATH_F16X3, whose range exponents are then chosen per tile); WW_CONV_MATH_F16X3_DIRECT has no tiled form: widths > 32 return
 * WW_EUNSUPPORTED under it.
 * scratch_dev: ww_cnn_wide_scratch_bytes(n, width, n_conv) bytes, 256-byte aligned (may be NULL only where ww_cnn_pool_f32 allows it). Its content on entry is unspecified and no result depends on it. */
WW_API int64_t ww_cnn_wide_scratch_bytes(int64_t n, int32_t width, int32_t n_conv);
WW_API int ww_cnn_pool_wide_f32(const float* mel_dev, int64_t n, int32_t width, const float* packed_dev, int32_t n_conv,
                                void* scratch_dev, float* pooled_dev, ww_stream_t stream);

/* ---- K3: 2-layer LSTM (one step, zero state) + Linear ---------------------------------------- */
/* Replaces `lstm_out, _ = self.lstm(x.unsqueeze(1)); x = lstm_out[:, -1, :]; x = self.fc(x)`
 * (train_wakeword.py:42-48 / wakeword_training_script.py:175-182), dropout = identity (eval).
 *   pooled_dev [n][C_last] -> logits_dev [n][2] */
WW_API int ww_lstm_fc_f32(const float* pooled_dev, int64_t n, const float* packed_dev, int32_t n_conv,
                   float* logits_dev, ww_stream_t stream);

/* ---- composed entry points ----------------------------------------------------------------- */
/* model.forward(x): SimpleWakewordModel.forward train_wakeword.py:38-49 /
 * WakewordModel.forward wakeword_training_script.py:167-184.  workspace >= ww_workspace_bytes. Its content on entry is unspecified and no result depends on it. */
WW_API int64_t ww_workspace_bytes(int64_t n, int32_t n_conv);
WW_API int ww_model_forward_f32(const float* mel_dev, int64_t n, int32_t width, const float* packed_dev,
                         int32_t n_conv, void* workspace_dev, float* logits_dev, ww_stream_t stream);
/* PCM -> logits: the eval loop body of wakeword_training.ipynb cell 17 / validate()
 * wakeword_training_script.py:269-289 with the Dataset's mel path folded in (K1 -> K2 -> K3).  workspace_dev as for
 * ww_model_forward_f32. Its content on entry is unspecified and no result depends on it. */
WW_API int ww_forward_pcm_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t clip_len,
                       int normalize, const float* packed_dev, int32_t n_conv, void* workspace_dev,
                       float* logits_dev, ww_stream_t stream);

/* PCM -> logits for any clip length: ww_logmel_frames_f32 -> ww_cnn_pool_wide_f32 -> ww_lstm_fc_f32 (arguments as there);
 * workspace_dev: ww_workspace_frames_bytes(n_clips, n_samples, n_conv) bytes, 256-byte aligned. Its content on entry is unspecified and no result depends on it. */
WW_API int64_t ww_workspace_frames_bytes(int64_t n, int64_t n_samples, int32_t n_conv);
WW_API int ww_forward_pcm_frames_f32(const float* pcm_dev, int64_t n_clips, int64_t clip_stride, int64_t clip_len, int64_t n_samples,
                                     int normalize, const float* packed_dev, int32_t n_conv, void* workspace_dev, float* logits_dev,
                                     ww_stream_t stream);

/* ---- long recordings: overlapping windows, events, thresholds ------------ */
/* Logits (and, if prob_dev is not NULL, softmax p(wakeword) as the streamer writes it) of n_windows windows of n_samples samples
 * (16000, or WW_MIN_CLIP_SAMPLES..WW_MAX_CLIP_SAMPLES) read in place from one signal: window k is the row at signal_dev + k * hop.
 * Rows may overlap: 4 <= hop <= n_samples, hop % 4 == 0, signal_dev 16-byte aligned, and the caller's buffer holds
 * (n_windows - 1) * hop + n_samples samples.  Nothing on the way writes the signal.  Bit for bit ww_forward_pcm_f32 (N = 16000) /
 * ww_forward_pcm_frames_f32 (other N) of the same windows copied out as rows.  workspace_dev: ww_forward_windows_workspace_bytes()
 * bytes, 256-byte aligned; workspace_bytes is its size. Its content on entry is unspecified and no result depends on it. */
WW_API int64_t ww_forward_windows_workspace_bytes(int64_t n_windows, int64_t n_samples, int32_t n_conv);
WW_API int ww_forward_windows_f32(const float* signal_dev, int64_t n_windows, int64_t hop, int64_t n_samples, int normalize,
                                  const float* packed_dev, int32_t n_conv, void* workspace_dev, int64_t workspace_bytes, float* logits_dev,
                                  float* prob_dev, ww_stream_t stream);
/* Event counts of n_segs recordings at n_thr thresholds.  prob_dev [n_windows] float32 per-window scores, segment g being windows
 * seg_offsets_dev[g] .. seg_offsets_dev[g + 1] - 1 (int64, non-decreasing, seg_offsets_dev[0] = 0, n_windows = seg_offsets_dev[n_segs];
 * the host reads nothing of it, the caller passes n_windows).  q = p where finite, else 0; s_k = the float64 mean of the segment's last
 * min(k, smooth) q values summed in ascending order (1 <= smooth <= 256); window k fires iff s_k >= (double)theta and no window of the
 * segment fired in the refractory windows before it (0 <= refractory <= 2^30).  counts_dev [n_segs][n_thr] int64; fired_dev (may be
 * NULL; only with n_thr == 1) [n_windows] uint8 0/1.  thresholds_dev [n_thr] float32, 1 <= n_thr <= 65536.
 * workspace_dev: ww_events_workspace_bytes(n_windows) bytes, 16-byte aligned. Its content on entry is unspecified and no result depends on it. */
WW_API int64_t ww_events_workspace_bytes(int64_t n_windows);
WW_API int ww_events_sweep_f32(const float* prob_dev, const int64_t* seg_offsets_dev, int64_t n_segs, int64_t n_windows, int32_t smooth,
                               int64_t refractory, const float* thresholds_dev, int32_t n_thr, int64_t* counts_dev, uint8_t* fired_dev,
                               void* workspace_dev, int64_t workspace_bytes, ww_stream_t stream);
/* The same rule one hop at a time for n_mics streams (StreamingDetector): state_dev of ww_events_state_bytes(n_mics, smooth) bytes,
 * 16-byte aligned, zeroed before the first hop; each call appends prob_dev [n_mics] and writes fired_dev [n_mics] uint8 0/1. */
WW_API int64_t ww_events_state_bytes(int32_t n_mics, int32_t smooth);
WW_API int ww_events_step_f32(const float* prob_dev, int32_t n_mics, int32_t smooth, float threshold, int64_t refractory, void* state_dev,
                              uint8_t* fired_dev, ww_stream_t stream);

/* ---- training clips in device memory ---------------------------------- */
/* A bank is one float32 device buffer audio_dev [total_samples] holding its entries back to back.
 * ww_bank_peaks_f32: peaks_dev[e] = the fmaxf-fold from 0.0f of fabsf(x) over entry e = samples offsets_dev[e] .. offsets_dev[e + 1] - 1
 * -- what K0 (ww_decode_resample with normalize) divides a file by: a NaN sample is ignored, an empty entry gives 0, an Inf gives Inf.
 * offsets_dev [n_entries + 1] int64 in device memory, non-decreasing, offsets_dev[0] = 0, offsets_dev[n_entries] <= total_samples
 * (ww_events_sweep_f32's convention; nothing at or past total_samples is read, whatever the table says).  The call zeroes peaks_dev
 * [n_entries] on the stream itself; its cost is linear in total_samples however the samples are split into entries, and the result does
 * not depend on the order the workgroups arrive in.  audio_dev / peaks_dev 4-byte, offsets_dev 8-byte aligned. */
WW_API int ww_bank_peaks_f32(const float* audio_dev, int64_t total_samples, const int64_t* offsets_dev, int64_t n_entries, float* peaks_dev,
                             ww_stream_t stream);
/* ww_bank_gather_f32: windows of N = n_samples samples cut from entries into rows of a batch.  For item i, row r = row, j in [0, N):
 *   v[j] = audio[offset + start + j] where 0 <= start + j < length; elsewhere out[r][j] is exactly +0.0f and is never divided
 *   WW_BANK_NORM_NONE    out = v
 *   WW_BANK_NORM_ENTRY   out = v / peak on the in-entry samples (IEEE division, K0's `o[w] / peak`: peak == 0 gives NaN there, as K0 does)
 *   WW_BANK_NORM_WINDOW  p = the fmaxf-fold from 0.0f of |v| over the window's in-entry samples, out = v / p; with p == 0 the row is all
 *                        zeros, NOT NaN -- a deliberate deviation from ENTRY: this is the normalisation the detector applies to every
 *                        window of a recording, where silent stretches are ordinary and must not poison a training step
 * out_dev [n_rows][out_stride] float32; rows that no item names, and the columns from N to out_stride, are not written.  items_host
 * [n_items] in host memory, checked before any HIP call (WW_EINVAL naming the field): N in WW_MIN_CLIP_SAMPLES..WW_MAX_CLIP_SAMPLES,
 * out_stride >= N, offset >= 0, length >= 0, offset + length <= total_samples, -N <= start <= length, a known norm, peak not negative,
 * 0 <= row < n_rows and no row named twice.  The items are staged through the library's pinned memory into workspace_dev
 * (>= ww_bank_gather_workspace_bytes(n_items), 256-byte aligned; its content on entry is unspecified and no result depends on it); the call is asynchronous on `stream` and cannot be captured into a
 * graph.  audio_dev / out_dev 4-byte aligned; entries and windows may start at any sample, and total_samples may exceed 2^31. */
#define WW_BANK_NORM_NONE 0
#define WW_BANK_NORM_ENTRY 1
#define WW_BANK_NORM_WINDOW 2
typedef struct ww_bank_item {
    int64_t offset; /* the entry's first sample in audio_dev */
    int64_t length; /* the entry's samples, >= 0 */
    int64_t start;  /* window start in entry coordinates, -N <= start <= length */
    float peak;     /* the divisor of WW_BANK_NORM_ENTRY (ww_bank_peaks_f32's value for the entry), >= 0 */
    int32_t row;    /* output row, 0 <= row < n_rows */
    int32_t norm;   /* WW_BANK_NORM_* */
    int32_t reserved;
} ww_bank_item;     /* 40 bytes */
WW_API int64_t ww_bank_gather_workspace_bytes(int64_t n_items);
WW_API int ww_bank_gather_f32(const float* audio_dev, int64_t total_samples, const ww_bank_item* items_host, int64_t n_items,
                              int64_t n_samples, float* out_dev, int64_t n_rows, int64_t out_stride, void* workspace_dev,
                              ww_stream_t stream);

/* ---- audit of a bank -------------------------------------------------- */
/* ww_bank_audit_f32: one pass over audio_dev [total_samples] and one record per entry e = samples offsets[e] .. offsets[e + 1] - 1
 * (len = their number, i = a sample's index in its entry, x its value, bits its float32 bit pattern).  This comment is the definition
 * of every field; the other documents point here.  A sample is non-finite when its exponent bits are all ones (Inf or NaN).
 *   nonfinite   the number of non-finite samples
 *   sum, sumsq  float64 sums of x and of x * x (exact in float64) over the finite samples; a non-finite sample adds 0
 *   clipped     the number of finite samples with fabsf(x) >= clip_level
 *   peak        ww_bank_peaks_f32's value for the entry, bit for bit: the fmaxf-fold from 0.0f of fabsf(x).  So a NaN adds nothing, and
 *               an Inf -- the one case where a non-finite sample shows outside `nonfinite` -- gives Inf, the divisor the gather uses
 *   hash        content hash, 64 bits: the wrapping uint64 sum over ALL samples of mix(bits, i), so partial sums combine in any order
 *               and the value does not depend on where the entry lies.  With uint32 wrapping arithmetic, lo = i mod 2^32, hi = i >> 32:
 *                 fmix32(x): x ^= x >> 16, x *= 0x85EBCA6B, x ^= x >> 13, x *= 0xC2B2AE35, x ^= x >> 16
 *                 m  = lo * 0x9E3779B1
 *                 k1 = bits ^ m ^ (hi * 0x85EBCA77)
 *                 k2 = bits + rotl32(m, 15) + hi * 0xC2B2AE3D + 0x27D4EB2F
 *                 mix(bits, i) = fmix32(k1) | fmix32(k2) << 32
 *               -0.0f and +0.0f differ, NaN payloads count.  An empty entry hashes to 0.  Equal (len, hash) is a filter for equal
 *               entries, not a proof: compare the samples before acting on it.
 *   active_start, active_end   the extent [a, b) of librosa.effects.trim(frame_length = 2048, hop_length = 512, centred, zero
 *               padded), stated in energies.  Hop block h of an entry is its samples [512 h, 512 h + 512), S[h] its float64 sum of
 *               squares as above, 0 for a block outside the entry.  Frame t, 0 <= t <= len / 512 (integer division), has energy
 *                 E_t = ((S[t - 2] + S[t - 1]) + S[t]) + S[t + 1]                     float64, added in that order
 *               and is active when E_max = max_t E_t > 0 and E_t > E_max * ratio, ratio = 10^(-top_db / 10) computed by the caller.
 *               a = 512 t_first, b = min(len, 512 (t_last + 1)) over the active frames; (0, 0) without one; (0, len) when
 *               nonfinite > 0.  This is librosa's rule (rms_t^2 = E_t / 2048, ref = max) except where librosa clamps an rms below
 *               1e-5 before taking the logarithm: there librosa treats a quieter frame as rms 1e-5, and this rule does not.
 *   max_frame_energy   E_max
 * sum and sumsq are added in a fixed order that depends on len alone: within a hop block lane l of 64 adds the samples 4 l .. 4 l + 3
 * and 256 + 4 l .. 256 + 4 l + 3 in that order and the lanes are added in a fixed xor tree; the blocks are then added in index order.
 * There are no float atomics, so every field is the same bits from run to run and wherever the entry lies in memory; sum and sumsq
 * differ from the exact sums by at most len * 2^-52 * sum |terms|.
 * offsets_dev [n_entries + 1] int64 in device memory and offsets_host the same values in host memory (the hop table is built from
 * them): non-decreasing, offsets[0] >= 0, offsets[n_entries] <= total_samples; nothing outside an entry is read, and nothing at or
 * past total_samples whatever the device table says.  stats_dev [n_entries] (8-byte aligned), every record written.  workspace_dev:
 * >= ww_bank_audit_workspace_bytes(total_samples, n_entries) bytes, 256-byte aligned. Its content on entry is unspecified and no result depends on it.  The hop table is staged through the library's
 * pinned memory; the call is asynchronous on `stream` and cannot be captured into a graph.  Checked before any HIP call (WW_EINVAL):
 * total_samples < 0, n_entries outside 0 .. 2^30, clip_level <= 0 or NaN, ratio outside (0, 1], the offsets as above, a null or
 * misaligned pointer.  n_entries == 0 is WW_OK without a launch. */
#define WW_AUDIT_HOP 512
#define WW_AUDIT_FRAME 2048
typedef struct ww_bank_entry_stats {
    double sum;
    double sumsq;
    double max_frame_energy;
    int64_t active_start;
    int64_t active_end;
    uint64_t hash;
    int64_t clipped;
    int64_t nonfinite;
    float peak;
    int32_t reserved;
} ww_bank_entry_stats; /* 72 bytes */
WW_API int64_t ww_bank_audit_workspace_bytes(int64_t total_samples, int64_t n_entries);
WW_API int ww_bank_audit_f32(const float* audio_dev, int64_t total_samples, const int64_t* offsets_dev, const int64_t* offsets_host,
                             int64_t n_entries, float clip_level, double ratio, ww_bank_entry_stats* stats_dev, void* workspace_dev,
                             ww_stream_t stream);

/* ---- training step ----------------------------------------------------- */
/* Replaces, for one batch, `output = model(data)` in train mode and `loss.backward()` of the reference's training loops
 * (wakeword_training/train_wakeword.py:109-115; WakewordTrainer.train_epoch, wakeword_training_script.py:241-267) for
 * SimpleWakewordModel and the 3-conv WakewordModel: the forward with nn.LSTM's inter-layer dropout and nn.Dropout before fc (train_wakeword.py:34-35,
 * 46-47), and d loss / d parameter given d loss / d logits.  CrossEntropyLoss and the optimiser stay with the caller.
 * Arithmetic: ww_set_train_math below (exact fp32, or the conv stack of the 2-conv model in split precision on the f16 / f64 matrix cores).
 * All pointers in the two structs are DEVICE pointers in torch layout (the live parameters
 * and their .grad buffers): nothing is packed on the host, the weights may change between calls.
 * Dropout factors come from a counter-based generator keyed by (seed, layer, clip, unit): the same seed reproduces the
 * step; torch's own random stream cannot be matched (documented, tests/test_gpu_train.py). */
typedef struct ww_train_params {
    int32_t n_conv;              /* 2 (SimpleWakewordModel) or 3 (WakewordModel) */
    int32_t hidden;              /* 256 */
    const float* conv_weight[3];
    const float* conv_bias[3];
    const float* lstm_weight_ih[2];
    const float* lstm_bias_ih[2];
    const float* lstm_bias_hh[2];
    const float* fc_weight;
    const float* fc_bias;
} ww_train_params;
typedef struct ww_train_grads {  /* outputs, overwritten (not accumulated) */
    float* conv_weight[3];       /* [32,1,3,3], [64,32,3,3], [128,64,3,3] (n_conv 3) */
    float* conv_bias[3];
    float* lstm_weight_ih[2];    /* [1024, 64 | 128], [1024, 256]; forget-gate rows come out zero like autograd's */
    float* lstm_bias[2];         /* [1024]: d/d bias_ih == d/d bias_hh; weight_hh gradients are exactly zero (h0 = 0): caller zero-fills */
    float* fc_weight;            /* [2, 256] */
    float* fc_bias;              /* [2] */
} ww_train_grads;
/* The arithmetic is part of every call of a step (ABI 4): train_math = WW_TRAIN_MATH_F32 | WW_TRAIN_MATH_F16X3 (below), or
 * WW_TRAIN_MATH_DEFAULT = the process-wide ww_set_train_math value read at that call.  The workspace LAYOUT depends on it (0.23 GB under
 * F16X3, 2.7 GB under F32 for 4096 clips of the 2-conv model), so forward and backward also take the size of the buffer they were given
 * and return WW_EINVAL when it is smaller than ww_train_workspace_bytes(n, n_conv, train_math) -- a mode switch between the size query and
 * the launch cannot write past the buffer; a backward under another mode than its forward is WW_EINVAL too. */
#define WW_TRAIN_MATH_DEFAULT (-1)
WW_API int64_t ww_train_workspace_bytes(int64_t n, int32_t n_conv, int32_t train_math);
/* mel_dev [n][80][width]; p_lstm / p_fc: drop probabilities (0 = eval-mode arithmetic); workspace_dev: workspace_bytes >=
 * ww_train_workspace_bytes bytes, 256-byte aligned, must stay untouched until the matching ww_train_backward_f32 has run; logits_dev [n][2].
 * The workspace's content on entry to the forward is unspecified and no result depends on it. */
WW_API int ww_train_forward_f32(const float* mel_dev, int64_t n, int32_t width, const ww_train_params* params, float p_lstm,
                                float p_fc, uint64_t seed, int32_t train_math, void* workspace_dev, int64_t workspace_bytes,
                                float* logits_dev, ww_stream_t stream);
WW_API int ww_train_backward_f32(const float* mel_dev, int64_t n, int32_t width, const ww_train_params* params,
                                 const float* dlogits_dev, int32_t train_math, void* workspace_dev, int64_t workspace_bytes,
                                 const ww_train_grads* grads, ww_stream_t stream);
/* Diagnostic: the dropout factors (0 or 1 / (1 - p)) the last forward on this workspace applied to the layer-0 output and to
 * fc's input, [n][256] each -- lets a test replay the step in another framework with the same masks. */
WW_API int ww_train_masks(const void* workspace_dev, int64_t n, int32_t n_conv, float* mask0_dev, float* mask1_dev, ww_stream_t stream);
/* Diagnostic: the packed image (ww_packed_weights_floats(2) floats) that the last WW_TRAIN_MATH_F16X3 forward of the 2-conv model wrote on
 * the device from the live parameters -- its conv1 / conv2-Winograd / range entries equal ww_pack_weights_host's bit for bit; the rest is 0. */
WW_API int ww_train_packed_image(const void* workspace_dev, int64_t n, int32_t n_conv, float* img_dev, ww_stream_t stream);
/* Diagnostic: what the last WW_TRAIN_MATH_F16X3 forward on this workspace kept of the activations instead of the activations themselves --
 * mask_last_dev [n][80][32][C/8] bytes, bit c of the position = [relu(last conv)[c] > 0] (C = 64 | 128, byte cb = channels 8 cb ..), in canonical
 * order (the kernels' own image holds the accumulator ballots); sign1_dev [n][80][32] words, bit c = [relu(conv1)[c] > 0]. */
WW_API int ww_train_bit_images(const void* workspace_dev, int64_t n, int32_t n_conv, uint8_t* mask_last_dev, uint32_t* sign1_dev, ww_stream_t stream);
/* Diagnostic, read-only: one intermediate of the step that last ran on this workspace (after its backward for the d... stages), copied to
 * out_dev; out_floats must be the stage's size.  train_math must be the arithmetic the workspace's forward ran under: a workspace no
 * forward of this process is on record for, or one written under the other arithmetic, is WW_EINVAL, and so is a stage that the model /
 * arithmetic does not keep, or a stage the backward writes (DHD1 .. DZ2) when no backward has run on the workspace since its last forward.
 * Shapes (H = 256, C = 64 | 128 channels of the last conv):
 *   POOLED [n][C]   GATES0/1 [4][n][H], planes sigmoid i, tanh g, sigmoid o, tanh c   HD0/1 [n][H] (LSTM outputs times their dropout factors)
 *   DHD1, DHD0 [n][H]   DG1, DG0 [n][4H] in torch's gate-row order i, f, g, o   DPOOLED, GP [n][C] (GP = DPOOLED / (80 width))
 *   DZ2 [n][80][64][32] (3-conv model: d loss / d conv2 pre-activation; under F16X3 decoded from the f16 halves with the per-clip scale applied)
 *   MID2 [n][80][64][32] relu(conv2) (F32; F16X3: 3-conv model only)   MID3 [n][80][128][32] relu(conv3) (F32, 3-conv model) */
#define WW_TRAIN_STAGE_POOLED 0
#define WW_TRAIN_STAGE_GATES0 1
#define WW_TRAIN_STAGE_GATES1 2
#define WW_TRAIN_STAGE_HD0 3
#define WW_TRAIN_STAGE_HD1 4
#define WW_TRAIN_STAGE_DHD1 5
#define WW_TRAIN_STAGE_DG1 6
#define WW_TRAIN_STAGE_DHD0 7
#define WW_TRAIN_STAGE_DG0 8
#define WW_TRAIN_STAGE_DPOOLED 9
#define WW_TRAIN_STAGE_GP 10
#define WW_TRAIN_STAGE_DZ2 11
#define WW_TRAIN_STAGE_MID2 12
#define WW_TRAIN_STAGE_MID3 13
WW_API int ww_train_stage(const void* workspace_dev, int64_t n, int32_t n_conv, int32_t train_math, int32_t stage, float* out_dev,
                          int64_t out_floats, ww_stream_t stream);
/* Arithmetic of the training step's convolution kernels (the head is always exact fp32); ww_set_train_math sets the process-wide DEFAULT that
 * WW_TRAIN_MATH_DEFAULT resolves to:
 *   WW_TRAIN_MATH_F32    exact fp32 matrix instructions throughout (v_mfma_f32_32x32x2_f32)
 *   WW_TRAIN_MATH_F16X3  (default) the conv stack in split precision on the f16 matrix instructions, for both models: forward = the
 *                        inference kernels with the ReLU masks as extra outputs (bit images); backward of the last conv: one operand
 *                        is the 0/1 mask, exact in f16, the other is carried as two f16 halves; below it both operands as two halves;
 *                        conv1's weight gradient in double on the f64 matrix instructions.  The head runs as under F32.
 *                        Gradients agree with F32 to the 2^-22 of the split. */
#define WW_TRAIN_MATH_F32 0
#define WW_TRAIN_MATH_F16X3 1
WW_API int ww_set_train_math(int mode);
WW_API int ww_get_train_math(void);

/* ---- loss, metrics and optimiser of the training loop ------------------ */
/* What WakewordTrainer.train_epoch (wakeword_training_script.py:241-267) does around forward and backward, as three kernels: nothing
 * here waits for the device, and every sum has one fixed order and uses no float atomics, so results repeat bit for bit from run to run.
 *
 * ww_ce_loss_f32: CrossEntropyLoss (mean reduction) over two classes, its gradient and the loop's running metrics.  Per clip, in float64:
 *   lse = max + log(exp(z0 - max) + exp(z1 - max)), loss = lse - z[y], prediction = 1 iff z1 > z0 (a tie gives 0, as torch.max(output, 1)).
 *   dlogits_dev [n][2] (NULL: the validation form, nothing is written) = (softmax - onehot) / n, rounded once: ww_train_backward_f32's input.
 *   loss_dev [1] (NULL allowed) = the batch mean: lane sums over fixed stripes of the batch, folded in a fixed order that does not depend
 *   on the launch geometry, in float64, rounded once to float32.
 *   stats_dev (NULL allowed): one lane adds this batch to the record, in stream order (calls on one stream serialise; calls on
 *   different streams must not share a record).  A label outside {0, 1} adds nothing to the loss or the gradient (its dlogits are
 *   exactly zero) and is counted in bad_labels; a clip with a non-finite logit is counted in nonfinite (its loss is what IEEE
 *   arithmetic makes of it, as in torch).  logits_dev [n][2] float32, labels_dev [n] int64; n in 1..2^30; 4-byte (labels, stats: 8-byte) alignment. */
typedef struct ww_loss_stats {
    double loss_sum;    /* sum of the batch means as float32 values: the reference's `running_loss += loss.item()` */
    int64_t correct;    /* clips whose prediction equals a valid label */
    int64_t total;      /* clips seen (`total += target.size(0)`) */
    int64_t batches;    /* calls */
    int64_t bad_labels; /* labels outside {0, 1} */
    int64_t nonfinite;  /* clips with an Inf or NaN logit */
} ww_loss_stats;        /* 48 bytes, DEVICE memory; zero it before an epoch */
WW_API int ww_ce_loss_f32(const float* logits_dev, const int64_t* labels_dev, int64_t n, float* dlogits_dev, float* loss_dev,
                          ww_loss_stats* stats_dev, ww_stream_t stream);
/* ww_ce_loss_ex_f32: the loss for imbalanced data -- ww_ce_loss_f32 with class weights, label smoothing,
 * ignore_index, a sum reduction and the focal loss.  One launch, no atomics, every sum in one fixed order; the options are read on the
 * HOST and travel by value in the kernel arguments, like the Adam table: nothing is uploaded.  Per clip in float64, with p = softmax(z),
 * y the label, w = class_weight, eps = label_smoothing, g = focal_gamma:
 *   y == ignore_index    tested FIRST (so ignore_index may be 0 or 1): nothing is added to loss, gradient or denominator; not a bad label.
 *   other y outside {0, 1}   as in ww_ce_loss_f32 (no loss, zero gradient, bad_labels += 1) and left out of the denominator too.
 *   WW_LOSS_CE     torch's F.cross_entropy(weight=w, label_smoothing=eps, ignore_index=):
 *                    l = (1 - eps) w[y] (-log p_y) + (eps / 2) sum_c w[c] (-log p_c)
 *                    dl/dz_k = (1 - eps) w[y] (p_k - [k == y]) + (eps / 2) ((w0 + w1) p_k - w[k])
 *                  WW_REDUCE_MEAN divides the sum of l and every gradient by W = sum over counted clips of w[y]; WW_REDUCE_SUM by 1.
 *   WW_LOSS_FOCAL  Lin et al. as torchvision reduces it, with q = the OTHER class's softmax term (never 1 - p_y):
 *                    l = w[y] q^g (-log p_y);  dl/dz_y = w[y] (g p_y q^g log p_y - q^(g+1));  dl/dz_other = -dl/dz_y
 *                  WW_REDUCE_MEAN divides by the NUMBER of counted clips.  label_smoothing must be 0.
 *   a denominator of 0 under WW_REDUCE_MEAN (every clip ignored, or only zero-weight classes present): the loss is NaN, as in torch, but
 *   every dlogits entry is exactly 0 -- unlike torch, whose gradient is NaN there: such a batch must not poison the weights.
 * Prediction, `correct` (an ignored clip is not correct) and `total += n` are ww_ce_loss_f32's; loss_sum adds the float32 value written to
 * loss_dev, the batch mean or the batch sum.  With unit weights, eps = 0 and nothing ignored the results have ww_ce_loss_f32's bits.
 * Pointers and n as for ww_ce_loss_f32.  Checked before any HIP call (WW_EINVAL naming the field): finite class_weight >= 0,
 * label_smoothing in [0, 1] (0 for the focal loss), finite focal_gamma >= 0, kind, reduction. */
#define WW_LOSS_CE 0
#define WW_LOSS_FOCAL 1
#define WW_REDUCE_MEAN 0
#define WW_REDUCE_SUM 1
typedef struct ww_loss_opts {
    double class_weight[2]; /* finite, >= 0 */
    double label_smoothing; /* [0, 1] */
    double focal_gamma;     /* >= 0; read by WW_LOSS_FOCAL only */
    int64_t ignore_index;   /* torch's default is -100 */
    int32_t kind;           /* WW_LOSS_CE or WW_LOSS_FOCAL */
    int32_t reduction;      /* WW_REDUCE_MEAN or WW_REDUCE_SUM */
} ww_loss_opts;             /* 48 bytes, HOST memory */
WW_API int ww_ce_loss_ex_f32(const float* logits_dev, const int64_t* labels_dev, int64_t n, const ww_loss_opts* opts_host, float* dlogits_dev,
                             float* loss_dev, ww_loss_stats* stats_dev, ww_stream_t stream);
/* ww_ce_loss_soft_f32: cross-entropy on CLASS PROBABILITIES -- torch's F.cross_entropy(z, t, weight=w,
 * label_smoothing=eps, reduction=) with a floating-point target t [n][2]: what mixup and soft relabelling need (distillation from a
 * teacher's LOGITS, with a temperature and a hard term in the same loss, is ww_distill_loss_f32 below).
 * ww_ce_loss_ex_f32's kernel shape: one launch, one workgroup, no atomics, every sum in one fixed order, the options by value in the
 * kernel arguments (opts_host NULL: unit weights, eps = 0, the mean).  Per clip in float64, with p = softmax(z) and lse as above:
 *   t'_c = (1 - eps) t_c + eps / 2;   l = w0 t'_0 (lse - z0) + w1 t'_1 (lse - z1);   dl/dz_k = p_k (w0 t'_0 + w1 t'_1) - w_k t'_k
 *   a row counts iff both its targets are finite and >= 0 (they need not sum to 1); any other row adds nothing to the loss or the
 *   denominator, its dlogits are exactly zero, and it is counted in bad_labels.
 *   WW_REDUCE_MEAN divides the sum of l and every gradient by the NUMBER of counted rows, as torch divides by n -- deliberately NOT
 *   the weighted denominator W of the integer-label form above: with class weights the two means differ, as they do in torch.
 *   WW_REDUCE_SUM divides by 1.  A denominator of 0 under the mean: a NaN loss and an all-zero gradient, as in ww_ce_loss_ex_f32.
 * Prediction, total, batches, nonfinite and loss_sum follow ww_ce_loss_f32; a counted clip is `correct` iff prediction == (t1 > t0):
 * a tie in the target gives class 0, the prediction's rule.  With one-hot rows, unit weights and eps = 0 the loss, the gradient and the
 * record have the bits of ww_ce_loss_f32 on the corresponding labels, under both reductions.
 * logits_dev, targets_dev [n][2] float32; pointers and n as for ww_ce_loss_f32 (4-byte alignment, stats 8-byte; dlogits / loss / stats
 * may be NULL).  Checked before any HIP call (WW_EINVAL naming the field): the range checks of ww_ce_loss_ex_f32, kind != WW_LOSS_CE,
 * ignore_index != -100 (torch refuses one for floating-point targets). */
WW_API int ww_ce_loss_soft_f32(const float* logits_dev, const float* targets_dev, int64_t n, const ww_loss_opts* opts_host, float* dlogits_dev,
                               float* loss_dev, ww_loss_stats* stats_dev, ww_stream_t stream);
/* ww_distill_loss_f32: knowledge distillation -- a hard term on the batch's own targets and Hinton's
 * teacher term in ONE loss, one launch in the place of ww_ce_loss_ex_f32 / ww_ce_loss_soft_f32 and in their kernel shape: one workgroup,
 * no atomics, every sum in one fixed order, the options, alpha and the temperature by value in the kernel arguments.  With z the student
 * logits, zt the teacher logits, T = temperature and alpha the mixing weight:
 *   L = (1 - alpha) H(z, y) + alpha T^2 KD(z, zt)
 *   KD_i = sum_c q_c (log q_c - log p_c),  q = softmax(zt_i / T),  p = softmax(z_i / T);   dKD_i / dz_k = (p_k - q_k) / T
 * which is F.kl_div(log_softmax(z / T), softmax(zt / T), reduction="batchmean") * T^2.  zt / T and z / T are formed in float64 and go
 * through the max-subtracted log-sum-exp of the other losses; log q_c = zt_c / T - lse, never log(q_c).
 *   H          target_kind WW_TARGET_LABELS: targets_dev is int64 [n] and H is ww_ce_loss_ex_f32's loss under *opts_host, per clip and
 *              in its denominator (class weights, smoothing, ignore_index, focal, mean or sum); opts_host NULL: unit weights, eps = 0,
 *              ignore_index -100, cross-entropy, the mean.  WW_TARGET_PROBS: targets_dev is float32 [n][2] and H is ww_ce_loss_soft_f32's.
 *              targets_dev NULL: no target at all (unlabelled audio) -- L = T^2 KD, alpha and target_kind are not read, and of the
 *              options only `reduction` is.
 *   KD rows    a row counts for KD iff both its teacher logits are finite; any other row adds nothing to KD or its gradient and is
 *              counted in teacher_nonfinite.
 *   mean       H is divided by its rule's own denominator and KD by the NUMBER of KD rows; WW_REDUCE_SUM divides both by 1.
 *   dlogits    (1 - alpha) dH/dz / (H's denominator) + alpha T (p - q) / (KD's denominator), in float64, rounded to float32 once.
 *   a term without a counted row (a denominator of 0 under the mean), or with coefficient 0, contributes exactly 0 to loss and gradient
 *   -- selected, never multiplied: 0 x NaN is not formed.  When NEITHER term has a counted row under the mean the loss is NaN and every
 *   dlogits entry exactly 0, the rule of ww_ce_loss_ex_f32; under WW_REDUCE_SUM such a batch sums to 0, as there.
 *   alpha = 0  loss, gradient and *stats_dev have the bits of ww_ce_loss_ex_f32 / ww_ce_loss_soft_f32 on the same inputs.
 * stats_dev is updated as the hard rule's own entry point updates it (loss_sum adds the float32 L); without a target only total,
 * batches, nonfinite and loss_sum move.  distill_stats_dev (NULL allowed) accumulates what tells the two terms apart.
 * logits_dev, teacher_logits_dev [n][2] float32, 4-byte aligned (16-byte loads where a pointer allows them); labels and both records
 * 8-byte aligned; dlogits_dev, loss_dev, stats_dev and distill_stats_dev may be NULL.  Checked before any HIP call (WW_EINVAL naming the
 * field): what ww_ce_loss_ex_f32 (labels) or ww_ce_loss_soft_f32 (probabilities) checks, target_kind, alpha in [0, 1], a finite
 * temperature > 0, a NULL teacher_logits_dev. */
#define WW_TARGET_LABELS 0
#define WW_TARGET_PROBS 1
typedef struct ww_distill_stats {
    double hard_sum;           /* sum over the batches of H as a float32 value, NOT weighted by 1 - alpha (0 for a batch without hard rows) */
    double kd_sum;             /* the same of T^2 KD, NOT weighted by alpha */
    int64_t kd_rows;           /* rows with two finite teacher logits */
    int64_t hard_rows;         /* rows the hard rule counts (a valid label that is not ignored; a valid probability row) */
    int64_t agree;             /* KD rows where the student's prediction equals the teacher's (a tie gives class 0, as everywhere) */
    int64_t teacher_correct;   /* hard rows where the TEACHER's prediction equals the label (the argmax of a probability row) */
    int64_t teacher_nonfinite; /* rows with an Inf or NaN teacher logit */
    int64_t batches;           /* calls */
} ww_distill_stats;            /* 64 bytes, DEVICE memory; zero it before an epoch */
WW_API int ww_distill_loss_f32(const float* logits_dev, const float* teacher_logits_dev, const void* targets_dev, int target_kind, int64_t n,
                               const ww_loss_opts* opts_host, double alpha, double temperature, float* dlogits_dev, float* loss_dev,
                               ww_loss_stats* stats_dev, ww_distill_stats* distill_stats_dev, ww_stream_t stream);
/* ww_hard_select_f32: online hard example mining -- rank the n rows of a candidate batch by the per-clip loss
 * the step's criterion would compute and name the `keep` hardest.  One launch of one workgroup, no wait, no float atomics (integer LDS
 * atomics fill histograms, whose result does not depend on order): the same bytes from run to run.
 *   score    the row's loss in float64 BEFORE the mean's division: ww_ce_loss_f32's rule with integer labels and opts_host NULL,
 *            ww_ce_loss_ex_f32's with integer labels and options (class weights, smoothing, ignore_index, focal; the reduction is not
 *            read), ww_ce_loss_soft_f32's with WW_TARGET_PROBS (opts_host NULL: its defaults) -- the same device functions.
 *   order    1. rank class, descending: 2 for a counting row of class keep_class (for probabilities the class is t1 > t0) with finite
 *               logits and a finite score; 1 for any other counting row with finite logits and a finite score; 0 for the rest -- an
 *               ignored or bad label, an invalid probability row, a non-finite logit or score
 *            2. score, descending        3. row index, ascending
 *   sel_dev [keep] int64: the first `keep` rows of that order, listed in RISING ROW INDEX (keep == n: 0 .. n - 1).
 *   scores_dev [n] float64 (NULL allowed): the scores; -inf for a rank-0 row.
 *   stats_dev (NULL allowed): one lane adds this call to the record, in stream order, as for ww_loss_stats.
 *   workspace_dev: ww_hard_select_workspace_bytes(n) bytes, 256-byte aligned; nothing outside the n rows, the keep outputs and it is touched.
 * logits_dev [n][2] float32 and probabilities [n][2] float32 need 4-byte alignment, labels [n] int64, sel, scores and stats 8-byte.
 * Checked before any HIP call (WW_EINVAL naming the field): 1 <= keep <= n <= 65536, keep_class in {-1, 0, 1}, target_kind, the options as
 * the loss entry points check them, null or misaligned pointers.
 *
 * ww_select_rows_f32: row sel_dev[j] -> row j, j < keep, of each tensor whose source and output are both given (a pair may be NULL, not
 * all four): mel [n][80][width] float32, the targets of either kind, entries [n] and labels [n] int64.  One launch; 16-byte accesses where
 * the row size and both mel pointers allow them, single floats otherwise -- the same bits.  An index outside [0, n) writes a row of zeros
 * and reads nothing.  Out of place: an output that overlaps its source is WW_EINVAL, as are n outside 1..2^30, keep outside 1..n and
 * null or misaligned pointers; width outside 1..32 is WW_EUNSUPPORTED. */
typedef struct ww_select_stats {
    int64_t batches;            /* calls */
    int64_t candidates;         /* rows scored (sum of n) */
    int64_t kept;               /* rows selected (sum of keep) */
    int64_t candidate_positive; /* counting rows of class 1 among the candidates (whatever their rank) */
    int64_t kept_positive;      /* ... among the selected */
    int64_t unranked;           /* rank-0 rows among the candidates */
    int64_t kept_unranked;      /* rank-0 rows that were selected: nothing else was left */
    int64_t threshold_bits;     /* NOT a sum: the float64 bits of the smallest selected score of the newest call (-inf: a rank-0 row) */
} ww_select_stats;              /* 64 bytes, DEVICE memory; zero it before an epoch */
WW_API int64_t ww_hard_select_workspace_bytes(int64_t n);
WW_API int ww_hard_select_f32(const float* logits_dev, const void* targets_dev, int target_kind, int64_t n, int64_t keep,
                              const ww_loss_opts* opts_host, int32_t keep_class, int64_t* sel_dev, double* scores_dev,
                              ww_select_stats* stats_dev, void* workspace_dev, ww_stream_t stream);
WW_API int ww_select_rows_f32(const float* mel_dev, int64_t n, int32_t width, const int64_t* sel_dev, int64_t keep, float* mel_out,
                              const void* targets_dev, int target_kind, void* targets_out, const int64_t* entries_dev, int64_t* entries_out,
                              const int64_t* labels_dev, int64_t* labels_out, ww_stream_t stream);
/* ww_mixup_f32: mixup on a log-mel batch, with the class-probability targets ww_ce_loss_soft_f32 takes.
 * Out of place (overlapping mel / out ranges: WW_EINVAL); one launch over B x chunks of a row; no atomics.  Per row i, with
 * p = partner_dev[i], lam = lambda_dev[i] and oml = 1.0f - lam (ONE float32 subtraction):
 *   lam == 1.0f, or p outside [0, B)   out[i] is a bit-exact copy of mel[i]; row p is not read
 *   otherwise                          out[i] = fmaf(lam, mel[i], oml * mel[p]) element by element, the product rounded once
 *   targets_dev[i]                     (NaN, NaN) when labels[i] lies outside {0, 1}, when p lies outside [0, B) (whatever lam is), or
 *                                      when the row is mixed and labels[p] lies outside {0, 1}: the loss then counts a bad label;
 *                                      else the exact one-hot of labels[i] when the row is not mixed or labels[p] == labels[i];
 *                                      else t[labels[i]] = lam, t[labels[p]] = oml.
 * The kernel clamps nothing and forms no address from an unchecked index: p is compared against the B ARGUMENT before mel[p] or
 * labels[p] is touched.  mel_dev, out_dev [B][80][T] float32 (16-byte accesses when both are 16-byte aligned, else one float at a
 * time: the same bits), labels_dev [B] int64, partner_dev [B] int32, lambda_dev [B] float32, targets_dev [B][2] float32.
 * Checked before any HIP call (WW_EINVAL naming the field): B in 1..2^30, T in 1..WW_MAX_FRAMES, null pointers, 4-byte (labels:
 * 8-byte) alignment, overlap. */
WW_API int ww_mixup_f32(const float* mel_dev, float* out_dev, int64_t B, int32_t T, const int64_t* labels_dev, const int32_t* partner_dev,
                        const float* lambda_dev, float* targets_dev, ww_stream_t stream);
/* ww_adam_step_f32: one launch of torch's single-tensor Adam (no amsgrad, no maximize) over up to WW_ADAM_MAX_TENSORS tensors.  The table
 * is read on the HOST and travels in the kernel arguments: nothing is uploaded.
 *   g' = g * scale + weight_decay * p;  m += (g' - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g'^2;
 *   p -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * with the bias corrections computed on the host in double.  scale = *grad_scale_dev, read by the kernel (NULL: 1) -- ww_grad_norm_f32
 * writes it, so clipping costs no host wait.  Two entries may share one g (bias_ih and bias_hh have the same gradient); the p, m and v
 * ranges of the table must not overlap one another.  p, g, m, v: device pointers, 4-byte aligned (16-byte accesses where the four share
 * their phase on the 16-byte grid).  Checked before any HIP call (WW_EINVAL naming the field): 1 <= n_tensors <= 16, n >= 1, no null
 * pointer, finite lr >= 0, betas in [0, 1), finite eps > 0, finite weight_decay >= 0, step >= 1. */
#define WW_ADAM_MAX_TENSORS 16
typedef struct ww_adam_tensor {
    float* p;       /* parameter, updated in place */
    const float* g; /* gradient, read only */
    float* m;       /* exp_avg */
    float* v;       /* exp_avg_sq */
    int64_t n;      /* elements */
} ww_adam_tensor;   /* 40 bytes */
WW_API int ww_adam_step_f32(const ww_adam_tensor* tensors_host, int64_t n_tensors, double lr, double beta1, double beta2, double eps,
                            double weight_decay, int64_t step, const float* grad_scale_dev, ww_stream_t stream);
/* Averaged weights: an exponential moving average (EMA) or an equal-weight average (SWA) of the parameters, kept as one more float32
 * tensor per parameter.  One rule, used by both entries: a = the averaged value, p = the parameter as stored
 * (after this step's Adam update), w = avg_weight, rounded ONCE on the host to w32 = (float)w and omw32 = (float)(1 - w):
 *   w == 1      a = p            a copy: a is NOT read, so a NaN or uninitialised average is simply overwritten
 *   w == 0      a keeps its bits: nothing is read or written for it (ww_adam_avg_step_f32 then is ww_adam_step_f32)
 *   w32 < 0.5   a = fmaf(w32, p - a, a)
 *   otherwise   a = fmaf(-omw32, p - a, p)
 * which is torch.lerp(a, p, w) with its threshold, each branch an explicit fma, so the bits do not depend on what a compiler contracts
 * and are the same on the 16-byte and on the one-float path.  The schedule -- which w an update gets -- is the caller's
 * (average.update_weight: 1 on the first update, then 1 - decay for an EMA or 1 / (n + 1) for SWA).
 * ww_adam_avg_step_f32: ww_adam_step_f32 with the rule applied to the register value of every p it stores, in the same launch:
 * avg_host[k] (HOST array of n_tensors DEVICE pointers, read on the host like the table) is the average of tensors_host[k].  36 bytes per
 * element against Adam's 28.  p, m and v get ww_adam_step_f32's bits; the average is accessed 16 bytes at a time where it shares the phase
 * of p, g, m and v on the 16-byte grid, one float at a time otherwise, with the same bits.
 * ww_weight_average_f32: the rule alone, one launch over up to 16 tensors; only p and n of an entry are read (g, m, v may be anything).
 * For per-epoch SWA, for parameters that got no gradient in a step, and for optimisers other than Adam.
 * Checked before any HIP call (WW_EINVAL naming the field): everything ww_adam_step_f32 checks (the second entry: n_tensors, n, p);
 * avg_weight finite and in [0, 1]; avg_host not NULL, every average pointer not NULL and 4-byte aligned; no average's range [a, a + n)
 * overlapping another average or any p, m, v or g range of the table (the second entry: any p range). */
WW_API int ww_adam_avg_step_f32(const ww_adam_tensor* tensors_host, float* const* avg_host, int64_t n_tensors, double lr, double beta1,
                                double beta2, double eps, double weight_decay, int64_t step, const float* grad_scale_dev, double avg_weight,
                                ww_stream_t stream);
WW_API int ww_weight_average_f32(const ww_adam_tensor* tensors_host, float* const* avg_host, int64_t n_tensors, double avg_weight,
                                 ww_stream_t stream);
/* ww_grad_norm_f32: *norm_dev = the L2 norm over every g of the table (an entry counts once per entry, as clip_grad_norm_ counts a
 * gradient once per parameter), float64 partial sums over 4096 elements each in a fixed order in element coordinates, added by a second
 * kernel; *scale_dev = min(1, max_norm / (norm + 1e-6)), clip_grad_norm_'s coefficient.  Only g and n of the entries are read.
 * workspace_dev: >= ww_grad_norm_workspace_bytes(...) bytes, 256-byte aligned. Its content on entry is unspecified and no result depends on it.  max_norm > 0 (infinity: the norm alone). */
WW_API int64_t ww_grad_norm_workspace_bytes(const ww_adam_tensor* tensors_host, int64_t n_tensors);
WW_API int ww_grad_norm_f32(const ww_adam_tensor* tensors_host, int64_t n_tensors, double max_norm, double* norm_dev, float* scale_dev,
                            void* workspace_dev, ww_stream_t stream);

/* ---- post-training weight quantisation: symmetric int8 per group ------------------------------------------ */
/* ww_quant_weights_f32: one launch over up to WW_QUANT_MAX_TENSORS tensors; the table is read on the HOST and travels in the kernel
 * arguments.  Nothing waits, nothing is allocated, there are no atomics.  A tensor is rows x cols float32, contiguous, and a row is one
 * quantisation group with one scale: an output channel of a conv weight (cols = Cin * 9), a gate row of an LSTM matrix, a row of
 * fc.weight, or the whole tensor (rows = 1).  With qmax = 2^(bits - 1) - 1, every operation in float32 and rounded to nearest once:
 *   amax  = max |w| over the row's finite elements (0 when it has none)
 *   scale = max(amax / qmax, 2^-126)                   one division; the floor keeps the next one finite
 *   q     = clamp(rint(w / scale), -qmax, qmax)        one division, ties to even; a non-finite w gives q = 0 and is counted in bad
 *   deq   = (float)q * scale                           one multiplication; -0.0 and every non-finite w give +0.0
 * err[row] = { sum of w^2, sum of (w - deq)^2, max |w - deq| } in float64 over the row's finite elements, in a fixed order: the same
 * call writes the same bytes every time.  Rows of up to 1024 elements take a wave each, longer rows a workgroup each; no row is split
 * across workgroups.  q, deq, err and bad may each be NULL.  w, scale, deq, bad: 4-byte aligned (longer rows use 16-byte accesses where
 * a row starts on the 16-byte grid, with the same bits); err: 8-byte aligned.
 * Checked before any HIP call (WW_EINVAL naming the field): n_tensors in 1..16, bits in 2..8, tensors_host, w and scale not NULL, rows
 * and cols in 1..2^30 with rows x cols <= 2^40, the alignments, deq not overlapping w. */
#define WW_QUANT_MAX_TENSORS 16
typedef struct ww_quant_tensor {
    const float* w;  /* [rows][cols], read only */
    float* scale;    /* [rows] */
    int8_t* q;       /* [rows][cols] or NULL */
    float* deq;      /* [rows][cols] or NULL: the fake-quant weights */
    double* err;     /* [rows][3] or NULL */
    int32_t* bad;    /* [rows] or NULL: non-finite elements of the row */
    int64_t rows;
    int64_t cols;
} ww_quant_tensor;   /* 64 bytes, DEVICE pointers */
WW_API int ww_quant_weights_f32(const ww_quant_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream);

/* ---- clipped scales and the straight-through estimator: quantisation-aware training ---------------------- */
/* A clipped scale gives up a row's outliers for a finer step.  Candidate j in 0 .. WW_QUANT_CLIP_STEPS - 1 has the fraction
 * f_j = (64 - j) / 64, exact in float32: 1.0 down to 17/64.  With amax and qmax as above, every operation float32 and rounded once:
 *   scale_j = max((amax * f_j) / qmax, 2^-126)         one multiplication, one division
 *   r       = rint(w / scale_j)                        ties to even; a non-finite w counts as 0 and goes to bad
 *   sat     = |r| > qmax                               the clamp moved this element
 *   q       = clamp(r, -qmax, qmax);  deq = (float)q * scale_j
 * j = 0 multiplies amax by 1.0f: it is ww_quant_weights_f32 bit for bit.
 * All three entry points below are one launch over up to WW_QUANT_MAX_TENSORS tensors with the table in the kernel arguments: no
 * atomics, no wait, no allocation, no row split across workgroups (rows of up to 1024 elements take a wave, longer rows a workgroup),
 * the same bytes for the same call.  Arguments are checked before any HIP call (WW_EINVAL naming the field): what
 * ww_quant_weights_f32 checks for the fields the two structs share, and the new fields as said below.
 *
 * ww_quant_weights_clip_f32: ww_quant_weights_f32 with one clip index per row, uint8 in DEVICE memory (an index above 47 counts as 47;
 * it is not read on the host), and one more optional output: sat [rows], the row's saturated elements.  clip not NULL; sat 4-byte aligned.
 *
 * ww_quant_clip_search_f32: per row, cand_err[row][j] = the float64 sum of (w - deq_j)^2 over the row's finite elements for all 48
 * candidates, in ww_quant_weights_f32's order of summation (so cand_err[row][0] is its err[row][1] bit for bit); clip[row] = the smallest j
 * whose cand_err is the minimum of the written values; scale[row] = that candidate's scale.  cand_err may be NULL; q, deq, err, bad and
 * sat are not read or written.  clip (written here) and scale not NULL; cand_err 8-byte aligned.  A workgroup per long row carries 48
 * float64 sums per thread: per-tensor mode is slow (scripts/bench_qat.py measures it) and is not on a per-step path.
 *
 * ww_quant_ste_f32: the straight-through estimator with clipping.  tensors[k] = { w, scale (read), g (modified in place), rows, cols }:
 * where w is finite and |rint(w / scale[row])| > qmax, g becomes +0.0 (a select: a NaN gradient there becomes 0 too); everywhere else,
 * every non-finite w included, g keeps its bits.  w, scale, g not NULL and 4-byte aligned; g must not overlap w. */
#define WW_QUANT_CLIP_STEPS 48
typedef struct ww_quant_clip_tensor {
    const float* w;   /* [rows][cols], read only */
    float* scale;     /* [rows] */
    int8_t* q;        /* [rows][cols] or NULL */
    float* deq;       /* [rows][cols] or NULL */
    double* err;      /* [rows][3] or NULL */
    int32_t* bad;     /* [rows] or NULL */
    uint8_t* clip;    /* [rows]: read by ww_quant_weights_clip_f32, written by ww_quant_clip_search_f32 */
    int32_t* sat;     /* [rows] or NULL: saturated elements of the row (ww_quant_weights_clip_f32) */
    double* cand_err; /* [rows][WW_QUANT_CLIP_STEPS] or NULL (ww_quant_clip_search_f32) */
    int64_t rows;
    int64_t cols;
} ww_quant_clip_tensor;   /* 88 bytes, DEVICE pointers */
typedef struct ww_quant_ste_tensor {
    const float* w;     /* [rows][cols], read only */
    const float* scale; /* [rows], read only: what the clipped launch stored */
    float* g;           /* [rows][cols], modified in place */
    int64_t rows;
    int64_t cols;
} ww_quant_ste_tensor;    /* 40 bytes, DEVICE pointers */
WW_API int ww_quant_weights_clip_f32(const ww_quant_clip_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream);
WW_API int ww_quant_clip_search_f32(const ww_quant_clip_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream);
WW_API int ww_quant_ste_f32(const ww_quant_ste_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream);

/* ---- clip evaluation: confusion, operating points and a margin histogram as device counters ---------- */
/* What notebook cell 17 collects clip by clip on the host (`all_preds.extend(predicted.cpu().numpy())`) kept as integer counters in
 * device memory: one launch per batch adds the batch to the record in stream order, nothing waits for the device, and the record is read
 * once.  Accuracy, precision / recall / F1, the confusion matrix, a ROC curve, AUC, EER and "the threshold for a false-positive rate"
 * are all functions of these integers (metrics.py).  Every sum is an integer sum: the record after a set of clips does not depend on the
 * batch size, the launch geometry or the order of the clips.
 *
 * Per clip, with z = logits [2] float32, y = label int64 and the margin d = z1 - z0 (ONE float32 subtraction):
 *   y outside {0, 1}        bad_labels += 1 and nothing else (total counts it: total = clips seen, as ww_loss_stats.total).
 *   argmax[y][pred] += 1    pred = 1 iff z1 > z0; a tie or a NaN gives 0 -- ww_ce_loss_f32's rule, so (argmax[0][0] + argmax[1][1]) is
 *                           its `correct` integer for integer.
 *   d NaN or +-inf          nonfinite += 1 (it is counted in argmax too) and none of the margin counters below.
 *   at[k][y][fired] += 1    for each of the n_thresholds operating points: fired = 1 iff d >= margin[k], compared in float32.
 *                           margin[k] = (float)log(p / (1 - p)) of the probability threshold p, evaluated in double
 *                           (ww_clip_metrics_margin_host).  d >= margin is softmax(z)[1] >= p except within rounding of the boundary:
 *                           the rule is defined on the margin, where float32 still resolves p beyond 0.9999999.
 *   hist[y][bin] += 1       bin = clamp((int)floorf((d + 32.0f) * 64.0f), 0, 4095): bins 1/64 wide over [-32, 32), the end bins take
 *                           everything beyond.  The multiply by 64 is exact, so float32 arithmetic anywhere reproduces the bin bit for bit.
 * One workgroup per call; a call's histogram is built in LDS (integer LDS adds) and one lane per touched bin adds it to the record with
 * a plain read-modify-write: calls on one stream serialise, calls on different streams must not share a record.  No float atomics, no
 * global atomics.
 *
 * ww_clip_metrics_init writes the margins of thresholds_host [n_thresholds] (each in (0, 1); they travel in the kernel arguments, the
 * host array is free on return) and zeroes every counter; ww_clip_metrics_reset zeroes the counters and keeps the margins.
 * ww_clip_metrics_update_f32 is a pure launch: no allocation, no copy, no synchronise, capturable; n == 0 returns WW_OK without a launch.
 * logits_dev [n][2] float32, 8-byte aligned; labels_dev [n] int64; state_dev: ww_clip_metrics_bytes() bytes, 8-byte aligned; n in 0..2^30.
 * Checked before any HIP call (WW_EINVAL naming the field): n < 0, null or misaligned pointers, n_thresholds outside
 * 0..WW_METRICS_MAX_THRESHOLDS, a threshold outside (0, 1) or NaN. */
#define WW_METRICS_MAX_THRESHOLDS 8
#define WW_METRICS_BINS 4096
typedef struct ww_clip_metrics {
    int64_t argmax[2][2];                              /* [label][prediction at argmax]: [[tn, fp], [fn, tp]] */
    int64_t total;                                     /* clips seen, bad labels included */
    int64_t batches;                                   /* calls with n > 0 */
    int64_t bad_labels;                                /* labels outside {0, 1} */
    int64_t nonfinite;                                 /* valid-label clips whose margin is NaN or +-inf */
    int64_t at[WW_METRICS_MAX_THRESHOLDS][2][2];       /* [k][label][fired at margin[k]] */
    int64_t hist[2][WW_METRICS_BINS];                  /* [label][bin of the margin] */
    float margin[WW_METRICS_MAX_THRESHOLDS];           /* the operating points, unused entries 0 */
    int32_t n_thresholds;
    int32_t reserved;
} ww_clip_metrics;                                     /* 65896 bytes, DEVICE memory */
WW_API int64_t ww_clip_metrics_bytes(void);
/* NaN (and ww_last_error names p) for p outside (0, 1). */
WW_API float ww_clip_metrics_margin_host(float p);
WW_API int ww_clip_metrics_init(ww_clip_metrics* state_dev, const float* thresholds_host, int32_t n_thresholds, ww_stream_t stream);
WW_API int ww_clip_metrics_reset(ww_clip_metrics* state_dev, ww_stream_t stream);
WW_API int ww_clip_metrics_update_f32(const float* logits_dev, const int64_t* labels_dev, int64_t n, ww_clip_metrics* state_dev,
                                      ww_stream_t stream);

/* ---- clip ledger: a per-clip training record as device integers ---------------------------------------- */
/* Which clips does the model never learn, which does it keep forgetting, which labels are probably wrong?  All of it follows from the
 * margin of the ASSIGNED class at every visit of a clip: its mean over training (the area under the margin; negative for likely label
 * errors), its spread, and the epochs in which the clip was classified wrongly.  A ledger keeps that per bank entry in device memory:
 * one launch per batch scatters the batch's rows into it in stream order, nothing waits for the device, and it is read once.
 *
 * A ledger is ONE device buffer: a ww_ledger_header followed by n_entries ww_ledger_entry records, ww_clip_ledger_bytes(n_entries)
 * = 64 + 56 n_entries bytes, 8-byte aligned.
 *
 * Per row i of a call, with z = logits [2] float32, y = label int64 and e = entry int64:
 *   always                  rows += 1
 *   e < 0                   skipped += 1 and nothing else: a caller marks placeholder rows this way.
 *   e >= n_entries          bad_entries += 1 and NO write to any record.  Compared as int64 against the n_entries ARGUMENT (the kernel
 *                           never reads a device value to decide where it may write): e = 2^32 + 1 is out of range, not entry 1.
 *   y outside {0, 1}        bad_labels += 1 and nothing else.
 * otherwise, on record e:
 *   d = z1 - z0             ONE float32 subtraction; pred = 1 iff z1 > z0 (a tie or a NaN gives 0: ww_ce_loss_f32's rule); m = y ? d : -d,
 *                           the margin of the assigned class.
 *   seen += 1; correct += (pred == y)
 *   epoch >= 0              seen_epochs |= 1 << epoch, and when pred != y also wrong_epochs |= 1 << epoch (64-bit shifts)
 *   m NaN or +-inf          the record's nonfinite += 1 and the header's nonfinite += 1; none of the margin fields below
 *   m finite                Q = (int32)rintf(fminf(fmaxf(m, -64.f), 64.f) * 65536.f): the margin in units of 2^-16, clamped to +-64.  The
 *                           multiply is exact and rintf rounds half to even, so float32 arithmetic anywhere reproduces Q bit for bit.
 *                           sum_q += Q; sum_q2 += (uint64)((int64)Q * Q); min_q = min(min_q, Q); max_q = max(max_q, Q)
 * The header's updates += 1 once per call with n > 0.
 *
 * One lane per row, workgroups of 256, ceil(n / 256) workgroups.  A batch may name an entry more than once and its rows are spread over
 * workgroups, so the records are updated with INTEGER global atomics at device scope (add, min, max, or): each is commutative and
 * associative, so the ledger after a set of rows does not depend on row order, batch split, launch geometry or run.  No float atomics,
 * no compare-and-swap loops.  The header counters are counted per wave with ballots: one atomic per wave and counter.  Calls on one
 * stream serialise; nothing is promised for two streams that share a ledger.
 *
 * ww_clip_ledger_init writes the header and clears every record (min_q = INT32_MAX, max_q = INT32_MIN, the rest 0); it does not depend on
 * what the buffer held.  ww_clip_ledger_update_f32 is a pure launch: no allocation, no copy, no synchronise, capturable; n == 0 returns
 * WW_OK without a launch.  logits_dev [n][2] float32, labels_dev [n] and entries_dev [n] int64; epoch in 0..63, or -1 for "no epoch bit".
 * Checked before any HIP call (WW_EINVAL naming the field): null pointers; logits_dev, labels_dev, entries_dev or ledger_dev not 8-byte
 * aligned; n outside 0..2^30; n_entries outside 0..2^28; epoch outside -1..63.  ww_clip_ledger_bytes returns WW_EINVAL for n_entries
 * outside 0..2^28. */
typedef struct ww_ledger_header {
    int64_t n_entries;      /* as given to ww_clip_ledger_init; for the reader, never read by a kernel */
    int64_t updates;        /* calls with n > 0 */
    int64_t rows;           /* rows seen, whatever became of them */
    int64_t skipped;        /* rows with e < 0 */
    int64_t bad_entries;    /* rows with e >= n_entries */
    int64_t bad_labels;     /* rows of a valid entry with a label outside {0, 1} */
    int64_t nonfinite;      /* scored rows whose margin is NaN or +-inf */
    int64_t reserved;
} ww_ledger_header;         /* 64 bytes, DEVICE memory */
typedef struct ww_ledger_entry {
    int64_t sum_q;          /* sum of Q over the finite visits */
    uint64_t sum_q2;        /* sum of Q * Q */
    uint64_t seen_epochs;   /* bit k: visited in epoch k */
    uint64_t wrong_epochs;  /* bit k: classified wrongly at some visit of epoch k */
    int32_t seen;           /* visits, non-finite ones included */
    int32_t correct;        /* visits with pred == y */
    int32_t nonfinite;      /* visits with a non-finite margin */
    int32_t min_q;          /* INT32_MAX until a finite visit */
    int32_t max_q;          /* INT32_MIN until a finite visit */
    int32_t reserved;
} ww_ledger_entry;          /* 56 bytes, DEVICE memory */
WW_API int64_t ww_clip_ledger_bytes(int64_t n_entries);
WW_API int ww_clip_ledger_init(void* ledger_dev, int64_t n_entries, ww_stream_t stream);
WW_API int ww_clip_ledger_update_f32(const float* logits_dev, const int64_t* labels_dev, const int64_t* entries_dev, int64_t n, int32_t epoch,
                                     void* ledger_dev, int64_t n_entries, ww_stream_t stream);

/* ---- streaming: sliding window of 0.25 .. 1 s, one hop per step, many microphones ------------- */
/* Semantics per window = predict_wakeword (wakeword_training.ipynb cell 19): normalise the last
 * N samples, log-mel, forward, softmax, p[wakeword].  The reference has no streaming code;
 * this is that function applied to every hop of every microphone.
 * The per-hop step (ring append -> K1 -> K2 -> K3 -> softmax) is captured once into a hipGraph and
 * replayed by ww_streamer_step. */
typedef struct ww_streamer ww_streamer;
/* A 1 s window: ww_streamer_create_n(n_mics, hop_samples, 16000, ...). */
WW_API int ww_streamer_create(int32_t n_mics, int32_t hop_samples, const float* packed_dev, int32_t n_conv,
                       ww_stream_t stream, ww_streamer** out);
/* A window of n_samples = N samples: 16000, or WW_MIN_CLIP_SAMPLES <= N <= WW_AUG_MAX_SAMPLES (0.25 s .. 32 frames, the lengths
 * the model trains at; T = 1 + N / 512 in [8, 32]); any other N is WW_EUNSUPPORTED.  hop_samples must be a multiple of 4 that
 * divides N (WW_EINVAL otherwise), which keeps N and the ring position multiples of 4.  The length is checked before the hop,
 * and both before any HIP call.  Each hop recomputes the T frames of the whole window. */
WW_API int ww_streamer_create_n(int32_t n_mics, int32_t hop_samples, int32_t n_samples, const float* packed_dev, int32_t n_conv,
                                ww_stream_t stream, ww_streamer** out);
/* hop_dev [n_mics][hop_samples] new samples; prob_dev [n_mics] softmax p(wakeword) of the window
 * ending at this hop; logits_dev (may be NULL) [n_mics][2]. */
WW_API int ww_streamer_step(ww_streamer* s, const float* hop_dev, float* prob_dev, float* logits_dev);
/* Copy of the current window of every mic, oldest sample first: [n_mics][N] (for tests). */
WW_API int ww_streamer_window(ww_streamer* s, float* window_dev);
WW_API int ww_streamer_destroy(ww_streamer* s);

/* A streamer fed at the microphone's own rate, sample format and channel count.  sample_rate: any rate K0 takes (1000 .. 384000 Hz);
 * format: WW_FMT_S16, S24, S32, F32, U8 or F64 (not FLAC); channels: 1 .. 8, frames interleaved as in a WAV data chunk.  With
 * (up, down) = ww_resample_taps_host(sample_rate), hop_frames * up must be a multiple of down and the 16 kHz hop
 * hop_frames * up / down must satisfy ww_streamer_create_n's rule (a multiple of 4 that divides N).  The window length is checked
 * first (WW_EUNSUPPORTED), then rate, format, channels and hop (WW_EINVAL), all before any HIP call.
 * The window holds exactly what K0 computes, without normalisation, for a file of every frame pushed so far (bit for bit: the same
 * conversion, the same filter, the same fused multiply-add order), delayed by ww_streamer_latency() samples at 16 kHz: the
 * outputs whose filter still reaches frames that have not arrived.  At (16000, WW_FMT_F32, 1) this is ww_streamer_create_n's
 * streamer, the same graph node for node. */
WW_API int ww_streamer_create_input(int32_t n_mics, int32_t hop_frames, int32_t sample_rate, int32_t format, int32_t channels,
                                    int32_t n_samples, const float* packed_dev, int32_t n_conv, ww_stream_t stream, ww_streamer** out);
/* hop_dev [n_mics][hop_frames][channels] in the streamer's sample format, aligned to its sample size (1 byte for U8 and S24);
 * prob_dev and logits_dev as for ww_streamer_step.  Also takes a streamer of ww_streamer_create_n (float32 mono hops). */
WW_API int ww_streamer_step_input(ww_streamer* s, const void* hop_dev, float* prob_dev, float* logits_dev);
/* D: the 16 kHz samples the window lags the input by (0 at 16 kHz); a negative WW_E* for a null handle. */
WW_API int ww_streamer_latency(const ww_streamer* s);

#ifdef __cplusplus
}
#endif
#endif /* WAKEWORD_AMD_H */
