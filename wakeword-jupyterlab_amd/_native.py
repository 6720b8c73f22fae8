"""ctypes binding of libwakeword_amd.so (the C ABI declared in include/wakeword_amd.h).

The shared library is the ONLY implementation of the hot path: importing this module fails loudly
when it has not been built (`python -c "import __graft_entry__ as g; g.build()"` or
`make -C wakeword-jupyterlab_amd/csrc`), and every launch fails with WW_ENODEVICE when no gfx950
device is visible.  There is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

# torch first: it carries its own libamdhip64 (SONAME libamdhip64.so.7).  Loading ours afterwards makes the
# dynamic loader bind libwakeword_amd.so to that SAME runtime instance, so torch's streams, allocations and
# device pointers are valid inside the library.  The other order would leave two HIP runtimes in the process.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WW_LIB_OVERRIDE") or os.path.join(_HERE, "libwakeword_amd.so")   # override: ablation builds only

WW_OK, WW_EINVAL, WW_ENODEVICE, WW_EHIP, WW_EUNSUPPORTED, WW_ENOSPACE = 0, -1, -2, -3, -4, -5
ABI_VERSION = 4


class NativeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libwakeword_amd: {msg} (code {code})")
        self.code = code


# the model's parameters in torch layout, as ww_state_dict (host pointers) and ww_train_params (device pointers) both declare them
_MODEL_FIELDS = [
    ("n_conv", C.c_int32), ("hidden", C.c_int32),
    ("conv_weight", C.c_void_p * 3), ("conv_bias", C.c_void_p * 3),
    ("lstm_weight_ih", C.c_void_p * 2), ("lstm_bias_ih", C.c_void_p * 2), ("lstm_bias_hh", C.c_void_p * 2),
    ("fc_weight", C.c_void_p), ("fc_bias", C.c_void_p),
]


class StateDict(C.Structure):
    """struct ww_state_dict (include/wakeword_amd.h)."""
    _fields_ = _MODEL_FIELDS


class TrainParams(C.Structure):
    """struct ww_train_params: DEVICE pointers, torch layout."""
    _fields_ = _MODEL_FIELDS


class TrainGrads(C.Structure):
    """struct ww_train_grads: DEVICE output pointers."""
    _fields_ = [
        ("conv_weight", C.c_void_p * 3), ("conv_bias", C.c_void_p * 3),
        ("lstm_weight_ih", C.c_void_p * 2), ("lstm_bias", C.c_void_p * 2),
        ("fc_weight", C.c_void_p), ("fc_bias", C.c_void_p),
    ]


class ClipDesc(C.Structure):
    """struct ww_clip_desc (include/wakeword_amd.h)."""
    _fields_ = [
        ("byte_offset", C.c_int64), ("n_frames", C.c_int64), ("channels", C.c_int32), ("sample_rate", C.c_int32),
        ("format", C.c_int32), ("crop_start", C.c_int32), ("up", C.c_int32), ("down", C.c_int32),
        ("half_len", C.c_int32), ("_pad", C.c_int32), ("taps_dev", C.c_void_p),
    ]


class AugmentPlan(C.Structure):
    """struct ww_augment_plan (include/wakeword_amd.h)."""
    _fields_ = [
        ("shift", C.c_int32), ("crop_start", C.c_int32), ("pitch_rate", C.c_double), ("stretch_rate", C.c_double),
        ("noise_sigma", C.c_float), ("noise_seed", C.c_uint32),
    ]


class AugmentLayout(C.Structure):
    """struct ww_augment_layout (include/wakeword_amd.h): byte offsets and strides of the augmentation workspace's regions."""
    _fields_ = [(k, C.c_int64) for k in ("records", "buf_a", "buf_b", "spec", "y", "record_bytes", "row_bytes", "spec_clip_bytes",
                                         "spec_step_bytes", "y_clip_bytes", "total_bytes")]


class AugmentBg(C.Structure):
    """struct ww_augment_bg (include/wakeword_amd.h): one clip's background segment."""
    _fields_ = [
        ("file_offset", C.c_int64), ("file_len", C.c_int64), ("start", C.c_int64), ("snr_db", C.c_float), ("enabled", C.c_int32),
    ]


class AugmentRir(C.Structure):
    """struct ww_augment_rir (include/wakeword_amd.h): one clip's room impulse response."""
    _fields_ = [
        ("index", C.c_int64), ("dpos", C.c_int32), ("taps", C.c_int32), ("enabled", C.c_int32), ("reserved", C.c_int32),
    ]


class BankItem(C.Structure):
    """struct ww_bank_item (include/wakeword_amd.h): one window of a bank entry and the output row it goes to."""
    _fields_ = [
        ("offset", C.c_int64), ("length", C.c_int64), ("start", C.c_int64), ("peak", C.c_float), ("row", C.c_int32), ("norm", C.c_int32),
        ("reserved", C.c_int32),
    ]


BANK_NORM_NONE, BANK_NORM_ENTRY, BANK_NORM_WINDOW = 0, 1, 2


class BankEntryStats(C.Structure):
    """struct ww_bank_entry_stats (include/wakeword_amd.h): what ww_bank_audit_f32 writes per entry, DEVICE memory."""
    _fields_ = [
        ("sum", C.c_double), ("sumsq", C.c_double), ("max_frame_energy", C.c_double), ("active_start", C.c_int64), ("active_end", C.c_int64),
        ("hash", C.c_uint64), ("clipped", C.c_int64), ("nonfinite", C.c_int64), ("peak", C.c_float), ("reserved", C.c_int32),
    ]


AUDIT_HOP, AUDIT_FRAME = 512, 2048
SPEC_RECORD_INT16 = 16
SPEC_FILL_MEAN, SPEC_FILL_MIN, SPEC_FILL_VALUE = 0, 1, 2
CHANNEL_SECTIONS, CHANNEL_MAX_PEAKS, CHANNEL_RECORD_F32 = 8, 4, 48


class ChannelConfig(C.Structure):
    """struct ww_channel_config (include/wakeword_amd.h): what the channel stage's generator draws a record from."""
    _fields_ = [(k, C.c_float) for k in (
        "prob", "highpass_prob", "highpass_lo", "highpass_hi", "low_shelf_prob", "low_shelf_lo", "low_shelf_hi", "high_shelf_prob",
        "high_shelf_lo", "high_shelf_hi", "shelf_db", "peak_prob", "peak_lo", "peak_hi", "peak_db", "peak_q_lo", "peak_q_hi", "lowpass_prob",
        "lowpass_lo", "lowpass_hi", "drive_prob", "drive_lo", "drive_hi")] + [("peaks", C.c_int32)]


class LossStats(C.Structure):
    """struct ww_loss_stats (include/wakeword_amd.h): the running metrics of an epoch, kept in device memory."""
    _fields_ = [("loss_sum", C.c_double), ("correct", C.c_int64), ("total", C.c_int64), ("batches", C.c_int64), ("bad_labels", C.c_int64),
                ("nonfinite", C.c_int64)]


class LossOpts(C.Structure):
    """struct ww_loss_opts (include/wakeword_amd.h): what ww_ce_loss_ex_f32 computes, HOST memory."""
    _fields_ = [("class_weight", C.c_double * 2), ("label_smoothing", C.c_double), ("focal_gamma", C.c_double), ("ignore_index", C.c_int64),
                ("kind", C.c_int32), ("reduction", C.c_int32)]


LOSS_CE, LOSS_FOCAL = 0, 1
REDUCE_MEAN, REDUCE_SUM = 0, 1
TARGET_LABELS, TARGET_PROBS = 0, 1


class DistillStats(C.Structure):
    """struct ww_distill_stats (include/wakeword_amd.h): what tells the two terms of a distillation epoch apart, device memory."""
    _fields_ = [("hard_sum", C.c_double), ("kd_sum", C.c_double), ("kd_rows", C.c_int64), ("hard_rows", C.c_int64), ("agree", C.c_int64),
                ("teacher_correct", C.c_int64), ("teacher_nonfinite", C.c_int64), ("batches", C.c_int64)]


class SelectStats(C.Structure):
    """struct ww_select_stats (include/wakeword_amd.h): what loss-ranked selection did over an epoch, device memory."""
    _fields_ = [(k, C.c_int64) for k in ("batches", "candidates", "kept", "candidate_positive", "kept_positive", "unranked", "kept_unranked",
                                         "threshold_bits")]


SELECT_MAX_ROWS = 65536


class AdamTensor(C.Structure):
    """struct ww_adam_tensor (include/wakeword_amd.h): one entry of the Adam / gradient-norm table, DEVICE pointers."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64)]


ADAM_MAX_TENSORS = 16


class QuantTensor(C.Structure):
    """struct ww_quant_tensor (include/wakeword_amd.h): one entry of the weight-quantisation table, DEVICE pointers."""
    _fields_ = [("w", C.c_void_p), ("scale", C.c_void_p), ("q", C.c_void_p), ("deq", C.c_void_p), ("err", C.c_void_p), ("bad", C.c_void_p),
                ("rows", C.c_int64), ("cols", C.c_int64)]


class QuantClipTensor(C.Structure):
    """struct ww_quant_clip_tensor (include/wakeword_amd.h): ww_quant_tensor's fields, then clip, sat and cand_err, DEVICE pointers."""
    _fields_ = [("w", C.c_void_p), ("scale", C.c_void_p), ("q", C.c_void_p), ("deq", C.c_void_p), ("err", C.c_void_p), ("bad", C.c_void_p),
                ("clip", C.c_void_p), ("sat", C.c_void_p), ("cand_err", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int64)]


class QuantSteTensor(C.Structure):
    """struct ww_quant_ste_tensor (include/wakeword_amd.h): one entry of the straight-through estimator's table, DEVICE pointers."""
    _fields_ = [("w", C.c_void_p), ("scale", C.c_void_p), ("g", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int64)]


QUANT_MAX_TENSORS = 16
QUANT_CLIP_STEPS = 48
METRICS_MAX_THRESHOLDS, METRICS_BINS = 8, 4096


class ClipMetrics(C.Structure):
    """struct ww_clip_metrics (include/wakeword_amd.h): the counters of a clip evaluation, kept in device memory."""
    _fields_ = [("argmax", C.c_int64 * 2 * 2), ("total", C.c_int64), ("batches", C.c_int64), ("bad_labels", C.c_int64),
                ("nonfinite", C.c_int64), ("at", C.c_int64 * 2 * 2 * METRICS_MAX_THRESHOLDS), ("hist", C.c_int64 * METRICS_BINS * 2),
                ("margin", C.c_float * METRICS_MAX_THRESHOLDS), ("n_thresholds", C.c_int32), ("reserved", C.c_int32)]


class LedgerHeader(C.Structure):
    """struct ww_ledger_header (include/wakeword_amd.h): the counters in front of a clip ledger's records, DEVICE memory."""
    _fields_ = [(k, C.c_int64) for k in ("n_entries", "updates", "rows", "skipped", "bad_entries", "bad_labels", "nonfinite", "reserved")]


class LedgerEntry(C.Structure):
    """struct ww_ledger_entry (include/wakeword_amd.h): one bank entry's record of a clip ledger, DEVICE memory."""
    _fields_ = [("sum_q", C.c_int64), ("sum_q2", C.c_uint64), ("seen_epochs", C.c_uint64), ("wrong_epochs", C.c_uint64),
                ("seen", C.c_int32), ("correct", C.c_int32), ("nonfinite", C.c_int32), ("min_q", C.c_int32), ("max_q", C.c_int32),
                ("reserved", C.c_int32)]


LEDGER_MAX_ENTRIES, LEDGER_MAX_EPOCHS = 1 << 28, 64

RIR_MAX_TAPS, RIR_FFT_SIZE, RIR_SPECTRUM_BINS = 16384, 32768, 16385


FMT_S16, FMT_S24, FMT_S32, FMT_F32, FMT_U8, FMT_F64, FMT_FLAC = 1, 2, 3, 4, 5, 6, 7
WAV_STATUS = {1: "ok", -1: "cannot open", -2: "not a RIFF/WAVE or FLAC file",
              -3: "missing fmt/data chunk, or a damaged FLAC stream (STREAMINFO, frame header or CRC)", -4: "unsupported WAV / FLAC encoding",
              -5: "read error", -6: "staging buffer full"}

# name -> (restype, argtypes); kept in one table so tests can check it against the header
PROTOTYPES = {
    "ww_abi_version": (C.c_int, []),
    "ww_last_error": (C.c_char_p, []),
    "ww_init": (C.c_int, []),
    "ww_set_conv_math": (C.c_int, [C.c_int]),
    "ww_get_conv_math": (C.c_int, []),
    "ww_set_conv_math_thread": (C.c_int, [C.c_int]),
    "ww_set_logmel_math_thread": (C.c_int, [C.c_int]),
    "ww_set_train_math": (C.c_int, [C.c_int]),
    "ww_get_train_math": (C.c_int, []),
    "ww_set_logmel_math": (C.c_int, [C.c_int]),
    "ww_get_logmel_math": (C.c_int, []),
    "ww_device_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "ww_sync_timeouts": (C.c_int, []),
    "ww_flac_errors": (C.c_int, []),
    "ww_mel_filterbank_host": (C.c_int, [C.c_void_p]),
    "ww_hann_window_host": (C.c_int, [C.c_void_p]),
    "ww_resample_taps_host": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ww_resampler_prepare": (C.c_int, [C.c_int32, C.POINTER(ClipDesc)]),
    "ww_decode_resample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "ww_wav_reader_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    "ww_wav_reader_staging": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "ww_wav_probe_host": (C.c_int, [C.c_char_p, C.POINTER(ClipDesc)]),
    "ww_wav_reader_destroy": (C.c_int, [C.c_void_p]),
    "ww_read_wav_batch_host": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int64, C.c_int32, C.POINTER(C.POINTER(ClipDesc)), C.c_void_p,
                                         C.POINTER(C.c_int64)]),
    "ww_wav_batch_decode": (C.c_int, [C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p]),
    "ww_wav_batch_decode_n": (C.c_int, [C.c_void_p, C.c_int32, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_wav_batch_stage": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "ww_decode_resample_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_augment_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ww_augment_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(AugmentPlan), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_augment_record_bytes": (C.c_int64, []),
    "ww_augment_plans_prepare": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "ww_augment_records_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_augment_n_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "ww_augment_workspace_layout": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(AugmentLayout)]),
    "ww_augment_n_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(AugmentPlan), C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p]),
    "ww_augment_plans_prepare_n": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "ww_augment_records_n_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_void_p]),
    "ww_augment_bg_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "ww_augment_bg_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(AugmentPlan), C.POINTER(AugmentBg), C.c_void_p,
                                    C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_augment_bg_record_bytes": (C.c_int64, []),
    "ww_augment_bg_prepare": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "ww_augment_bg_records_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_mix_background_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ww_mix_background_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(AugmentBg), C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_rir_spectra_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ww_rir_spectra_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_augment_rir_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "ww_augment_rir_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(AugmentPlan), C.POINTER(AugmentBg), C.c_void_p,
                                     C.c_int64, C.POINTER(AugmentRir), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_augment_rir_record_bytes": (C.c_int64, []),
    "ww_augment_rir_prepare": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "ww_augment_rir_records_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_reverb_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ww_reverb_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(AugmentRir), C.c_void_p, C.c_int64, C.c_void_p,
                                C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_kaiser_best_host": (C.c_int, [C.c_void_p]),
    "ww_logmel_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "ww_packed_weights_floats": (C.c_int64, [C.c_int32]),
    "ww_pack_weights_host": (C.c_int, [C.POINTER(StateDict), C.c_void_p]),
    "ww_cnn_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "ww_cnn_pool_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_lstm_fc_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ww_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "ww_model_forward_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_forward_pcm_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_logmel_frames_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "ww_cnn_wide_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "ww_cnn_pool_wide_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_workspace_frames_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "ww_forward_pcm_frames_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "ww_forward_windows_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "ww_forward_windows_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_events_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ww_events_sweep_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ww_events_state_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "ww_events_step_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_bank_peaks_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_bank_gather_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ww_bank_gather_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                     C.c_void_p]),
    "ww_bank_audit_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "ww_bank_audit_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_double, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "ww_spec_augment_record_bytes": (C.c_int64, []),
    "ww_spec_augment_draw": (C.c_int, [C.c_uint64, C.c_int64, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p]),
    "ww_spec_augment_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_uint64, C.c_float, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "ww_channel_record_bytes": (C.c_int64, []),
    "ww_channel_draw": (C.c_int, [C.c_uint64, C.c_int64, C.POINTER(ChannelConfig), C.c_void_p, C.c_void_p]),
    "ww_channel_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_uint64, C.POINTER(ChannelConfig),
                                 C.c_void_p]),
    "ww_train_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "ww_train_forward_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(TrainParams), C.c_float, C.c_float, C.c_uint64, C.c_int32,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_train_backward_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(TrainParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                        C.POINTER(TrainGrads), C.c_void_p]),
    "ww_ce_loss_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_ce_loss_ex_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(LossOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_ce_loss_soft_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(LossOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_distill_loss_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.POINTER(LossOpts), C.c_double, C.c_double,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_hard_select_workspace_bytes": (C.c_int64, [C.c_int64]),
    "ww_hard_select_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(LossOpts), C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_select_rows_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_mixup_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_adam_step_f32": (C.c_int, [C.POINTER(AdamTensor), C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64,
                                   C.c_void_p, C.c_void_p]),
    "ww_adam_avg_step_f32": (C.c_int, [C.POINTER(AdamTensor), C.POINTER(C.c_void_p), C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double,
                                       C.c_double, C.c_int64, C.c_void_p, C.c_double, C.c_void_p]),
    "ww_weight_average_f32": (C.c_int, [C.POINTER(AdamTensor), C.POINTER(C.c_void_p), C.c_int64, C.c_double, C.c_void_p]),
    "ww_grad_norm_workspace_bytes": (C.c_int64, [C.POINTER(AdamTensor), C.c_int64]),
    "ww_grad_norm_f32": (C.c_int, [C.POINTER(AdamTensor), C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_quant_weights_f32": (C.c_int, [C.POINTER(QuantTensor), C.c_int64, C.c_int, C.c_void_p]),
    "ww_quant_weights_clip_f32": (C.c_int, [C.POINTER(QuantClipTensor), C.c_int64, C.c_int, C.c_void_p]),
    "ww_quant_clip_search_f32": (C.c_int, [C.POINTER(QuantClipTensor), C.c_int64, C.c_int, C.c_void_p]),
    "ww_quant_ste_f32": (C.c_int, [C.POINTER(QuantSteTensor), C.c_int64, C.c_int, C.c_void_p]),
    "ww_clip_metrics_bytes": (C.c_int64, []),
    "ww_clip_metrics_margin_host": (C.c_float, [C.c_float]),
    "ww_clip_metrics_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "ww_clip_metrics_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ww_clip_metrics_update_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ww_clip_ledger_bytes": (C.c_int64, [C.c_int64]),
    "ww_clip_ledger_init": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "ww_clip_ledger_update_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "ww_train_masks": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_train_packed_image": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "ww_train_bit_images": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_train_stage": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "ww_streamer_create": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ww_streamer_create_n": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ww_streamer_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_streamer_window": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ww_streamer_destroy": (C.c_int, [C.c_void_p]),
    "ww_streamer_create_input": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.POINTER(C.c_void_p)]),
    "ww_streamer_step_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ww_streamer_latency": (C.c_int, [C.c_void_p]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP library is the only implementation of this path (no CPU "
            "fallback). Build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C wakeword-jupyterlab_amd/csrc`.")
    # RTLD_LOCAL (the default): nothing of this library enters the global symbol scope.  HIP kernel stubs have default visibility, so a
    # globally loaded copy would interpose the kernels of every other build opened later in the process (scripts/ab_kernels.py opens
    # several); libwakeword_amd_torch.so gets the addresses it needs from this handle instead (ops.py -> ww_torch_bind).
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch: fail loudly
        fn.restype, fn.argtypes = res, args
    if lib.ww_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI {lib.ww_abi_version()} != expected {ABI_VERSION}; rebuild")
    return lib


lib = _load()


def check(rc: int) -> int:
    """Raise NativeError on a negative return code; pass sizes / WW_OK through."""
    if rc < 0:
        raise NativeError(rc, (lib.ww_last_error() or b"").decode("utf-8", "replace"))
    return rc


def device_info():
    n_cu, khz = C.c_int(0), C.c_int(0)
    name = C.create_string_buffer(128)
    check(lib.ww_device_info(C.byref(n_cu), C.byref(khz), name, 128))
    return {"n_cu": n_cu.value, "clock_khz": khz.value, "name": name.value.decode()}
