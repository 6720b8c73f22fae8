"""Constants of the path, mirroring the reference's config namespaces.

AudioConfig / ModelConfig : /root/reference/wakeword_training_script.py:29-43 (dup notebook cell 3)
Config                    : /root/reference/wakeword_training/train_wakeword.py:16-25
AugmentationConfig        : /root/reference/wakeword_training_script.py:52-58
TrainingConfig            : /root/reference/wakeword_training_script.py:45-50 (read by trainer.WakewordTrainer)
Only the fields the accelerated path reads are kept.
"""


class AudioConfig:
    SAMPLE_RATE = 16000
    DURATION = 1.0
    N_MELS = 80
    N_FFT = 2048
    HOP_LENGTH = 512
    WIN_LENGTH = 2048
    FMIN = 0
    FMAX = 8000


class AugmentationConfig:
    AUGMENTATION_PROB = 0.8
    NOISE_FACTOR = 0.15
    TIME_SHIFT_MAX = 0.3
    PITCH_SHIFT_MAX = 3
    SPEED_CHANGE_MIN = 0.7
    SPEED_CHANGE_MAX = 1.3
    # background noise (AudioProcessor.set_background_noise): mixed with this probability at an SNR drawn uniformly in [MIN, MAX] dB
    # (MS-SNSD's noisyspeech_synthesizer.cfg bounds); used only when the processor has a noise bank attached
    BACKGROUND_PROB = 0.8
    BACKGROUND_SNR_MIN = 0.0
    BACKGROUND_SNR_MAX = 40.0
    # reverberation (AudioProcessor.set_room_impulse_responses): a random RIR of the bank with this probability, before the background;
    # 0.5 (half the clips stay close-talk) is this project's choice, not a published recipe's
    RIR_PROB = 0.5


class SpecAugmentConfig:
    """Time and frequency masks on the log-mel batch (AudioProcessor.set_spec_augment; not in the reference).  These values are this
    project's choices, not a published recipe's: a clip is masked at all with PROB, then gets FREQ_MASKS bands of 0 .. FREQ_MASK_MAX mel
    bins and TIME_MASKS blocks of 0 .. int(TIME_MASK_MAX_FRACTION * T) frames (4 frames at T = 32, 1 at T = 8, 7 at T = 63)."""
    PROB = 0.8
    FREQ_MASKS = 2
    FREQ_MASK_MAX = 12
    TIME_MASKS = 2
    TIME_MASK_MAX_FRACTION = 0.125
    FILL = "mean"             # "mean" or "min" of the clip before masking, or a float


SPEC_MAX_MASKS = 4            # masks per axis one record holds (csrc/ww_specaug.hip)


def check_spec_augment_config(cfg) -> None:
    """ValueError for what the masking kernel refuses: PROB outside [0, 1], more than 4 masks per axis, a band wider than the 80 mel
    bins, a fraction outside [0, 1] (a block wider than the clip), a FILL that is neither "mean", "min" nor a number."""
    import math
    prob, frac = float(cfg.PROB), float(cfg.TIME_MASK_MAX_FRACTION)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"SpecAugment PROB {cfg.PROB}: expected a probability in [0, 1]")
    for name in ("FREQ_MASKS", "TIME_MASKS"):
        v = getattr(cfg, name)
        if int(v) != v or not 0 <= v <= SPEC_MAX_MASKS:
            raise ValueError(f"SpecAugment {name} {v}: expected an integer in 0..{SPEC_MAX_MASKS}")
    if int(cfg.FREQ_MASK_MAX) != cfg.FREQ_MASK_MAX or not 0 <= cfg.FREQ_MASK_MAX <= AudioConfig.N_MELS:
        raise ValueError(f"SpecAugment FREQ_MASK_MAX {cfg.FREQ_MASK_MAX}: expected an integer in 0..{AudioConfig.N_MELS}")
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"SpecAugment TIME_MASK_MAX_FRACTION {cfg.TIME_MASK_MAX_FRACTION}: expected a fraction in [0, 1]")
    fill = cfg.FILL
    if isinstance(fill, str):
        if fill not in ("mean", "min"):
            raise ValueError(f"SpecAugment FILL {fill!r}: expected 'mean', 'min' or a float")
    elif isinstance(fill, bool) or not isinstance(fill, (int, float)) or math.isnan(float(fill)):
        raise ValueError(f"SpecAugment FILL {fill!r}: expected 'mean', 'min' or a float")


class ChannelConfig:
    """Microphone-channel augmentation on the waveform (AudioProcessor.set_channel_effects; not in the reference): a random equaliser
    -- high-pass, low shelf, up to PEAKS peaks, high shelf, low-pass, each second-order and each on with its own probability -- and a
    peak-preserving tanh saturator.  These values are this project's choices, not a published recipe's.  A clip is touched at all with
    PROB.  Frequencies (Hz) and Q are drawn log-uniformly in their (lo, hi) range, gains uniformly in +-DB and the drive uniformly;
    passes and shelves have Q = 1/sqrt(2)."""
    PROB = 0.5
    HIGHPASS_PROB = 0.5
    HIGHPASS_HZ = (20.0, 400.0)
    LOW_SHELF_PROB = 0.5
    LOW_SHELF_HZ = (100.0, 400.0)
    HIGH_SHELF_PROB = 0.5
    HIGH_SHELF_HZ = (2000.0, 5000.0)
    SHELF_DB = 6.0
    PEAKS = 3
    PEAK_PROB = 0.5
    PEAK_HZ = (100.0, 6000.0)
    PEAK_DB = 6.0
    PEAK_Q = (0.5, 2.0)
    LOWPASS_PROB = 0.3
    LOWPASS_HZ = (3000.0, 7500.0)
    DRIVE_PROB = 0.2
    DRIVE = (0.5, 3.0)


CHANNEL_SECTIONS = 8          # second-order sections one record holds (csrc/ww_channel.hip)
CHANNEL_MAX_PEAKS = 4
CHANNEL_MAX_HZ = 7600.0       # below Nyquist, where the cookbook forms stay well conditioned
CHANNEL_MAX_DRIVE = 8.0
CHANNEL_MAX_DB = 40.0
CHANNEL_MAX_Q = 1e6


def check_channel_config(cfg) -> None:
    """ValueError for what the channel stage refuses: a probability outside [0, 1], a frequency outside (0, 7600], a Q <= 0, more than
    4 peaks, a drive < 0 or > 8, a dB span outside [0, 40], a reversed range, a value that is not a finite number.  Every value is
    judged as the float32 the kernel receives (a frequency of 1e-50 is 0 there), so what passes here passes the library's own check."""
    import ctypes
    import math

    def num(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
            raise ValueError(f"Channel {name} {v!r}: expected a finite number")
        v = ctypes.c_float(float(v)).value
        if not math.isfinite(v):
            raise ValueError(f"Channel {name}: the value does not fit a float32")
        return v

    def rng(name):
        v = getattr(cfg, name)
        if not isinstance(v, (tuple, list)) or len(v) != 2:
            raise ValueError(f"Channel {name} {v!r}: expected a (lo, hi) pair")
        lo, hi = num(name, v[0]), num(name, v[1])
        if lo > hi:
            raise ValueError(f"Channel {name} {v!r}: the range is reversed")
        return lo, hi

    for name in ("PROB", "HIGHPASS_PROB", "LOW_SHELF_PROB", "HIGH_SHELF_PROB", "PEAK_PROB", "LOWPASS_PROB", "DRIVE_PROB"):
        if not 0.0 <= num(name, getattr(cfg, name)) <= 1.0:
            raise ValueError(f"Channel {name} {getattr(cfg, name)}: expected a probability in [0, 1]")
    for name in ("HIGHPASS_HZ", "LOW_SHELF_HZ", "HIGH_SHELF_HZ", "PEAK_HZ", "LOWPASS_HZ"):
        lo, hi = rng(name)
        if not (0.0 < lo and hi <= CHANNEL_MAX_HZ):
            raise ValueError(f"Channel {name} {getattr(cfg, name)}: expected frequencies in (0, {CHANNEL_MAX_HZ:g}] Hz")
    q_lo, q_hi = rng("PEAK_Q")
    if not (q_lo > 0.0 and q_hi <= CHANNEL_MAX_Q):
        raise ValueError(f"Channel PEAK_Q {cfg.PEAK_Q}: expected 0 < Q <= {CHANNEL_MAX_Q:g}")
    for name in ("SHELF_DB", "PEAK_DB"):
        if not 0.0 <= num(name, getattr(cfg, name)) <= CHANNEL_MAX_DB:
            raise ValueError(f"Channel {name} {getattr(cfg, name)}: expected a span in [0, {CHANNEL_MAX_DB:g}] dB")
    if isinstance(cfg.PEAKS, bool) or int(cfg.PEAKS) != cfg.PEAKS or not 0 <= cfg.PEAKS <= CHANNEL_MAX_PEAKS:
        raise ValueError(f"Channel PEAKS {cfg.PEAKS}: expected an integer in 0..{CHANNEL_MAX_PEAKS}")
    lo, hi = rng("DRIVE")
    if lo < 0.0 or hi > CHANNEL_MAX_DRIVE:
        raise ValueError(f"Channel DRIVE {cfg.DRIVE}: expected drives in [0, {CHANNEL_MAX_DRIVE:g}]")


class MixupConfig:
    """Mixup on the log-mel batch (AudioProcessor.set_mixup; Zhang et al. 2018; not in the reference).  A row is mixed with PROB; its
    weight lam is one Beta(ALPHA, ALPHA) draw, and with DOMINANT it is folded to lam >= 0.5 so that a row stays mostly itself.  PROB
    and DOMINANT are this project's choices; ALPHA = 0.2 is the paper's value for speech commands."""
    PROB = 0.5
    ALPHA = 0.2
    DOMINANT = True


def check_mixup_config(cfg) -> None:
    """ValueError for a PROB outside [0, 1] or an ALPHA that is not a positive finite number."""
    import math
    for name in ("PROB", "ALPHA"):
        v = getattr(cfg, name)
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"Mixup {name} {v!r}: expected a number")
    if not 0.0 <= float(cfg.PROB) <= 1.0:
        raise ValueError(f"Mixup PROB {cfg.PROB}: expected a probability in [0, 1]")
    if not (math.isfinite(float(cfg.ALPHA)) and float(cfg.ALPHA) > 0.0):
        raise ValueError(f"Mixup ALPHA {cfg.ALPHA}: expected a positive finite number")


class ModelConfig:            # WakewordModel (3 convs)
    HIDDEN_SIZE = 256
    NUM_LAYERS = 2
    DROPOUT = 0.6
    NUM_CLASSES = 2


class TrainingConfig:         # WakewordTrainer
    BATCH_SIZE = 16
    LEARNING_RATE = 0.0001
    EPOCHS = 10
    VALIDATION_SPLIT = 0.2
    TEST_SPLIT = 0.1


class Config:                 # SimpleWakewordModel (2 convs)
    SAMPLE_RATE = 16000
    DURATION = 1.0
    N_MELS = 80
    HIDDEN_SIZE = 256
    NUM_LAYERS = 2
    DROPOUT = 0.5


CLIP_SAMPLES = int(AudioConfig.SAMPLE_RATE * AudioConfig.DURATION)          # 16000
N_FRAMES = 1 + CLIP_SAMPLES // AudioConfig.HOP_LENGTH                       # 32


MIN_DURATION, MAX_DURATION = 0.25, 2.0          # other clip lengths: 4,000 .. 32,000 samples, 8 .. 63 frames (training and augmentation: <= 32)


def check_audio_config(cfg) -> None:
    """The kernels are built for the reference constants, at DURATION 1.0 for everything and at any DURATION in [0.25, 2.0] for inference;
    training, augmentation and streaming take DURATION 0.25 .. 1.0 (T <= 32 frames).  Refuse anything else loudly."""
    want = {k: getattr(AudioConfig, k) for k in ("SAMPLE_RATE", "N_MELS", "N_FFT", "HOP_LENGTH", "WIN_LENGTH", "FMIN", "FMAX")}
    got = {k: getattr(cfg, k, None) for k in want}
    dur = float(getattr(cfg, "DURATION", 1.0))
    if not MIN_DURATION <= dur <= MAX_DURATION or any(float(got[k]) != float(want[k]) for k in want):
        raise NotImplementedError(f"the HIP front-end is built for {want} at DURATION {MIN_DURATION}..{MAX_DURATION} s; got {got}, "
                                  f"DURATION {dur}")


def n_samples(cfg) -> int:
    """N = int(SAMPLE_RATE * DURATION): the clip length pad_or_truncate produces (16000 at 1 s)."""
    return int(cfg.SAMPLE_RATE * cfg.DURATION)


def n_frames(cfg) -> int:
    """T = 1 + N // HOP_LENGTH: the mel frames of one clip (librosa center=True; 32 at 1 s, 8 .. 63 over 0.25 .. 2 s)."""
    return 1 + n_samples(cfg) // cfg.HOP_LENGTH


def is_one_second(cfg) -> bool:
    return n_samples(cfg) == CLIP_SAMPLES
