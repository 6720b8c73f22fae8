"""AudioProcessor drop-in (reference: /root/reference/wakeword_training_script.py:61-138).

Same method names, arguments and return conventions:
  load_audio(path)            -> float32 ndarray at 16 kHz mono, or None (prints the error; never raises)
  normalize_audio(audio)      -> audio / max|audio|            (empty-array guard only, as the reference)
  pad_or_truncate(audio, n)   -> random crop (python `random`) or right zero-pad
  audio_to_mel(audio)         -> ndarray [80, T] log-mel dB     <- HIP kernel K1
  process_audio_file(path)    -> ndarray [80, T] or None

plus the batched form the GPU wants: `mel_batch(pcm[B, n]) -> torch.Tensor [B, 1, 80, T]` on the device.
T = 32 for the default 1 s config; a config with DURATION in [0.25, 2.0] gives T = 1 + int(16000 * DURATION) // 512 for audio_to_mel and
mel_batch, and for process_audio_file / load_clips_gpu (K0 crops and pads to N samples).  Augmentation runs where training does,
T <= 32 (DURATION 0.25 .. 1.0, N = 4000 .. 16000 samples), and refuses longer clips.

  augment_audio(audio)        -> time shift / pitch shift / time stretch / noise, each with probability 0.8
                                 (random draws from python `random` in the reference's order)  <- HIP kernels KA
  set_background_noise(paths) -> background noise at a random SNR, mixed in after the stretch (background.py; not in the reference)
  set_room_impulse_responses(paths) -> reverberation with a random room impulse response, before the background (reverb.py; idem)
  set_spec_augment(config)    -> SpecAugment: blocks of mel bins and of frames masked on the log-mel batch, after K1 (idem)
  set_channel_effects(config) -> microphone-channel augmentation: random EQ, band limit and clipping on the waveform, before K1 (idem)
  set_mixup(config)           -> mixup: rows of the log-mel batch mixed with a partner row, the targets with them, last of all (idem)
`load_audio` / `process_audio_file` read the file with the library's native reader (csrc/ww_files.cpp) and decode, mix down and
resample it on the GPU (kernel K0: scipy.signal.resample_poly's Kaiser design -- NOT librosa's soxr resampler, an absent third-party
library: parity unpinned) -- the same code path as the batched loaders, one file at a time.  PCM / float WAV and FLAC.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from . import ops
from .config import AudioConfig, AugmentationConfig, check_audio_config, is_one_second, n_frames, n_samples


class AudioProcessor:
    def __init__(self, config=AudioConfig, device=None):
        check_audio_config(config)
        self.config = config
        self._n = n_samples(config)                      # N: 16000 at 1 s; 4000 .. 32000 over DURATION 0.25 .. 2 (inference)
        self.device = torch.device(device) if device is not None else None

    def _dev(self):
        if self.device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("AudioProcessor.audio_to_mel runs on the MI355X only and no GPU is visible (no CPU fallback)")
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    # ---- reference API --------------------------------------------------------------------------
    def load_audio(self, file_path):
        """= librosa.load(path, sr=16000) (:65-71): the WHOLE file as float32 at 16 kHz mono, or None (prints the error, never raises on a
        bad file).  Native reader, then ONE upload of the file's bytes and ONE K0 launch over all its 1 s windows (descriptors that share the
        byte offset and differ in crop_start; without normalisation K0 computes a window's samples only): linear in the file's length
        (round 3 uploaded and resampled the whole file once per second of it).  No normalisation, no crop."""
        rd = self.gpu_reader(1)                                   # raises without a GPU: a missing device is not a bad file
        try:
            samples = decode_whole_file(rd, file_path, self._dev())
            if samples is None:
                return np.zeros(0, dtype=np.float32)
            audio = samples.cpu().numpy()      # (synchronises: the slot's device buffer is free again)
            return np.ascontiguousarray(audio, dtype=np.float32)
        except Exception as e:                                             # reference: print and return None (:66-71)
            print(f"Error loading {file_path}: {e}")
            return None

    def normalize_audio(self, audio):
        if len(audio) == 0:
            return audio
        with np.errstate(invalid="ignore", divide="ignore"):
            return audio / np.max(np.abs(audio))

    def pad_or_truncate(self, audio, target_length):
        if len(audio) > target_length:
            start_idx = random.randint(0, len(audio) - target_length)
            return audio[start_idx:start_idx + target_length]
        return np.pad(audio, (0, target_length - len(audio)), mode="constant")

    def audio_to_mel(self, audio):
        """[n <= N] samples -> ndarray [80, T] (dB; [80, 32] at 1 s).  No normalisation here (reference :85-101)."""
        n_frames = int(self.config.SAMPLE_RATE * self.config.DURATION / self.config.HOP_LENGTH) + 1
        if len(audio) == 0:
            return np.zeros((self.config.N_MELS, n_frames))
        pcm = torch.as_tensor(np.ascontiguousarray(audio, dtype=np.float32)).unsqueeze(0).to(self._dev())
        return self._logmel(pcm, False)[0, 0].cpu().numpy()

    def _logmel(self, pcm, normalize):
        if is_one_second(self.config):
            return ops.logmel(pcm, normalize)
        return ops.logmel_frames(pcm, self._n, normalize)

    def _check_augment(self):
        if n_frames(self.config) > 32:
            raise NotImplementedError(f"augmentation at DURATION {self.config.DURATION}: not supported yet (augmentation and training take "
                                      f"clips of at most 32 frames, DURATION <= 1.0; longer clips are inference only, augment=False)")

    def draw_augment_plan(self, config=AugmentationConfig, length=None):
        """The random draws of augment_audio (:103-123) in the reference's order -> one plan dict.
        pad_or_truncate's crop start (:116-117) is drawn here too, right after the speed factor."""
        sr = self.config.SAMPLE_RATE
        n = length or int(sr * self.config.DURATION)
        plan = {"shift": 0, "n_steps": None, "rate": None, "crop": 0, "sigma": 0.0, "seed": 0}
        if random.random() < config.AUGMENTATION_PROB:
            plan["shift"] = int(random.uniform(-config.TIME_SHIFT_MAX, config.TIME_SHIFT_MAX) * sr)
        if random.random() < config.AUGMENTATION_PROB:
            plan["n_steps"] = random.uniform(-config.PITCH_SHIFT_MAX, config.PITCH_SHIFT_MAX)
        if random.random() < config.AUGMENTATION_PROB:
            plan["rate"] = random.uniform(config.SPEED_CHANGE_MIN, config.SPEED_CHANGE_MAX)
            stretched = int(round(n / plan["rate"]))
            if stretched > n:
                plan["crop"] = random.randint(0, stretched - n)
        if random.random() < config.AUGMENTATION_PROB:
            plan["sigma"] = float(config.NOISE_FACTOR)
            plan["seed"] = random.getrandbits(32)
        # background noise: drawn only with a bank attached (set_background_noise), after the reference's draws; a plan without
        # background keeps exactly the reference's keys
        bank = getattr(self, "_background", None)
        prob = getattr(config, "BACKGROUND_PROB", 0.0)
        if bank is not None and prob > 0 and random.random() < prob:
            f = random.randrange(bank.n_files)
            plan["bg_file"] = f
            plan["bg_start"] = random.randrange(int(bank.lengths[f]))
            plan["snr_db"] = random.uniform(config.BACKGROUND_SNR_MIN, config.BACKGROUND_SNR_MAX)
        # reverberation: drawn only with an RIR bank attached (set_room_impulse_responses), after the background draws
        rirs = getattr(self, "_rirs", None)
        rir_prob = getattr(config, "RIR_PROB", 0.0)
        if rirs is not None and rir_prob > 0 and random.random() < rir_prob:
            plan["rir"] = random.randrange(rirs.n_rirs)
        return plan

    def set_background_noise(self, paths_or_bank, max_seconds=None):
        """Attach a background noise bank: a background.BackgroundNoiseBank, or the paths / directory to build one from (WAV and FLAC,
        decoded whole on this processor's device; `max_seconds` caps the audio it keeps).  From then on every augmentation of this
        processor -- augment_audio, augment_batch, process_audio_file(augment=True), WakewordDataset(augment=True) per item and through
        loader() / batches() -- mixes a random file's segment into a clip with probability BACKGROUND_PROB, at an SNR drawn uniformly in
        [BACKGROUND_SNR_MIN, BACKGROUND_SNR_MAX] dB.  `None` detaches the bank.  Returns the bank (or None)."""
        from .background import BackgroundNoiseBank
        if paths_or_bank is None:
            self._background = None
        elif isinstance(paths_or_bank, BackgroundNoiseBank):
            self._background = paths_or_bank
        else:
            self._background = BackgroundNoiseBank(paths_or_bank, device=self._dev(), max_seconds=max_seconds)
        return self._background

    @property
    def background_noise(self):
        """The attached background.BackgroundNoiseBank, or None."""
        return getattr(self, "_background", None)

    def set_room_impulse_responses(self, paths_or_bank):
        """Attach a room impulse response bank: a reverb.ImpulseResponseBank, or the paths / directory to build one from (WAV and FLAC,
        decoded whole on this processor's device, only their spectra kept).  From then on every augmentation of this processor --
        augment_audio, augment_batch, process_audio_file(augment=True), WakewordDataset(augment=True) per item and through the package
        DataLoader -- convolves a clip with a random RIR with probability RIR_PROB, after the stretch and before the background noise,
        keeping the keyword where it was and the clip's energy.  `None` detaches the bank.  Returns the bank (or None)."""
        from .reverb import ImpulseResponseBank
        if paths_or_bank is None:
            self._rirs = None
        elif isinstance(paths_or_bank, ImpulseResponseBank):
            self._rirs = paths_or_bank
        else:
            self._rirs = ImpulseResponseBank(paths_or_bank, device=self._dev())
        return self._rirs

    @property
    def room_impulse_responses(self):
        """The attached reverb.ImpulseResponseBank, or None."""
        return getattr(self, "_rirs", None)

    def set_spec_augment(self, config):
        """Turn SpecAugment on (a config.SpecAugmentConfig, or a class with its fields; validated here) or off (`None`, the default).
        From then on everything of this processor that augments -- process_audio_file(augment=True), WakewordDataset(augment=True) per
        item and through loader() / batches(), ClipBank loaders with augment=True -- follows the log-mel with one in-place masking
        launch whose seed is one `random.getrandbits(64)` per batch, drawn after augment_batch's draws.  Nothing that runs with
        augment=False draws or launches anything more.  Returns the config (or None)."""
        if config is not None:
            from .config import check_spec_augment_config
            check_spec_augment_config(config)
        self._spec_augment = config
        return config

    @property
    def spec_augment(self):
        """The SpecAugment config in force, or None."""
        return getattr(self, "_spec_augment", None)

    def spec_augment_batch(self, mel, plans=None, seed=None, inplace=False) -> torch.Tensor:
        """mel [B, 1, 80, T] or [B, 80, T] on the GPU -> the masked batch, with the config in force (config.SpecAugmentConfig when none
        is set).  `plans`: a list of {"freq": [(start, width), ...], "time": [...]} per clip (ops.pack_spec_plans); else the records
        are drawn on the device from `seed`, which is `random.getrandbits(64)` when not given."""
        from .config import SpecAugmentConfig
        config = self.spec_augment or SpecAugmentConfig
        out = mel if inplace else None
        if plans is not None:
            if seed is not None:
                raise ValueError("spec_augment_batch: give `plans` or `seed`, not both")
            records = torch.from_numpy(ops.pack_spec_plans(plans, mel.shape[-1])).to(mel.device)
            return ops.spec_augment(mel, records=records, config=config, out=out)
        if seed is None:
            seed = random.getrandbits(64)
        return ops.spec_augment(mel, seed=seed, config=config, out=out)

    def set_channel_effects(self, config):
        """Turn the microphone-channel stage on (a config.ChannelConfig, or a class with its fields; validated here) or off (`None`, the
        default).  From then on everything of this processor that augments -- process_audio_file(augment=True), WakewordDataset(augment=True)
        per item and through loader() / batches(), ClipBank loaders with augment=True -- follows augment_batch with one in-place launch
        on the waveform (a random equaliser and saturator per clip: the microphone hears speech, room, background and noise alike)
        whose seed is one `random.getrandbits(64)` per batch, drawn after augment_batch's draws and before SpecAugment's seed.  Nothing
        that runs with augment=False draws or launches anything more.  Returns the config (or None)."""
        if config is not None:
            from .config import check_channel_config
            check_channel_config(config)
        self._channel_effects = config
        return config

    @property
    def channel_effects(self):
        """The channel-effects config in force, or None."""
        return getattr(self, "_channel_effects", None)

    def channel_effects_batch(self, pcm, plans=None, seed=None, inplace=False) -> torch.Tensor:
        """pcm [B, N] float32 on the GPU -> the batch through the channel stage, with the config in force (config.ChannelConfig when none
        is set).  `plans`: a list of dicts per clip (ops.pack_channel_plans); else the records are drawn on the device from `seed`,
        which is `random.getrandbits(64)` when not given."""
        from .config import ChannelConfig
        config = self.channel_effects or ChannelConfig
        out = pcm if inplace else None
        if plans is not None:
            if seed is not None:
                raise ValueError("channel_effects_batch: give `plans` or `seed`, not both")
            records = torch.from_numpy(ops.pack_channel_plans(plans)).to(pcm.device)
            return ops.channel_effects(pcm, records=records, config=config, out=out)
        if seed is None:
            seed = random.getrandbits(64)
        return ops.channel_effects(pcm, seed=seed, config=config, out=out)

    def set_mixup(self, config):
        """Turn mixup on (a config.MixupConfig, or a class with its fields; validated here) or off (`None`, the default).  From then on
        the batched loaders that augment -- dataset.loader() / batches() of a WakewordDataset(augment=True), ClipBank loaders with
        augment=True -- finish every batch with mixup_batch: one more launch, after SpecAugment and after unreadable rows are zeroed, and
        they yield `(data, target)` with target float32 [B, 2] class probabilities instead of int64 labels (WakewordTrainer.step takes
        both).  Nothing that runs with augment=False, and nothing per item, draws or launches anything more.  Returns the config."""
        if config is not None:
            from .config import check_mixup_config
            check_mixup_config(config)
        self._mixup = config
        return config

    @property
    def mixup(self):
        """The mixup config in force, or None."""
        return getattr(self, "_mixup", None)

    def mixup_plan(self, B, bad=None):
        """The draws of one batch of B rows, from python `random` in this order: one random.sample(range(B), B) for the partners; per
        row, in batch order, random.random() < PROB; for a chosen row only, one random.betavariate(ALPHA, ALPHA), rounded to float32 and,
        with DOMINANT and lam < 0.5, replaced by float32(1) - lam.  A row that is not chosen gets lam = 1 and itself as partner.  `bad`
        (a boolean mask [B]: unreadable files, placeholders): those rows, and every row whose partner is one, are unmixed -- a fix-up
        after the draws, which it does not change.  Returns (partner int32 [B], lam float32 [B]) on the host."""
        from .config import MixupConfig
        config = self.mixup or MixupConfig
        B = int(B)
        if B < 1:
            raise ValueError(f"mixup_plan: B = {B}")
        partner = np.asarray(random.sample(range(B), B), dtype=np.int32)
        lam = np.ones(B, dtype=np.float32)
        for i in range(B):
            if random.random() < config.PROB:
                v = np.float32(random.betavariate(config.ALPHA, config.ALPHA))
                lam[i] = np.float32(1.0) - v if config.DOMINANT and v < np.float32(0.5) else v
        if bad is not None:
            bad = np.asarray(bad, dtype=bool)
            if bad.shape != (B,):
                raise ValueError(f"mixup_plan: bad must be a boolean mask [{B}], got {bad.shape}")
            lam[bad | bad[partner]] = 1.0
        mixed = lam != 1.0
        partner = np.where(mixed, partner, np.arange(B, dtype=np.int32)).astype(np.int32)
        return partner, lam

    def mixup_batch(self, data, labels, plan=None):
        """data [B, 1, 80, T] or [B, 80, T] and labels int64 [B] or [B, 1], both on the GPU -> (mixed data, targets float32 [B, 2]) by
        `plan` = (partner, lam) as mixup_plan returns it (drawn here when None).  The plan goes up in ONE host-to-device copy."""
        B = int(data.shape[0])
        partner, lam = self.mixup_plan(B) if plan is None else plan
        host = np.empty((2, B), dtype=np.int32)
        host[0] = np.asarray(partner, dtype=np.int32)
        host[1] = np.ascontiguousarray(lam, dtype=np.float32).view(np.int32)
        dev = torch.from_numpy(host).to(data.device)
        return ops.mixup(data, labels, dev[0], dev[1].view(torch.float32))

    def augment_batch(self, pcm, plans=None, config=AugmentationConfig) -> torch.Tensor:
        """pcm [B, N] (ndarray or tensor) -> augmented device tensor [B, N]; one plan per clip (drawn here if None).
        N = 16000 at 1 s; any configured clip length of at most 32 frames (DURATION 0.25 .. 1.0)."""
        self._check_augment()
        t = torch.as_tensor(pcm, dtype=torch.float32)
        if t.device.type != "cuda":
            t = t.to(self._dev(), non_blocking=True)
        if plans is None:
            plans = [self.draw_augment_plan(config, t.shape[1]) for _ in range(t.shape[0])]
        rirs = getattr(self, "_rirs", None)
        if rirs is None:                                      # (the call without an RIR bank is the one it always was)
            return ops.augment(t, plans, bank=getattr(self, "_background", None))
        return ops.augment(t, plans, bank=getattr(self, "_background", None), rirs=rirs)

    def augment_audio(self, audio, config=AugmentationConfig):
        """[N] samples -> augmented float32 ndarray [N] (reference :103-123), on the GPU (N = 16000 at 1 s)."""
        self._check_augment()
        a = np.ascontiguousarray(audio, dtype=np.float32)
        if a.shape != (self._n,):
            raise ValueError(f"augment_audio takes exactly one padded clip of {self._n} samples, got {a.shape}")
        return self.augment_batch(a[None, :], config=config)[0].cpu().numpy()

    def process_audio_file(self, file_path, augment=False):
        """load -> normalise over the whole file -> random crop / zero pad -> (augment) -> log-mel (:125-138), all on the GPU:
        native reader -> K0 -> (KA) -> (channel effects, when set_channel_effects is on) -> K1 -> (SpecAugment, when set_spec_augment is
        on).  The random draws are python `random`'s in the reference's order (crop, then augmentation, then the channel seed, then the
        masking seed)."""
        if augment:
            self._check_augment()
        pcm, ok = self.load_clips_gpu([file_path])
        if not bool(ok[0]):
            return None
        if augment:
            pcm = self.augment_batch(pcm)
            if self.channel_effects is not None:
                self.channel_effects_batch(pcm, inplace=True)
        mel = self.mel_batch(pcm, normalize=False)
        if augment and self.spec_augment is not None:
            self.spec_augment_batch(mel, inplace=True)
        return mel[0, 0].cpu().numpy()

    # ---- batched form ---------------------------------------------------------------------------
    def mel_batch(self, pcm, normalize: bool = True) -> torch.Tensor:
        """pcm [B, n<=N] (ndarray or tensor, any device) -> device tensor [B, 1, 80, T] (N = 16000, T = 32 at 1 s).
        normalize=True folds normalize_audio + zero-pad + audio_to_mel, the order process_audio_file uses."""
        t = torch.as_tensor(pcm, dtype=torch.float32)
        if t.device.type != "cuda":
            t = t.to(self._dev(), non_blocking=True)
        return self._logmel(t, normalize)

    def load_clips_gpu(self, paths, normalize: bool = True, lo: int = 0, hi=None):
        """Host: the library's reader threads open the files, walk their RIFF headers and read the sample bytes into pinned
        staging (files.WavBatchReader -> ww_read_wav_batch_host).  GPU (kernel K0): sample conversion, mono mix, polyphase
        resample to 16 kHz, whole-file peak normalisation, random crop / zero pad to N samples (the config's DURATION) --
        process_audio_file :125-133 up to the mel call.  `paths`: a list, or a files.EncodedPaths with a window [lo, hi).  Returns (device tensor [B, N],
        ok mask); unreadable files give a zero row, ok False."""
        from .files import EncodedPaths
        hi = len(paths) if hi is None else hi
        if not isinstance(paths, EncodedPaths):
            paths = list(paths)
        return self.gpu_reader(hi - lo).load(paths, normalize, lo=lo, hi=hi)

    def gpu_reader(self, batch_size: int = 64):
        """This processor's native batch reader (3 staging slots, sized for `batch_size` files of up to 2 s of 16 kHz PCM-16; it grows on demand)."""
        from .files import WavBatchReader
        dev = self._dev()
        if getattr(self, "_reader", None) is None or self._reader.device != dev:
            self._reader = WavBatchReader(max_clips=max(64, batch_size), max_raw_bytes=max(64, batch_size) * 65536, slots=3, device=dev,
                                          n_samples=self._n)
        elif self._reader.max_clips < batch_size:
            self._reader.regrow(batch_size, batch_size * 65536)
        return self._reader


def decode_whole_file(rd, file_path, dev, before_read=None):
    """One file, whole, through the native reader `rd` and K0 -> 1-D float32 device tensor of its samples at 16 kHz mono (None for a file
    of no samples); raises on an unreadable file.  ONE upload of the file's bytes and ONE K0 launch over all its 1 s windows (descriptors
    that share the byte offset and differ in crop_start; without normalisation K0 computes a window's samples only), enqueued on the
    current stream.  `before_read(slot)` runs before the reader writes a slot's staging (a caller that does not synchronise between files
    waits there for the work that last read the slot).  AudioProcessor.load_audio and background.BackgroundNoiseBank share it."""
    import ctypes as C
    from . import _native as nat
    from .files import CLIP_SAMPLES, DESC_DTYPE

    def read():
        slot = rd.next_slot()
        if before_read is not None:
            before_read(slot)
        return slot, rd.read([file_path], slot)
    try:
        slot, (descs, status) = read()
    except nat.NativeError as e:
        if e.code != nat.WW_ENOSPACE:
            raise
        rd.regrow(1, int(e.needed * 1.25) + 4096)
        slot, (descs, status) = read()
    if status[0] != 1:
        raise ValueError(nat.WAV_STATUS.get(int(status[0]), int(status[0])))
    n_out = int(-(-(int(descs["n_frames"][0]) * int(descs["up"][0])) // max(1, int(descs["down"][0]))))
    if n_out == 0:
        return None
    n_win = -(-n_out // CLIP_SAMPLES)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if int(descs["format"][0]) == nat.FMT_FLAC:
            # FLAC: the reader uploads the frames and decodes them on the device; K0 then reads the float32 samples it points at
            staged = np.zeros(1, dtype=DESC_DTYPE)
            raw_p = C.c_void_p()
            nat.check(nat.lib.ww_wav_batch_stage(rd._h, slot, stream, C.byref(raw_p), staged.ctypes.data))
            src, raw_dev = staged, None
        else:
            raw_dev = torch.from_numpy(rd.staging(slot)).to(dev)
            src, raw_p = descs[:1], C.c_void_p(raw_dev.data_ptr())
        win = np.repeat(np.asarray(src), n_win)                          # a copy: same bytes, same filter, one window each
        win["crop_start"] = np.arange(n_win, dtype=np.int64) * CLIP_SAMPLES
        descs_dev = torch.from_numpy(win.view(np.uint8).reshape(n_win, DESC_DTYPE.itemsize)).to(dev)
        out = torch.empty((n_win, CLIP_SAMPLES), device=dev, dtype=torch.float32)
        nat.check(nat.lib.ww_decode_resample(raw_p, C.c_void_p(descs_dev.data_ptr()), n_win, 0, C.c_void_p(out.data_ptr()), stream))
    return out.reshape(-1)[:n_out]
