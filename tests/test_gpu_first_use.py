"""Order of first use.  A kernel that needs more than 64 KiB of dynamic LDS is opted in at its own first launch on a device
(csrc/ww_internal.h: launch), whichever sibling ran before it.  Each path below is therefore run as the FIRST GPU work of a fresh
process and compared, bit for bit, with the same call in this (warm) process.  Correctness against the float64 oracles stays with the
parity tests; a launch that lacks its opt-in is an error return of the launch call, not a fault.

  frames_f16x3   forward_pcm_frames, 2 clips of 17,408 samples (35 frames, two column tiles), 3-conv model: cnn2w_kernel<0, true>,
                 cnn3w_kernel<false, true> and the 64-frame log-mel instances
  frames_f32     the same under conv math f32: cnn2_kernel<false, true>, cnn3_kernel<false, true>
  pcm_f16x3d     forward_pcm, 2 one-second clips, 3-conv, direct f16x3: cnn2h16_kernel<false>, cnn3h_kernel
  train3_f16x3   one training forward and backward, B = 2, T = 32, 3-conv, split precision: cnn2w_kernel<3>, cnn3w_kernel<true> and
                 the kernels of ww_train_h.hip; the hash covers the logits and every gradient
  train2_f32     the same for the 2-conv model in exact fp32: conv_wgrad_kernel and conv_dgrad_kernel of ww_train.hip
  augment        ops.augment with a pitch and a stretch plan: stft_pv_kernel, istft_kernel, resample_kernel
  streamer       the first two hops of a StreamingDetector: the opt-ins happen inside the stream capture of its first step
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_first_use_in_a_fresh_process_gives_the_bits_of_a_warm_one():
    import _first_use_child as child
    from wakeword_jupyterlab_amd import _native as nat

    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_first_use_child.py")
    for path in child.PATHS:
        # one child at a time, and none after one that ended abnormally or ran out of time (subprocess.run raises on the timeout)
        res = subprocess.run([sys.executable, script, path], capture_output=True, text=True, timeout=180)
        assert res.returncode == 0, f"{path}: child exited with {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
        lines = [ln.split() for ln in res.stdout.splitlines() if ln.startswith("FIRST_USE ")]
        assert len(lines) == 1 and lines[0][1] == path, res.stdout[-2000:]
        cold, timeouts = lines[0][2], int(lines[0][3])
        assert timeouts == 0, f"{path}: {timeouts} bounded waits expired in the fresh process"
        warm = child.digest(path)
        assert warm == child.digest(path), f"{path}: two runs in this process disagree"
        assert cold == warm, f"{path}: the first launch of a fresh process and a warm process disagree"
    assert nat.lib.ww_sync_timeouts() == 0
