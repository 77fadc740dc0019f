"""What the live-conversion tests share: the small configuration (three posterior layers, two flows of two layers: a
conversion halo of 22 frames at hop 256), its synthetic weights, the recordings, and a brute-force restatement of the
window plan.  Nothing here calls the library."""
import dataclasses

import numpy as np

from test_other_configs import ALT

POS = ("n_vocab", "spec_channels", "hop_length", "sampling_rate", "segment_size", "inter_channels", "hidden_channels",
       "filter_channels", "n_heads", "n_layers", "kernel_size", "p_dropout", "resblock", "resblock_kernel_sizes",
       "resblock_dilation_sizes", "upsample_rates", "upsample_initial_channel", "upsample_kernel_sizes")
HOP, N_FFT, UP, PAD, H_SMALL = 256, 512, 256, 128, 22


def small_dims():
    from vispeech_amd.schema import dims_from_ctor
    dims = dims_from_ctor(*[ALT[k] for k in POS], n_speakers=ALT["n_speakers"], gin_channels=ALT["gin_channels"])
    return dataclasses.replace(dims, posterior_layers=3, flow_layers=2, n_flows=2)


def small_weights(dims):
    from vispeech_amd.synth import synth_state_dict
    return synth_state_dict(dims, seed=1515)


def recording(n, seed, rate=22050.0):
    """Sine plus noise, clipped to [-1, 1]: the signal of tests/test_convert_gpu.py, one row."""
    r = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / rate
    return (0.4 * np.sin(2 * np.pi * 220.0 * t) * r.uniform(0.2, 1.0) + 0.1 * r.standard_normal(n)).astype(np.float32).clip(-1, 1)


def frames_of(n, n_fft=N_FFT, hop=HOP):
    pad = (n_fft - hop) // 2
    return 0 if (n <= pad or n + 2 * pad < n_fft) else 1 + (n + 2 * pad - n_fft) // hop


def brute_plan(n_fft, hop, halo, n, closed, e0, e1):
    """(ready, w0, w1, s_lo, s_hi) by enumerating the sample every (frame, tap) of the window reads."""
    pad = (n_fft - hop) // 2
    w0, w1 = max(0, e0 - halo), e1 + halo
    if closed:
        w1 = min(frames_of(n, n_fft, hop), w1)
    j = (np.arange(w0, w1, dtype=np.int64)[:, None] * hop - pad + np.arange(n_fft, dtype=np.int64)[None, :]).reshape(-1)
    j = np.abs(j)                                           # torch's reflect padding at sample 0
    if closed:
        j = np.where(j >= n, 2 * (n - 1) - j, j)            # ... and at the end of a finished recording
    return bool(((j >= 0) & (j < n)).all()), w0, w1, int(j.min()), int(j.max()) + 1
