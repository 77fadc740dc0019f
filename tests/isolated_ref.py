"""Shared helpers of the isolated-mode tests (tests/test_isolated_host.py, tests/test_isolated_batch.py): batches with
exact frame and phoneme counts whose control tensors hold NON-ZERO garbage behind ``lengths``, and the checker -- the CPU
oracle run on one utterance ALONE with its unpadded inputs, which is what the reference's callers do (one utterance
per call).  Not a test module."""
import numpy as np

INTER = 192
GARBAGE = dict(duration=7.0, f0=333.0, energy=77.0)      # what a careless caller leaves behind `lengths`
SCALARS = dict(duration=0.25, pitch=1.1, energy=0.9)     # the scalar controls of the predictor cases

# which controls are tensors: (duration, pitch, energy)
MODES = {"controls": (True, True, True), "predictors": (True, False, False), "all_predicted": (False, False, False)}


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def make_batch(frames, phonemes, seed, tp=None, t_f=None):
    """Utterance b has exactly ``phonemes[b]`` phonemes and ``frames[b]`` frames (as the sum of its durations); every
    control tensor holds GARBAGE behind ``lengths``; noise [B, 192, max(t_f, max(frames))]."""
    r = np.random.Generator(np.random.PCG64(seed))
    frames, lengths = np.asarray(frames, np.int64), np.asarray(phonemes, np.int64)
    B, tp = len(frames), int(tp or lengths.max())
    ph = r.integers(1, 200, size=(B, tp)).astype(np.int64)             # (ids behind `lengths` are garbage too)
    dur = np.full((B, tp), GARBAGE["duration"], np.float32)
    f0 = np.full((B, tp), GARBAGE["f0"], np.float32)
    en = np.full((B, tp), GARBAGE["energy"], np.float32)
    for b in range(B):
        n, L = int(lengths[b]), int(frames[b])
        cut = np.sort(r.integers(0, L + 1, size=n - 1))
        dur[b, :n] = np.diff(np.concatenate([[0], cut, [L]]))
        v = r.uniform(150.0, 400.0, size=n)
        v[r.random(n) < 0.10] = 0.0
        f0[b, :n] = v
        en[b, :n] = r.uniform(0.0, 100.0, size=n)
    tf = max(int(frames.max()), int(t_f or 0))
    return dict(phonemes=ph, lengths=lengths, sid=r.integers(0, 67, size=B).astype(np.int64), duration=dur, f0=f0, energy=en,
                frame_lengths=frames, noise=r.standard_normal((B, INTER, tf), dtype=np.float32))


def controls(batch, mode, sl=slice(None), n=None):
    """(duration_control, pitch_control, energy_control) of ``mode`` for utterances ``sl``, cut to ``n`` phonemes."""
    use = MODES[mode]
    cut = lambda a: a[sl] if n is None else a[sl, :n]
    return (cut(batch["duration"]) if use[0] else SCALARS["duration"], cut(batch["f0"]) if use[1] else SCALARS["pitch"],
            cut(batch["energy"]) if use[2] else SCALARS["energy"])


def alone(oracle, batch, b, mode, noise_scale=0.667, max_len=None, noise=None):
    """The oracle on utterance ``b`` alone: B = 1, its own phonemes / controls, noise[b][:, :L_b].  With predicted
    durations L_b is the oracle's own count and the noise is the caller's first L_b columns."""
    n = int(batch["lengths"][b])
    sl = slice(b, b + 1)
    d, p, e = controls(batch, mode, sl, n)
    enc = oracle.encode(batch["phonemes"][sl, :n], batch["lengths"][sl], batch["sid"][sl], d, p, e)
    L = int(enc["frame_lengths"][0])
    nz = (batch["noise"] if noise is None else noise)[sl, :, :L]
    out = oracle.decode(enc, nz, noise_scale, max_len)
    out.update(enc)
    return {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in out.items()}, n, L


def padded(oracle, batch, mode, noise_scale=0.667):
    """The oracle on the padded batch (the reference's batched call): what isolated mode deliberately does NOT compute."""
    d, p, e = controls(batch, mode)
    return oracle.infer(batch["phonemes"], batch["lengths"], batch["sid"], noise=batch["noise"], noise_scale=noise_scale,
                        duration_control=d, pitch_control=p, energy_control=e)
