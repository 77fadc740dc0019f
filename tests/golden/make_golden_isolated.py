#!/usr/bin/env python3
"""Generate tests/golden/isolated.npz from the REAL reference, called the way its own callers call it: ONE utterance
per call (inference.py, inference_api.py, gui.py), with the utterance's unpadded inputs.

Four utterances of one batch -- 1, 14, 40 and 41 frames (T_f = 41), 2, 5, 9 and 9 phonemes (T_p = 9) -- each run alone,
twice: every control given ("controls") and durations given with pitch and energy PREDICTED ("predictors": predicted
durations would not give these frame counts).  The file holds arrays only: the batch (control tensors with non-zero
garbage behind `lengths`, tests/isolated_ref.py) and, per case, the alone results laid into padded tensors that are zero
behind every utterance's extent -- what isolated mode returns for the batch.

Runs only where the reference is checked out (imported read-only; nothing of it is copied):

    python tests/golden/make_golden_isolated.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import _Noise, build_reference     # noqa: E402  (also puts the repo and the reference on sys.path)
import isolated_ref as iso                            # noqa: E402

FRAMES, PHONEMES, NOISE_SCALE = [1, 14, 40, 41], [2, 5, 9, 9], 0.667


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    net, dims = build_reference()
    batch = iso.make_batch(FRAMES, PHONEMES, seed=1010)
    B, tp, tf, up = len(FRAMES), max(PHONEMES), max(FRAMES), 512
    out = {f"in_{k}": v for k, v in batch.items()}
    out["in_noise_scale"] = np.float32(NOISE_SCALE)
    for mode in ("controls", "predictors"):
        res = dict(o=np.zeros((B, 1, tf * up), np.float32), duration=np.zeros((B, tp), np.float32),
                   F0=np.zeros((B, tp), np.float32), energy=np.zeros((B, tp), np.float32),
                   **{k: np.zeros((B, dims.inter_channels, tf), np.float32) for k in ("z", "m_p", "logs_p")})
        for b in range(B):
            n, L = PHONEMES[b], FRAMES[b]
            sl = slice(b, b + 1)
            d, p, e = iso.controls(batch, mode, sl, n)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
            with torch.no_grad(), _Noise(np.ascontiguousarray(batch["noise"][sl, :, :L])):
                o, x_mask, (z, z_p, m_p, logs_p), duration, f0, energy = net.infer(
                    t(batch["phonemes"][sl, :n]), t(batch["lengths"][sl]), sid=t(batch["sid"][sl]), noise_scale=NOISE_SCALE,
                    duration_control=t(d), pitch_control=t(p), energy_control=t(e))
            assert x_mask.shape[2] == L and o.shape[2] == L * up
            res["o"][b, :, :L * up] = o[0].numpy()
            for k, v in (("z", z), ("m_p", m_p), ("logs_p", logs_p)):     # (z_p follows from m_p, logs_p and the noise)
                res[k][b, :, :L] = v[0].numpy()
            res["duration"][b, :n] = duration.reshape(-1).numpy()
            res["F0"][b, :n] = f0.reshape(-1).numpy()
            res["energy"][b, :n] = energy.reshape(-1).numpy()
        out.update({f"{mode}_{k}": v for k, v in res.items()})
    path = os.path.join(HERE, "isolated.npz")
    np.savez_compressed(path, **out)
    print(f"isolated: B={B} Tp={tp} Tf={tf} -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
