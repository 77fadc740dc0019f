"""Shared helpers of the per-row-control tests (tests/test_row_controls_host.py, tests/test_row_controls_gpu.py): the
checker of a batch that runs with a row table -- the CPU oracle on one utterance ALONE with ITS OWN arguments
(tests/isolated_ref.alone, generalised from one mode per batch to one set of arguments per row) -- the table of the
golden fixture, and the fixture's margin condition on predicted durations.  Not a test module."""
import os

import numpy as np

import isolated_ref as iso      # (rel_err, make_batch: shared with the isolated-mode tests)

STAGE_TOL, WAVE_TOL = 1e-5, 1e-4      # the project's isolated-mode gates (tests/test_isolated_batch.py)


def table(duration_scale, pitch_scale, energy_scale, noise_scale, given):
    from vispeech_amd.models import RowControls
    return RowControls(duration_scale, pitch_scale, energy_scale, noise_scale, given)


def take(rows, idx):
    """Rows ``idx`` of a table, in that order."""
    idx = list(idx)
    return table(rows.duration_scale[idx], rows.pitch_scale[idx], rows.energy_scale[idx], rows.noise_scale[idx], rows.given[idx])


def load_golden(golden_dir):
    """(batch arrays, table, expected arrays) of tests/golden/row_controls.npz."""
    g = np.load(os.path.join(golden_dir, "row_controls.npz"))
    batch = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    rows = table(batch.pop("duration_scale"), batch.pop("pitch_scale"), batch.pop("energy_scale"), batch.pop("noise_scale"),
                 batch.pop("given"))
    return batch, rows, {k: g[k] for k in g.files if not k.startswith("in_")}


def row_arguments(batch, rows, b, n):
    """(duration_control, pitch_control, energy_control, noise_scale) of utterance ``b``'s own B = 1 call."""
    sl = slice(b, b + 1)
    pick = lambda k, key, scale: batch[key][sl, :n] if rows.given[b, k] else float(scale[b])
    return (pick(0, "duration", rows.duration_scale), pick(1, "f0", rows.pitch_scale), pick(2, "energy", rows.energy_scale),
            float(rows.noise_scale[b]))


def alone(oracle, batch, rows, b, noise=None):
    """The oracle on utterance ``b`` alone with row b's arguments: B = 1, its own phonemes, noise[b][:, :L_b]."""
    n = int(batch["lengths"][b])
    sl = slice(b, b + 1)
    d, p, e, ns = row_arguments(batch, rows, b, n)
    enc = oracle.encode(batch["phonemes"][sl, :n], batch["lengths"][sl], batch["sid"][sl], d, p, e)
    L = int(enc["frame_lengths"][0])
    nz = (batch["noise"] if noise is None else noise)[sl, :, :L]
    out = oracle.decode(enc, nz, ns)
    out.update(enc)
    return {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in out.items()}, n, L


def assert_margin(logw, scale):
    """The fixture's condition on the INPUTS of a predicted-duration row: every (exp(logw) - 1) * scale lies at least
    10 * 1e-5 * max|logw| * max(exp(logw)) * scale away from an integer, so a logw within the stage gate cannot flip a ceil."""
    logw = np.asarray(logw, dtype=np.float64).reshape(-1)
    w = (np.exp(logw) - 1.0) * scale
    margin = 10 * STAGE_TOL * np.abs(logw).max() * np.exp(logw).max() * scale
    nearest = float(np.abs(w - np.rint(w)).min())
    assert nearest >= margin, (nearest, margin)
