"""The path finder's specification restated in fp64 numpy: every frame's candidates, the best path
through a candidate table, and every frame's max-marginal.  Built on the autocorrelation helpers of tests/prosody_ref.py
(section 4m's quantities are that file's); nothing here is shared with the library.

A table is ``(cand_f, cand_s)``, both ``[F, 16]``: slot 0 the unvoiced candidate (0, U), slots 1.. the strongest voiced
candidates (f, S) in descending S (the lower lag first among equals), unused slots (0, -inf)."""
from __future__ import annotations

import numpy as np

import prosody_ref as ref
from prosody_ref import FS, HOP

SLOTS, MAX_CANDIDATES = 16, 15
PATH_DEFAULTS = dict(octave_jump_cost=0.35, voiced_unvoiced_cost=0.14)


def kappa(hop: int = HOP) -> float:
    """Praat's time-step correction 0.01 fs / hop (exactly 1 where fs = 100 hop)."""
    return FS / (100.0 * hop)


def candidates(x, hop: int = HOP, max_candidates: int = MAX_CANDIDATES, floor=80.0, ceiling=750.0, voicing_threshold=0.6,
               silence_threshold=0.03, octave_cost=0.01, with_curvature: bool = False):
    """``(cand_f, cand_s, lags, gap)`` of one recording: the two tables ``[F, 16]``; the integer lag behind every voiced slot
    (0 in slot 0, -1 where unused); and per frame the strength of the last maximum kept minus that of the first left out
    (inf where none is left out) -- below a threshold, fp32 may rightly keep the other one.  ``with_curvature``: also
    ``[F, 16]`` |r(t - 1) - 2 r(t) + r(t + 1)| of every voiced slot (inf elsewhere): the parabola divides by it, so an error
    eps in r moves the refined lag by about eps / curvature."""
    assert 2 <= max_candidates <= MAX_CANDIDATES
    x = np.asarray(x, np.float64)
    F = ref.frames(len(x), hop)
    W = ref.window_samples(floor)
    tmin, tmax = int(np.floor(FS / ceiling)), int(np.ceil(FS / floor))
    gpk = np.abs(x - x.mean()).max()
    xz = np.concatenate([np.zeros(W // 2), x, np.zeros(W // 2 + hop)])
    s = np.stack([xz[hop * k: hop * k + W] for k in range(F)])
    s = s - s.mean(1, keepdims=True)
    lpk = np.abs(s).max(1)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(W) + 0.5) / W)
    ra = ref._autocorr(s * w, tmax + 2)
    rw = np.array([np.dot(w[: W - t], w[t:]) for t in range(tmax + 2)])
    inv_rw = (rw[0] / rw).astype(np.float32).astype(np.float64)         # the specification's float32 table
    cand_f = np.zeros((F, SLOTS))
    cand_s = np.full((F, SLOTS), -np.inf)
    lags = np.full((F, SLOTS), -1, np.int64)
    lags[:, 0] = 0
    gap = np.full(F, np.inf)
    curvature = np.full((F, SLOTS), np.inf)
    t = np.arange(tmin, tmax + 1)
    nv = max_candidates - 1
    for k in range(F):
        if not gpk > 0 or not ra[k, 0] > 0:
            cand_s[k, 0] = voicing_threshold + 2.0                     # a dead frame: the unvoiced candidate alone
            continue
        cand_s[k, 0] = voicing_threshold + max(0.0, 2.0 - (lpk[k] / gpk) / (silence_threshold / (1.0 + voicing_threshold)))
        r = ra[k] / ra[k, 0] * inv_rw
        rm, r0, rp = r[t - 1], r[t], r[t + 1]
        c = (r0 > rm) & (r0 >= rp)
        if not c.any():
            continue
        rm, r0, rp, tc = rm[c], r0[c], rp[c], t[c]
        d = 0.5 * (rm - rp) / (rm - 2.0 * r0 + rp)
        R = r0 - 0.25 * (rm - rp) * d
        f = FS / (tc + d)
        S = R + octave_cost * np.log2(f / floor)
        order = np.lexsort((tc, -S))                                    # descending S, the lower lag first among equals
        keep = order[:nv]
        cand_f[k, 1: 1 + len(keep)] = f[keep]
        cand_s[k, 1: 1 + len(keep)] = S[keep]
        lags[k, 1: 1 + len(keep)] = tc[keep]
        curvature[k, 1: 1 + len(keep)] = np.abs(rm - 2.0 * r0 + rp)[keep]
        if len(order) > nv:
            gap[k] = S[order[nv - 1]] - S[order[nv]]
    return (cand_f, cand_s, lags, gap, curvature) if with_curvature else (cand_f, cand_s, lags, gap)


def transition(fa, fb, hop: int = HOP, octave_jump_cost=0.35, voiced_unvoiced_cost=0.14) -> np.ndarray:
    """T[p, c] between the candidates of one frame (``fa``) and of the next (``fb``); f = 0 (or below) is unvoiced."""
    fa, fb = np.asarray(fa, np.float64), np.asarray(fb, np.float64)
    ua, ub = ~(fa > 0), ~(fb > 0)
    octaves = np.abs(np.log2(np.where(ua, 1.0, fa)[:, None] / np.where(ub, 1.0, fb)[None, :]))
    k = kappa(hop)
    return np.where(ua[:, None] & ub[None, :], 0.0,
                    np.where(ua[:, None] | ub[None, :], voiced_unvoiced_cost * k, octave_jump_cost * k * octaves))


def best_path(cand_f, cand_s, frames=None, hop: int = HOP, **path):
    """``(f0, choice)`` of one row: the path through its first ``frames`` frames (None: all) that maximises the summed delta
    minus the summed transition costs -- forward recursion, every frame's scores normalised by their maximum, the lowest
    previous candidate among equals, the lowest candidate among equals at the end.  f0 has the table's length, zeros behind
    ``frames``; ``choice`` has ``frames`` entries."""
    cand_f, cand_s = np.asarray(cand_f, np.float64), np.asarray(cand_s, np.float64)
    F = len(cand_f) if frames is None else int(frames)
    assert 1 <= F <= len(cand_f)
    N = cand_f.shape[1]
    back = np.zeros((F, N), np.int64)
    s = cand_s[0].copy()
    with np.errstate(invalid="ignore"):
        for k in range(F):
            if k > 0:
                v = s[:, None] - transition(cand_f[k - 1], cand_f[k], hop, **path)         # [p, c]
                back[k] = np.argmax(v, axis=0)                                             # (the first maximum: the lowest p)
                s = cand_s[k] + v[back[k], np.arange(N)]
            if s.max() > -np.inf:
                s = s - s.max()
    choice = np.zeros(F, np.int64)
    choice[F - 1] = int(np.argmax(s))
    for k in range(F - 1, 0, -1):
        choice[k - 1] = back[k, choice[k]]
    f0 = np.zeros(len(cand_f))
    f0[:F] = cand_f[np.arange(F), choice]
    return f0, choice


def path_margins(cand_f, cand_s, frames=None, hop: int = HOP, **path) -> np.ndarray:
    """Per frame, the best total of a path through the chosen candidate minus the best total through any other candidate of
    that frame (max-marginals: forward plus backward scores; inf where the frame has one candidate).  A frame whose
    margin is small is one where fp32 may rightly choose otherwise."""
    cand_f, cand_s = np.asarray(cand_f, np.float64), np.asarray(cand_s, np.float64)
    F = len(cand_f) if frames is None else int(frames)
    N = cand_f.shape[1]
    _, choice = best_path(cand_f, cand_s, F, hop, **path)
    T = [transition(cand_f[k - 1], cand_f[k], hop, **path) for k in range(1, F)]          # T[k - 1]: frame k - 1 -> k
    fwd = np.zeros((F, N))
    bwd = np.zeros((F, N))
    fwd[0] = cand_s[0]
    with np.errstate(invalid="ignore"):
        for k in range(1, F):
            fwd[k] = cand_s[k] + (fwd[k - 1][:, None] - T[k - 1]).max(axis=0)
        for k in range(F - 2, -1, -1):
            bwd[k] = ((cand_s[k + 1] + bwd[k + 1])[None, :] - T[k]).max(axis=1)
    through = fwd + bwd
    margin = np.full(F, np.inf)
    for k in range(F):
        others = np.delete(through[k], choice[k])
        others = others[others > -np.inf]
        if len(others):
            margin[k] = through[k, choice[k]] - others.max()
    return margin


def brute_force(cand_f, cand_s, hop: int = HOP, **path):
    """Every path of a small table, enumerated: ``(the best total, the first path in lexicographic order that reaches it)``."""
    import itertools
    cand_f, cand_s = np.asarray(cand_f, np.float64), np.asarray(cand_s, np.float64)
    F, N = cand_f.shape
    T = [transition(cand_f[k - 1], cand_f[k], hop, **path) for k in range(1, F)]
    best, best_c = -np.inf, None
    for c in itertools.product(range(N), repeat=F):
        total = sum(cand_s[k, c[k]] for k in range(F)) - sum(T[k - 1][c[k - 1], c[k]] for k in range(1, F))
        if total > best:
            best, best_c = total, c
    return best, best_c


def path_total(cand_f, cand_s, choice, hop: int = HOP, **path) -> float:
    cand_f, cand_s = np.asarray(cand_f, np.float64), np.asarray(cand_s, np.float64)
    total = sum(cand_s[k, c] for k, c in enumerate(choice))
    return total - sum(transition(cand_f[k - 1], cand_f[k], hop, **path)[choice[k - 1], choice[k]] for k in range(1, len(choice)))


# ---------------------------------------------------------------------------------------------- test signals
F_STEADY = 220.5                      # period 200 samples: the lags 100, 200 and 400 are whole
OCTAVE_FRAMES = (14, 15, 16)          # the frames of `octave_signal` whose windows hold even partials alone
DIP_FRAMES = (15,)                    # the frame of `dip_signal` whose window lies in the dip


def octave_signal(n: int = 30 * HOP + 100) -> np.ndarray:
    """(a) A harmonic complex at F_STEADY whose odd partials are switched off over the windows of OCTAVE_FRAMES: there the
    signal has period 100 as well as 200, the lag-100 peak wins every such frame by the octave cost alone."""
    ph = 2.0 * np.pi * F_STEADY * np.arange(n) / FS
    odd = sum(0.6 ** h * np.sin(h * ph) for h in (1, 3, 5, 7))
    even = sum(0.6 ** h * np.sin(h * ph) for h in (2, 4, 6, 8))
    W = ref.window_samples(80.0)
    g = np.ones(n)
    g[OCTAVE_FRAMES[0] * HOP - W // 2: OCTAVE_FRAMES[-1] * HOP + W // 2 + 1] = 0.0
    return 0.25 * (g * odd + even)


def dip_signal(n: int = 30 * HOP + 100, depth: float = 0.1, width: int = 3000, sigma: float = 0.025, seed: int = 7) -> np.ndarray:
    """(b) A steady complex at F_STEADY over a noise floor, whose amplitude dips smoothly (a raised cosine of ``width`` samples)
    to ``depth`` around DIP_FRAMES: there the tone sinks towards the noise, the voiced strength falls below the voicing
    threshold for that frame, and stays well above it in its neighbours."""
    x = ref.harmonic(F_STEADY, n)
    i = np.arange(n) - DIP_FRAMES[0] * HOP
    env = np.where(np.abs(i) < width / 2, 1.0 - (1.0 - depth) * (0.5 + 0.5 * np.cos(2.0 * np.pi * i / width)), 1.0)
    return x * env + np.random.default_rng(seed).standard_normal(n) * sigma


# ---------------------------------------------------------------------------------------------- constructed tables
TABLE_FRAMES = (1, 2, 63, 64, 65, 130)        # ragged rows of one batch: one chunk of the kernel's 64, its edges, three chunks
TABLE_SEED = 3                                # (tests/test_prosody_path_host.py: at most 1 % of its frames have a margin below 1e-3)
TIE_HOP = 441                                 # kappa = 1 exactly


def empty_tables(frames=TABLE_FRAMES, behind=np.nan):
    """Tables ``[B, F_max, 16]`` float32 of unused slots (0, -inf); ``behind`` in both behind every row's frames (NaN: what
    must not be read poisons whatever reads it)."""
    B, F_max = len(frames), max(frames)
    cand_f = np.zeros((B, F_max, SLOTS), np.float32)
    cand_s = np.full((B, F_max, SLOTS), -np.inf, np.float32)
    for b, F in enumerate(frames):
        cand_f[b, F:], cand_s[b, F:] = behind, behind
    return cand_f, cand_s


def random_tables(n_used: int, seed: int = TABLE_SEED, frames=TABLE_FRAMES):
    """Slot 0 unvoiced, ``n_used - 1`` voiced slots of f in [80, 750) Hz (where a row's neighbours often lie an octave
    apart), delta uniform in [0, 3)."""
    rng = np.random.default_rng(seed)
    cand_f, cand_s = empty_tables(frames)
    for b, F in enumerate(frames):
        cand_f[b, :F, 1:n_used] = rng.uniform(80.0, 750.0, (F, n_used - 1))
        cand_s[b, :F, :n_used] = rng.uniform(0.0, 3.0, (F, n_used))
    return cand_f, cand_s


TIE_PATH = dict(octave_jump_cost=0.5, voiced_unvoiced_cost=1.0)


def tie_tables(seed: int = 5, frames=TABLE_FRAMES):
    """Exact ties: delta in {0, 1, 2}, f in {128, 256, 512} (log2 exact), six used slots, two of them unvoiced, and the same f
    in several slots of a frame; with TIE_PATH at TIE_HOP every score is a multiple of 0.5, exact in fp32 as in fp64."""
    rng = np.random.default_rng(seed)
    cand_f, cand_s = empty_tables(frames)
    for b, F in enumerate(frames):
        cand_f[b, :F, 1:5] = 2.0 ** rng.integers(7, 10, (F, 4))
        cand_s[b, :F, :6] = rng.integers(0, 3, (F, 6))                  # (slots 0 and 5: f = 0, both unvoiced)
    return cand_f, cand_s


# ---------------------------------------------------------------------------------------------- recordings
ROW_LENGTHS = (61 * HOP, 61 * HOP - 1, 20 * HOP + 300, 641)     # tones, glide, noise, silence (the minimum: 2 frames)
TONES = (90.0, 100.0, 220.5, 333.0, 441.0, 700.0)


def glide_row(n, seed=2):
    """180 + 60 sin(2 pi 1.5 t) Hz with 10 partials; hops 15-25 zeroed, hops 40-48 replaced by noise."""
    t = np.arange(n) / FS
    x = ref.harmonic(180.0 + 60.0 * np.sin(2.0 * np.pi * 1.5 * t), n, partials=10)
    x[15 * HOP: 26 * HOP] = 0.0
    x[40 * HOP: 49 * HOP] = np.random.default_rng(seed).standard_normal(9 * HOP) * 0.1
    return x


def main_rows():
    """The four kinds of row the contour tests use, as float32: six harmonic complexes spliced, a glide with a pause and a
    noise burst, noise (about a third of its lags are maxima: the selection of the strongest 14 is at work), silence."""
    n = ROW_LENGTHS[0]
    cuts = np.linspace(0, n, len(TONES) + 1).astype(int)
    tones = np.concatenate([ref.harmonic(f, b - a) for f, a, b in zip(TONES, cuts[:-1], cuts[1:])])
    rng = np.random.default_rng(1)
    rows = [tones, glide_row(ROW_LENGTHS[1]), rng.standard_normal(ROW_LENGTHS[2]) * 0.1, np.zeros(ROW_LENGTHS[3])]
    return [r.astype(np.float32) for r in rows]


def pad(rows, fill=0.0):
    a = np.full((len(rows), max(len(r) for r in rows)), fill, np.float32)
    for b, r in enumerate(rows):
        a[b, : len(r)] = r
    return a
