"""The alignment of a recording to a text restated in fp64 numpy: the Gaussian scores in the direct
form, the left-to-right path with at most ``max_advance`` states a frame (lowest advance among equals), and the per-phoneme
durations.  It is the specification the device code is held to, and it is judged on its own in tests/test_align_host.py
(every path enumerated on small tables).  Also here: the inputs the GPU tests use, so that the host tests can assert the
properties those tests rest on."""
import itertools

import numpy as np


# ---------------------------------------------------------------------------------------------- scores
def scores(x, m, logs, with_sums=False):
    """One row: ``x`` [C, F], ``m`` and ``logs`` [C, K] (any float type, widened exactly) -> ``S`` [F, K] float64,
    ``S[j][k] = sum_c -0.5 (x[c][j] - m[c][k])^2 exp(-2 logs[c][k]) - sum_c logs[c][k]``.  ``with_sums``: also
    ``sum_c |term_c|`` [F, K] and ``sum_c |logs_c|`` [K], what the error bound of an fp32 evaluation is made of."""
    x, m, logs = (np.asarray(a, dtype=np.float64) for a in (x, m, logs))
    d = x[:, :, None] - m[:, None, :]                                  # [C, F, K]
    term = -0.5 * d * d * np.exp(-2.0 * logs)[:, None, :]
    S = term.sum(axis=0) - logs.sum(axis=0)[None, :]
    if with_sums:
        return S, np.abs(term).sum(axis=0), np.abs(logs).sum(axis=0)
    return S


# ---------------------------------------------------------------------------------------------- path
def _shift(q, n, fill=-np.inf):
    """``q`` moved up by n states: entry k is ``q[k - n]``, ``fill`` below."""
    return np.concatenate((np.full(n, fill), q))[: len(q)]


def feasible(F, K, A):
    return F >= 1 and K >= 1 and K <= A * (F - 1) + 1


def best_path(S, max_advance=2, stay_cost=0.0, skip_cost=0.0, with_value=False):
    """``S`` [F, K] (float32 or float64; widened exactly) -> ``states`` [F] int32, the path of the specification: fp64
    accumulation, candidates in the order advance 0, 1, 2 with a strict comparison (the lowest advance among equals).  The
    costs go through float32 first, as the C structure carries them."""
    S = np.asarray(S, dtype=np.float64)
    F, K = S.shape
    A = int(max_advance)
    if A not in (1, 2):
        raise ValueError("max_advance must be 1 or 2")
    if not (stay_cost >= 0 and skip_cost >= 0):
        raise ValueError("costs must be at least 0")
    if not feasible(F, K, A):
        raise ValueError(f"infeasible: {F} frames, {K} states, max_advance {A}")
    stay, skip = float(np.float32(stay_cost)), float(np.float32(skip_cost))
    ninf = -np.inf
    q = np.full(K, ninf)
    q[0] = S[0, 0]
    back = np.zeros((F, K), dtype=np.int8)
    for j in range(1, F):
        p1 = _shift(q, 1)
        best = q - stay
        adv = np.zeros(K, dtype=np.int8)
        take = p1 > best
        best = np.where(take, p1, best)
        adv[take] = 1
        if A == 2:
            p2 = _shift(q, 2) - skip
            take = p2 > best
            best = np.where(take, p2, best)
            adv[take] = 2
        q = S[j] + best
        back[j] = adv
    states = np.zeros(F, dtype=np.int32)
    k = K - 1
    for j in range(F - 1, -1, -1):
        states[j] = k
        if j > 0:
            k -= int(back[j, k])
    assert k == 0
    if with_value:
        return states, float(q[K - 1])
    return states


def path_value(S, states, stay_cost=0.0, skip_cost=0.0):
    """The objective of one path, in fp64, accumulated in frame order as the forward pass does."""
    S = np.asarray(S, dtype=np.float64)
    stay, skip = float(np.float32(stay_cost)), float(np.float32(skip_cost))
    v = S[0, states[0]]
    for j in range(1, len(states)):
        a = int(states[j]) - int(states[j - 1])
        v = S[j, states[j]] + (v - (stay if a == 0 else skip if a == 2 else 0.0))
    return float(v)


def all_paths(F, K, A):
    """Every path of the specification for a small table: k(0) = 0, k(F - 1) = K - 1, advances in {0 .. A}."""
    out = []
    for adv in itertools.product(range(A + 1), repeat=F - 1):
        if sum(adv) == K - 1:
            out.append(np.concatenate(([0], np.cumsum(adv))).astype(np.int32) if F > 1 else np.zeros(1, np.int32))
    return out


# ---------------------------------------------------------------------------------------------- durations
def durations(states, cum_dur, length, Tp):
    """``states`` [F] (monotone), ``cum_dur`` the row's inclusive cumulative template frames, ``length`` its phonemes ->
    [Tp] int32: ``d_i = #{ j : cum_{i-1} <= k(j) < cum_i }``, 0 behind ``length``."""
    d = np.zeros(Tp, dtype=np.int32)
    prev = 0
    for i in range(int(length)):
        c = int(cum_dur[i])
        d[i] = int(np.count_nonzero((states >= prev) & (states < c)))
        prev = c
    return d


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
PATH_ROWS_A2 = [(1, 1), (2, 3), (64, 64), (65, 33), (130, 200), (63, 125)]      # (F, K); the last: all skips
PATH_ROWS_A1 = [(130, 130), (130, 1), (65, 40)]                                  # the first: the diagonal
COSTS = [(0.0, 0.0), (0.3, 0.7)]                                                 # (stay, skip)


def random_tables(rows, seed):
    """Random normal float32 score tables, one per (F, K) of ``rows``."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((F, K)).astype(np.float32) for F, K in rows]


def ties_table(F=65, K=40, seed=5):
    """Scores in {0, 1, 2}: with costs 0.5 and 1 every candidate is a multiple of 0.5, so equal candidates are common and
    exact in any float type."""
    return np.random.default_rng(seed).integers(0, 3, size=(F, K)).astype(np.float32)


def count_ties(S, max_advance, stay_cost, skip_cost):
    """Cells of the forward pass in which two finite candidates are equal and maximal."""
    S = np.asarray(S, dtype=np.float64)
    F, K = S.shape
    q = np.full(K, -np.inf)
    q[0] = S[0, 0]
    n = 0
    for j in range(1, F):
        c = [q - stay_cost, _shift(q, 1)]
        if max_advance == 2:
            c.append(_shift(q, 2) - skip_cost)
        c = np.stack(c)
        best = c.max(axis=0)
        n += int(np.count_nonzero(np.isfinite(best) & ((c == best).sum(axis=0) > 1)))
        q = S[j] + best
    return n


def pack(tables, F_max=None, K_max=None, fill=0.0):
    """Tables [F_b, K_b] -> one padded [B, F_max, K_max] float32 (``fill`` outside a row's extent), frames, states."""
    F_max = F_max or max(t.shape[0] for t in tables)
    K_max = K_max or max(t.shape[1] for t in tables)
    out = np.full((len(tables), F_max, K_max), fill, dtype=np.float32)
    for b, t in enumerate(tables):
        out[b, : t.shape[0], : t.shape[1]] = t
    return out, [t.shape[0] for t in tables], [t.shape[1] for t in tables]


SCORE_SIZES = (1, 63, 64, 65, 130)


def score_rows(C, seed):
    """The ragged batch of the score test: every (F, K) of SCORE_SIZES x SCORE_SIZES; m, x ~ N(0, 1), logs uniform in
    [-2, 1].  Returns per row (x [C, F], m [C, K], logs [C, K]) float32."""
    rng = np.random.default_rng(seed)
    rows = []
    for F in SCORE_SIZES:
        for K in SCORE_SIZES:
            rows.append((rng.standard_normal((C, F)).astype(np.float32), rng.standard_normal((C, K)).astype(np.float32),
                         rng.uniform(-2.0, 1.0, (C, K)).astype(np.float32)))
    return rows


def pack_inputs(rows, fill=np.nan):
    """Rows of (x, m, logs) -> padded x [B, C, F_max], m, logs [B, C, K_max] with ``fill`` behind every extent."""
    C = rows[0][0].shape[0]
    F_max, K_max = max(r[0].shape[1] for r in rows), max(r[1].shape[1] for r in rows)
    x = np.full((len(rows), C, F_max), fill, dtype=np.float32)
    m = np.full((len(rows), C, K_max), fill, dtype=np.float32)
    logs = np.full((len(rows), C, K_max), fill, dtype=np.float32)
    for b, (xr, mr, lr) in enumerate(rows):
        x[b, :, : xr.shape[1]] = xr
        m[b, :, : mr.shape[1]] = mr
        logs[b, :, : lr.shape[1]] = lr
    return x, m, logs, [r[0].shape[1] for r in rows], [r[1].shape[1] for r in rows]


def planted(C=192, K=40, F=55, seed=11):
    """A monotone k*(j) of 31 steps, 4 skips and 19 stays in random order (0 + 31 + 8 = K - 1, 1 + 54 = F) and a row in
    which x[:, j] = m[:, k*(j)] exactly: (x [C, F], m [C, K], logs [C, K], k* [F])."""
    rng = np.random.default_rng(seed)
    adv = np.array([1] * 31 + [2] * 4 + [0] * 19)
    rng.shuffle(adv)
    k = np.concatenate(([0], np.cumsum(adv))).astype(np.int32)
    assert len(k) == F and k[-1] == K - 1
    m = rng.standard_normal((C, K)).astype(np.float32)
    logs = rng.uniform(-2.0, 1.0, (C, K)).astype(np.float32)
    return m[:, k].copy(), m, logs, k
