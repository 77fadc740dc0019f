"""A size and its run agree: every entry point of the stand-alone audio operators (prosody, align, loudness, limiter)
carves its workspace by the function whose dry pass is ``vsp_*_workspace_bytes`` (csrc/op_host.h).

Host part (no kernel is launched; every device pointer is one no kernel may ever see).  Rows that pass every check, all at
the call's maxima.  Where a size function is the dry pass of the call itself, a workspace one byte shorter than its value
is refused with ``VSP_ERR_WORKSPACE`` and the message holds that same number.  A call that needs the head of a workspace
only (the rows' upload: the gate, the apply, the calls over a set of streams, the true-peak meter, the path and the
durations alone) has no size function of its own: what it asks for in its message must be covered by the size the header
and ``Engine`` use for it, and one byte less than what it asks for is refused.

GPU part.  B = 3 uneven rows, so that the 256-byte roundings differ from row to row; the workspace is the size function's
value with 4096 guard bytes of a pattern behind it; the call returns 0 and after a synchronise the guard is untouched.
The denoiser is left out: it needs a context with loaded weights; ``test_denoiser_gpu.py`` builds one in a fixture of
module scope, which this module could only import and so build a second time.  It keeps the model's ``run_sized`` path,
which ``test_workspace_overlay_host.py`` pins."""
import ctypes as C
import re

import numpy as np
import pytest

from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

BAD = 8                                 # a pointer no kernel may ever see
WORKSPACE = -6                          # VSP_ERR_WORKSPACE
GUARD, PATTERN = 4096, 0xA5
B = 3
I64 = lambda v: (C.c_int64 * len(v))(*[int(x) for x in v])


class Host:
    """Every device buffer is BAD: the refusals under test are decided before a device is needed."""
    def f32(self, *shape): return BAD
    f64 = i32 = i64 = zeros_i32 = f32


class Device:
    def __init__(self, torch):
        self.torch, self.keep, self.gen = torch, [], torch.Generator(device="cpu").manual_seed(7)

    def _new(self, t):
        t = t.to("cuda:0").contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def f32(self, *shape): return self._new(0.1 + 0.4 * self.torch.rand(shape, generator=self.gen, dtype=self.torch.float32))
    def f64(self, *shape): return self._new(0.1 + 0.4 * self.torch.rand(shape, generator=self.gen, dtype=self.torch.float64))
    def i32(self, *shape): return self._new(self.torch.zeros(shape, dtype=self.torch.int32))
    def i64(self, *shape): return self._new(self.torch.zeros(shape, dtype=self.torch.int64))
    zeros_i32 = i32


# ------------------------------------------------------------------------------------------------------------ the calls
# A builder returns (need, exact, call): `need` the size function's value for the call, `exact` whether that function is
# the call's own dry pass, call(workspace, workspace_bytes) -> rc.  `top`: the rows sit at the call's maxima.
def _loudness(fs):
    h = (fs + 5) // 10
    uneven = [2 * h + 7, h, 5 * h]
    L, S, T = 5 * h, 5, 5

    def rows(top): return I64([L] * B if top else uneven)
    def lp(): return (_lib.VspLoudnessParams * B)(*[_lib.VspLoudnessParams(-23.0, 1.0, 30.0)] * B)
    def lv(): return (_lib.VspLoudnessLevelParams * B)(*[_lib.VspLoudnessLevelParams(-23.0, 12.0, 12.0, 3.0, 0.0)] * B)

    def time_rows(d, top, **extra):
        count = [S] * B if top else [2, 1, S]
        return (_lib.VspLoudnessRow * B)(*[_lib.VspLoudnessRow(seg=d.f64(S), M=d.f32(S), S=d.f32(S), I=d.f32(S), kept=d.i32(S), c_db=d.f32(S),
                                                               c=d.f32(S), first=0, count=count[b], entries=S, **extra) for b in range(B)])

    def segments(lib, h_, s, d, top):
        return lib.vsp_loudness_workspace_bytes(B, L, fs), True, lambda ws, n: lib.vsp_loudness_segments(
            h_, s, B, L, fs, d.f32(B, L), L, rows(top), d.f64(B, S), d.f32(B), ws, n)

    def segments_from(lib, h_, s, d, top):
        return lib.vsp_loudness_workspace_bytes(B, L, fs), True, lambda ws, n: lib.vsp_loudness_segments_from(
            h_, s, B, L, fs, d.f32(B, L), L, rows(top), I64([0, h, 3 * h]), d.f64(B, 4), d.f64(B, 4), d.f64(B, S), d.f32(B), ws, n)

    def gate(lib, h_, s, d, top):
        return lib.vsp_loudness_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN), False, lambda ws, n: lib.vsp_loudness_gate(
            h_, s, B, S, fs, d.f64(B, S), rows(top), d.f32(B), lp(), d.f32(B), d.i32(B, 2), d.f32(B), ws, n)

    def apply(lib, h_, s, d, top):
        return lib.vsp_loudness_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN), False, lambda ws, n: lib.vsp_loudness_apply(
            h_, s, B, L, d.f32(B, L), L, d.f32(B, L), L, rows(top), d.f32(B), lp(), ws, n)

    def normalize(lib, h_, s, d, top):
        return lib.vsp_loudness_workspace_bytes(B, L, fs), True, lambda ws, n: lib.vsp_loudness_normalize(
            h_, s, B, L, fs, d.f32(B, L), L, d.f32(B, L), L, rows(top), lp(), d.f32(B), d.f32(B), d.f32(B), d.i32(B, 2), ws, n)

    def time(lib, h_, s, d, top):
        return lib.vsp_loudness_time_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN), False, lambda ws, n: lib.vsp_loudness_time(
            h_, s, B, fs, time_rows(d, top), d.f32(B), d.f32(B), ws, n)

    def level_gains(lib, h_, s, d, top):
        return lib.vsp_loudness_time_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN), False, lambda ws, n: lib.vsp_loudness_level_gains(
            h_, s, B, time_rows(d, top), lv(), ws, n)

    def level_apply(lib, h_, s, d, top):
        def call(ws, n):
            r = (_lib.VspLoudnessRow * B)(*[_lib.VspLoudnessRow(c=d.f32(S), entries=S, inp=d.f32(L), out=d.f32(L), pos=0, samples=k)
                                            for k in rows(top)])
            return lib.vsp_loudness_level_apply(h_, s, B, fs, r, lv(), ws, n)
        return lib.vsp_loudness_time_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN), False, call

    def level(lib, h_, s, d, top):
        return lib.vsp_loudness_time_workspace_bytes(B, L, fs), True, lambda ws, n: lib.vsp_loudness_level(
            h_, s, B, L, fs, d.f32(B, L), L, d.f32(B, L), L, rows(top), lv(), d.f32(B, T), d.f32(B, T), d.f32(B, T), d.i32(B, T), d.f32(B, T),
            d.f32(B, T), T, d.f32(B), d.f32(B), d.f32(B), d.f32(B), ws, n)

    def time_hist(lib, h_, s, d, top):
        return lib.vsp_loudness_hist_workspace_bytes(B, 1, _lib.LOUDNESS_FS_MIN), False, lambda ws, n: lib.vsp_loudness_time_hist(
            h_, s, B, fs, time_rows(d, top), (C.c_void_p * B)(*[d.zeros_i32(2, _lib.LOUDNESS_HIST_BINS) for _ in range(B)]), d.f32(B), d.f32(B),
            d.f32(B), ws, n)

    def range_(lib, h_, s, d, top):
        return lib.vsp_loudness_hist_workspace_bytes(B, L, fs), True, lambda ws, n: lib.vsp_loudness_range(
            h_, s, B, L, fs, d.f32(B, L), L, rows(top), d.f32(B), d.f32(B), d.f32(B, T), d.f32(B, T), d.f32(B, T), d.i32(B, T), T, ws, n)

    calls = dict(segments=segments, segments_from=segments_from, gate=gate, apply=apply, normalize=normalize, time=time,
                 level_gains=level_gains, level_apply=level_apply, level=level, time_hist=time_hist, range=range_)
    return {f"loudness_{k}[{fs}]": v for k, v in calls.items()}


def _limiter(A, H):
    uneven, L = [3000, 1, 2000], 3000

    def rows_call(lib, h_, s, d, top):
        def call(ws, n):
            r = (_lib.VspLimiterRow * B)(*[_lib.VspLimiterRow(d.f32(k), 0, k, d.f32(k), 0, k, k, 0.5) for k in ([L] * B if top else uneven)])
            return lib.vsp_limiter_rows(h_, s, B, A, H, r, None, d.f32(B), ws, n)
        return lib.vsp_limiter_workspace_bytes(B, L, A, H), True, call

    def true_peak(lib, h_, s, d, top):
        return lib.vsp_limiter_workspace_bytes(B, 1, 0, 0), False, lambda ws, n: lib.vsp_true_peak(
            h_, s, B, L, d.f32(B, L), L, I64([L] * B if top else uneven), d.f32(B), ws, n)

    out = {f"limiter_rows[{A},{H}]": rows_call}
    if (A, H) == (0, 0):
        out["true_peak"] = true_peak
    return out


def _align():
    Cc, Fm, Km, Tp = 8, 40, 30, 12

    def fk(top): return ([Fm] * B, [Km] * B) if top else ([40, 17, 33], [30, 9, 12])
    def cum(K):
        ln = [12, 5, 12]
        c = np.zeros((B, Tp), np.int32)
        for b in range(B):
            c[b, :ln[b]] = [-(-(i + 1) * K[b] // ln[b]) for i in range(ln[b])]
        return c.ctypes.data_as(C.POINTER(C.c_int32)), c, I64(ln)

    def scores(lib, h_, s, d, top):
        F, K = fk(top)
        return lib.vsp_align_scores_workspace_bytes(B, Fm, Km), True, lambda ws, n: lib.vsp_align_scores(
            h_, s, B, Cc, Fm, Km, d.f32(B, Cc, Fm), d.f32(B, Cc, Km), d.f32(B, Cc, Km), I64(F), I64(K), d.f32(B, Fm, Km), ws, n)

    def path(lib, h_, s, d, top):
        F, K = fk(top)
        return lib.vsp_align_path_workspace_bytes(B, Fm, Km), True, lambda ws, n: lib.vsp_align_path(
            h_, s, B, Fm, Km, d.f32(B, Fm, Km), I64(F), I64(K), None, d.i32(B, Fm), ws, n)

    def durations(lib, h_, s, d, top):
        F, K = fk(top)
        p, keep, ln = cum(K)
        return lib.vsp_align_workspace_bytes(B, Fm, Km, Tp), False, lambda ws, n, keep=keep: lib.vsp_align_durations(
            h_, s, B, Fm, Tp, d.i32(B, Fm), I64(F), p, ln, d.i32(B, Tp), ws, n)

    def align(lib, h_, s, d, top):
        F, K = fk(top)
        p, keep, ln = cum(K)
        return lib.vsp_align_workspace_bytes(B, Fm, Km, Tp), True, lambda ws, n, keep=keep: lib.vsp_align(
            h_, s, B, Cc, Fm, Km, Tp, d.f32(B, Cc, Fm), d.f32(B, Cc, Km), d.f32(B, Cc, Km), I64(F), I64(K), p, ln, None, d.i32(B, Fm),
            d.i32(B, Tp), ws, n)

    return dict(align_scores=scores, align_path=path, align_durations=durations, align=align)


def _prosody():
    hop, Tp, L, uneven = 512, 8, 4096, [4096, 641, 3000]
    Fm = L // hop + 1

    def rows(top): return [L] * B if top else uneven

    def contours(lib, h_, s, d, top):
        return lib.vsp_prosody_workspace_bytes(B, L, hop, Tp, None), True, lambda ws, n: lib.vsp_prosody_contours(
            h_, s, B, L, hop, d.f32(B, L), L, I64(rows(top)), None, d.f32(B, Fm), d.f32(B, Fm), d.i64(B), ws, n)

    def candidates(lib, h_, s, d, top):
        return lib.vsp_prosody_workspace_bytes(B, L, hop, Tp, None), True, lambda ws, n: lib.vsp_prosody_candidates(
            h_, s, B, L, hop, d.f32(B, L), L, I64(rows(top)), None, _lib.PROSODY_MAX_CANDIDATES, d.f32(B, Fm, 16), d.f32(B, Fm, 16),
            d.f32(B, Fm), d.i64(B), ws, n)

    def path(lib, h_, s, d, top):
        return lib.vsp_prosody_path_workspace_bytes(B, L, hop, None, None), False, lambda ws, n: lib.vsp_prosody_path(
            h_, s, B, Fm, hop, d.f32(B, Fm, 16), d.f32(B, Fm, 16), I64([k // hop + 1 for k in rows(top)]), None, d.f32(B, Fm), ws, n)

    def contours_path(lib, h_, s, d, top):
        return lib.vsp_prosody_path_workspace_bytes(B, L, hop, None, None), True, lambda ws, n: lib.vsp_prosody_contours_path(
            h_, s, B, L, hop, d.f32(B, L), L, I64(rows(top)), None, None, d.f32(B, Fm), d.f32(B, Fm), d.i64(B), ws, n)

    def phonemes(lib, h_, s, d, top):
        # the size is the larger of the contour call's and this call's: at 9 frames the contours' (this call is covered by
        # it), at 2000 frames this call's own
        F = 2000 if top else Fm
        frames = [F] * B if top else [k // hop + 1 for k in uneven]
        ln = [8, 2, 5]
        dur = np.zeros((B, Tp), np.int64)
        for b in range(B):
            dur[b, :ln[b]] = 1
        return lib.vsp_prosody_workspace_bytes(B, hop * (F - 1), hop, Tp, None), top, lambda ws, n, dur=dur: lib.vsp_prosody_phonemes(
            h_, s, B, F, Tp, d.f32(B, F), d.f32(B, F), I64(frames), dur.ctypes.data_as(C.POINTER(C.c_int64)), I64(ln), d.f32(B, Tp),
            d.f32(B, Tp), ws, n)

    return dict(prosody_contours=contours, prosody_candidates=candidates, prosody_path=path, prosody_contours_path=contours_path,
                prosody_phonemes=phonemes)


CASES = {**_prosody(), **_align(), **_loudness(8000), **_loudness(44100), **_limiter(66, 882), **_limiter(0, 0)}


# ------------------------------------------------------------------------------------------------------------ host part
@pytest.fixture(scope="module")
def ctx():
    lib = _lib.lib()
    cfg = _lib.make_config(ModelDims())
    h = C.c_void_p()
    assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0
    yield lib, h
    lib.vsp_destroy(h)


def _asked(lib, h):
    m = re.search(rb"the workspace needs (\d+) bytes", lib.vsp_last_error(h))
    assert m, lib.vsp_last_error(h)
    return int(m.group(1))


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_byte_less_than_the_size_is_refused_and_the_message_holds_the_size(ctx, name):
    lib, h = ctx
    need, exact, call = CASES[name](lib, h, None, Host(), True)
    assert need > 0
    if not exact:                          # a head-only call: what it asks for is covered by the size used for it
        assert call(BAD, 0) == WORKSPACE
        assert 0 < _asked(lib, h) <= need
        need = _asked(lib, h)
    assert call(BAD, need - 1) == WORKSPACE, lib.vsp_last_error(h)
    assert _asked(lib, h) == need
    assert call(None, need) == WORKSPACE and _asked(lib, h) == need      # (a NULL workspace, whatever its size)


# ------------------------------------------------------------------------------------------------------------- GPU part
@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd.engine import Engine
    return Engine(ModelDims(), "cuda:0")                   # (none of these operators needs weights)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_run_on_exactly_the_size_leaves_the_guard_behind_it_untouched(eng, name):
    import torch
    dev = Device(torch)
    need, _, call = CASES[name](eng.lib, eng.ctx, eng._stream(), dev, False)
    assert need > 0
    ws = torch.full((need + GUARD,), PATTERN, dtype=torch.uint8, device="cuda:0")
    with torch.cuda.device("cuda:0"):
        rc = call(ws.data_ptr(), need)
    assert rc == 0, eng.lib.vsp_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert bool((ws[need:] == PATTERN).all()), f"{name}: the call wrote behind its {need} bytes"
