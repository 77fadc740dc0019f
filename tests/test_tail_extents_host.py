"""The silence table's extents, host side (no GPU): the support arithmetic of the vocoder restated in Python gives
back = fwd = 13 and reach1 = 2 for configs/config.json and what ``vsp_generator_tail_extents`` reports for the five-stage
and the resblock "2" configurations, and the frame counts the change was proposed on follow from ``synth_batch``:
stage 0 computes utterance b to min(T, len + back + 1 + fwd) frames, the stages behind it to len + back + reach1 where
len + back + fwd <= T (vispeech_amd/csrc/kernels.h, gen_plan)."""
import ctypes as C

import numpy as np
import pytest

from vispeech_amd import _lib
from vispeech_amd import config as vcfg
from vispeech_amd.schema import ModelDims, dims_from_ctor

PRE_K = POST_K = 7           # conv_pre / conv_post (reference models.py:254, 268)


def resblock_support(dims, j):
    """One-sided support of ResBlock j in samples at its stage's rate (reference modules.py:210-223, 245-249)."""
    k, dil = dims.resblock_kernel_sizes[j], dims.resblock_dilation_sizes[j]
    if dims.resblock_kind == 2:
        return sum((k - 1) * d // 2 for d in dil[:2])
    return sum((k - 1) * d // 2 + (k - 1) // 2 for d in dil)


def support(dims, first, end):
    """[lo, hi]: the positions of stage end - 1's output that an impulse at position 0 of stage first's input reaches, and
    the positions per input position.  first == 0 starts in front of conv_pre; end == the stage count includes conv_post."""
    n = len(dims.upsample_rates)
    lo = hi = 0
    up = 1
    if first == 0:
        lo, hi = -((PRE_K - 1) // 2), (PRE_K - 1) // 2
    rb = max(resblock_support(dims, j) for j in range(len(dims.resblock_kernel_sizes)))
    for s, k in list(zip(dims.upsample_rates, dims.upsample_kernel_sizes))[first:end]:
        p = (k - s) // 2
        lo, hi, up = lo * s - p - rb, hi * s - p + k - 1 + rb, up * s
    if end >= n:
        lo, hi = lo - (POST_K - 1) // 2, hi + (POST_K - 1) // 2
    return lo, hi, up


def extents(dims):
    n = len(dims.upsample_rates)
    total = int(np.prod(dims.upsample_rates))
    lo, hi, up = support(dims, 0, n)
    assert up == total
    back, fwd = hi // total, (total - 1 - lo) // total
    lo1, _, _ = support(dims, 1, n)
    reach1 = max(1, (total - 1 - lo1) // total) if n > 1 else fwd + 1
    return back, fwd, reach1


def reported(dims):
    lib = _lib.lib()
    cfg = _lib.make_config(dims)
    h = C.c_void_p()
    rc = lib.vsp_create_ex(C.byref(cfg), dims.resblock_kind, 0, C.byref(h))
    try:
        assert rc == 0, lib.vsp_last_error(h)
        b, f, r = C.c_int(), C.c_int(), C.c_int()
        assert lib.vsp_generator_tail_extents(h, C.byref(b), C.byref(f), C.byref(r)) == 0
        b2, f2 = C.c_int(), C.c_int()
        assert lib.vsp_generator_frame_dependence(h, C.byref(b2), C.byref(f2)) == 0
        assert (b.value, f.value) == (b2.value, f2.value)
        assert lib.vsp_generator_tail_extents(h, None, C.byref(f), C.byref(r)) == -1
        return b.value, f.value, r.value
    finally:
        lib.vsp_destroy(h)


def dims_for(**model):
    hp = vcfg.default_hparams()
    for k, v in model.items():
        hp.model[k] = v
    args, kwargs = vcfg.synthesizer_args(hp)
    return dims_from_ctor(*args, **kwargs)


def test_default_config_is_13_13_2():
    dims = ModelDims()
    assert extents(dims) == (13, 13, 2)
    assert reported(dims) == (13, 13, 2)
    # the figures the extent rests on: from stage 0's output on, 64 samples per column, an impulse reaches [-696, 759]
    assert support(dims, 1, 4) == (-696, 759, 64)


@pytest.mark.parametrize("model", [
    dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512),
    dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512, resblock="2"),
    dict(resblock="2"),
], ids=["five-stage", "five-stage-resblock2", "resblock2"])
def test_other_configs_report_the_restated_arithmetic(model):
    dims = dims_for(**model)
    back, fwd, reach1 = extents(dims)
    assert reported(dims) == (back, fwd, reach1)
    assert 1 <= reach1 <= fwd          # (something behind stage 0 is always cut)


def stage_frames(lengths, T, back, fwd, reach1):
    lengths = np.asarray(lengths, dtype=np.int64)
    glen0 = np.minimum(T, lengths + back + 1 + fwd)
    eligible = lengths + back + fwd <= T
    glen1 = np.where(eligible, np.minimum(glen0, lengths + back + reach1), glen0)
    return int(eligible.sum()), int(glen0.sum()), int(glen1.sum())


@pytest.mark.parametrize("name,expect", [("C3", (52, 28902, 28278)), ("C2", (9, 7516, 7408))])
def test_frame_counts_of_the_benchmark_workloads(name, expect):
    from vispeech_amd.synth import WORKLOADS, synth_batch
    fl = synth_batch(**WORKLOADS[name])["frame_lengths"]
    assert stage_frames(fl, int(fl.max()), *extents(ModelDims())) == expect
