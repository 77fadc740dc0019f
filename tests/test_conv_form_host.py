"""Which kernel a frame-rate convolution launch takes (conv_mfma.hip conv_form, the decision tree of launch_conv), checked
without a GPU through plan-only calls of vsp_conv1d_ex: the shapes tests/test_frame_conv_epilogue.py runs report the form
they were written for, every grid-size threshold flips where the code says, what the latency kernels cannot take goes to
the throughput kernel, and refusals come back as error codes.  A threshold that moves fails here, not silently."""
import ctypes as C

import pytest

import frame_conv_ref as R
from frame_conv_ref import ERR_ARG, ERR_UNSUPPORTED, H, case, plan, with_
from vispeech_amd import _lib


@pytest.mark.parametrize("cid,c,B,T,want", R.FORM_CASES, ids=[x[0] for x in R.FORM_CASES])
def test_shape_table_reports_the_form_it_names(cid, c, B, T, want):
    rc, form = plan(c, B, T)
    if isinstance(want, int):
        assert rc == want, (rc, form)
    else:
        assert rc == 0 and form == want, (rc, form)


def tiles_T(n, width):
    """a T (a multiple of 4, not of the tile) with ceil(T / width) == n"""
    return width * (n - 1) + 4


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("M", [192, 384, 768])
def test_thresholds_flip_where_the_code_says(M, K):
    """Today's thresholds, both sides of each, for the model's three widths: rb = ceil(M / 64) row blocks;
    n = B * (column tiles) is the largest with n rb <= limit on one side and n + 1 on the other."""
    rb = (M + 63) // 64
    c = case(Cin=H, Cout=M, K=K, mask_post=1, res="sep")
    wide_p = "tile2222p" if M % 128 == 0 else "tile2214"
    # 512 blocks of 32 columns (T > 96): channel-split | latency  (one long utterance: b128 = ceil(n / 4) rb <= 256 here)
    n = 512 // rb
    assert (n + 1) * rb > 512 >= n * rb and -(-(n + 1) // 4) * rb <= 256
    assert plan(c, 1, tiles_T(n, 32)) == (0, "splitk"), n
    assert plan(c, 1, tiles_T(n + 1, 32)) == (0, "frame"), n + 1
    # 8 x 512 blocks of 32 columns at T <= 96: channel-split | throughput short (2 b128 > 256 there).  One tile per
    # utterance (T = 4), and three (T = 96: 3 (n // 3 + 1) rb = 4104 at every one of the three widths)
    n = 4096 // rb
    assert (n + 1) * rb > 4096 >= n * rb and 3 * (n // 3 + 1) * rb > 4096 >= 3 * (n // 3) * rb
    assert plan(c, n, 4) == (0, "splitk"), n
    assert plan(c, n + 1, 4) == (0, "tile2112"), n + 1
    assert plan(c, n // 3, 96) == (0, "splitk"), n // 3
    assert plan(c, n // 3 + 1, 96) == (0, "tile2112"), n // 3 + 1
    # 256 blocks of 128 columns (T = 100: one of them and four of 32 per utterance, b32 = 4 n rb > 512): latency | throughput
    n = 256 // rb
    assert (n + 1) * rb > 256 >= n * rb and 4 * n * rb > 512
    assert plan(c, n, 100) == (0, "frame"), n
    assert plan(c, n + 1, 100) == (0, "tile2114p"), n + 1
    # ... and at T >= 1024 (9 tiles of 128, 33 of 32 per utterance): the wide / <2,2,1,4> tiles behind it
    n = 256 // (9 * rb)
    assert 9 * (n + 1) * rb > 256 >= 9 * n * rb and 33 * n * rb > 512
    assert plan(c, n, 1028) == (0, "frame"), n
    assert plan(c, n + 1, 1028) == (0, wide_p), n + 1
    # Nq >= 1024 for the wide tiles, on a grid of the throughput kernel (b128 = 16 * 8 * rb > 256)
    assert plan(c, 16, 1020) == (0, "tile2114p")
    assert plan(c, 16, 1024) == (0, wide_p)


@pytest.mark.parametrize("K", [1, 3, 5])
def test_short_latency_threshold_flips_where_the_code_says(K):
    """T <= 96 with one input chunk (Cin <= 32: the channel-split kernel declines): the latency kernel's <2,1,1,2> form up to
    2 b128 <= 256, the throughput kernel's behind it.  M = 192: rb = 3, 2 * 42 * 3 = 252, 2 * 43 * 3 = 258."""
    c = case(Cin=32, Cout=H, K=K, mask_post=1)
    for T in (4, 60, 96):
        assert plan(c, 42, T) == (0, "frame_short")
        assert plan(c, 43, T) == (0, "tile2112")
    assert plan(c, 1, 100) == (0, "frame")                       # T > 96: the <2,1,1,4> form
    assert plan(with_(c, Cin=64), 42, 60) == (0, "splitk")       # two chunks: the channel-split kernel again


def test_what_the_latency_forms_cannot_take_goes_to_the_throughput_kernel():
    c = case(Cin=H, Cout=H, K=3, mask_post=1)                    # (2, 132): b32 = 2 * 5 * 3 = 30 -- channel-split otherwise
    assert plan(c, 2, 132) == (0, "splitk")
    assert plan(with_(c, K=7), 2, 132) == (0, "tile2114p")       # no K = 7 instantiation
    assert plan(with_(c, K=3, dil=4), 2, 132) == (0, "tile2114p")    # (K - 1) dil + 6 = 14 > 12: the window's halo
    assert plan(with_(c, K=5, dil=2), 2, 132) == (0, "tile2114p")
    assert plan(with_(c, K=5, dil=1), 2, 132) == (0, "splitk")       # 4 + 6 = 10
    assert plan(with_(c, K=3, dil=3), 2, 132) == (0, "splitk")       # 6 + 6 = 12: the last one in
    # rows that are not 16-byte aligned, a leaky-relu slope the max form does not cover: the UN-pruned instantiation
    assert plan(with_(c, x_pad=1), 2, 132) == (0, "tile2114")
    assert plan(c, 2, 132, x_addr=0x10004) == (0, "tile2114")
    assert plan(with_(c, in_act=1, in_slope=1.5), 2, 132) == (0, "tile2114")
    assert plan(with_(c, in_act=1, in_slope=-0.1), 2, 132) == (0, "tile2114")
    assert plan(with_(c, in_act=1, in_slope=0.1), 2, 132) == (0, "splitk")
    assert plan(with_(c, in_act=0, in_slope=1.5), 2, 132) == (0, "splitk")     # (the slope counts only with in_act)
    assert plan(with_(c, Cout=2 * H, x_pad=1), 1, 1028) == (0, "tile2222")
    assert plan(with_(c, Cout=2 * H, in_act=1, in_slope=1.5), 16, 1028) == (0, "tile2222")
    # 32 rows or fewer without the gate: the 32-row tiles at every grid size; one time step with a plain epilogue: the GEMV
    assert plan(with_(c, Cout=32), 2, 132) == (0, "tile1112")
    assert plan(with_(c, Cout=32), 2, 1024) == (0, "tile1414")
    assert plan(case(Cin=256, Cout=3072), 3, 1) == (0, "gemv")
    assert plan(case(Cin=256, Cout=3072, mask_post=1), 3, 1) == (0, "tile2112")        # (rows of one float: not 16-byte aligned)
    # the f32 path has the throughput kernel only
    assert plan(with_(c, split_f16=0), 2, 132) == (0, "f32_2114")
    assert plan(with_(c, split_f16=0, Cout=2), 2, 132) == (0, "f32_1112")
    assert plan(with_(c, split_f16=0), 2, 60) == (0, "f32_2112")


def test_the_form_carries_its_instantiation():
    d = R.base_desc(R.E1(), 2, 68)
    d.plan_only, d.x, d.out, d.w, d.cond, d.cond_bs = 1, 0x10000, 0x20000, 0x30000, 0x40000, 8 * H
    f = _lib.VspConvForm()
    assert _lib.lib().vsp_conv1d_ex(None, C.byref(d), C.byref(f)) == 0
    assert (f.kernel, f.k, f.gate) == (_lib.CONV_FORM_SPLITK, 5, 1)
    d.B, d.T = 8, 332
    assert _lib.lib().vsp_conv1d_ex(None, C.byref(d), C.byref(f)) == 0
    assert (f.kernel, f.k, f.mt, f.nt, f.wm, f.wn) == (_lib.CONV_FORM_FRAME, 5, 2, 1, 1, 4)
    d.B = 16
    assert _lib.lib().vsp_conv1d_ex(None, C.byref(d), C.byref(f)) == 0
    assert (f.kernel, f.mt, f.nt, f.wm, f.wn, f.f16s, f.ring, f.prune) == (_lib.CONV_FORM_TILE, 2, 1, 1, 4, 1, 1, 1)


def _raw(c, n_batch, n_cols, **fields):
    """plan-only with descriptor fields overridden after the case's own"""
    d = R.base_desc(c, n_batch, n_cols)
    rows, rows2 = R.rows_of(c)
    d.plan_only, d.x, d.out, d.w, d.bias = 1, 0x10000, 0x20000, 0x30000, 0x30000
    if rows2:
        d.out2 = 0x40000
    if c["mask_in"] or c["mask_pre"] or c["mask_post"] or c["mask_post2"]:
        d.lengths = 0x50000
    if c["res"]:
        d.res = 0x60000
    if c["ln"]:
        d.ln_gamma = d.ln_beta = 0x30000
    for k, v in fields.items():
        setattr(d, k, v)
    f = _lib.VspConvForm()
    return _lib.lib().vsp_conv1d_ex(None, C.byref(d), C.byref(f))


def test_refusals_come_back_as_error_codes():
    lib = _lib.lib()
    ok = case(mask_post=1, res="sep")
    assert _raw(ok, 2, 68) == 0
    f = _lib.VspConvForm()
    assert lib.vsp_conv1d_ex(None, None, C.byref(f)) == ERR_ARG
    d = R.base_desc(ok, 2, 68)
    d.plan_only, d.x, d.out, d.w, d.lengths = 1, 0x10000, 0x20000, 0x30000, 0x50000
    assert lib.vsp_conv1d_ex(None, C.byref(d), None) == ERR_ARG                      # a plan with nowhere to go
    # ---- VSP_ERR_ARG: null or contradictory pointers, options that exclude each other
    for fields in (dict(x=None), dict(out=None), dict(w=None), dict(lengths=None), dict(B=-1), dict(T=-1), dict(act=3), dict(act=-1),
                   dict(out2=0x40000), dict(acc_prev2=1), dict(mask_post2=1), dict(ln_gamma=0x30000), dict(ln=2), dict(ln=3),
                   dict(ln=2, ln_gamma=0x30000), dict(cols=2), dict(split_f16=2), dict(div=0.0), dict(cond_bs=-1),
                   dict(o_cs=67), dict(x_cs=64), dict(r_cs=10), dict(o_bs=H * 68 - 1), dict(split_row=H), dict(split_row=-32, out2=0x40000),
                   dict(split_row=2 * H, out2=0x40000)):
        assert _raw(ok, 2, 68, **fields) == ERR_ARG, fields
    assert _raw(R.E1(), 2, 68, res=0x60000) == ERR_ARG                               # the gate has no residual operand
    assert _raw(R.E1(), 2, 68, split_row=H, out2=0x40000) == ERR_ARG                 # ... and one destination
    assert _raw(R.E7(2), 2, 68, cols=0, ln=1) == ERR_ARG                             # the fused LayerNorm is the column-tile kernel's
    assert _raw(R.E2(), 2, 68, out2=None) == ERR_ARG
    # ---- VSP_ERR_UNSUPPORTED: what launch_conv / launch_conv_cols refuse
    for fields in (dict(K=2), dict(K=0), dict(Cin=0), dict(Cout=0), dict(dilation=0), dict(K=3, dilation=31), dict(K=63)):
        assert _raw(ok, 2, 68, **fields) == ERR_UNSUPPORTED, fields
    assert _raw(ok, 2, 68, K=3, dilation=30) == 0                                    # (K - 1) dil + 3 = 63 <= 64
    assert _raw(R.E1(), 2, 68, Cout=2 * H + 32) == ERR_UNSUPPORTED                   # the gate pairs 32-row tiles
    assert _raw(R.E1(), 2, 68, mask_pre=1, lengths=0x50000) == ERR_UNSUPPORTED       # the gate's epilogue: cond, mask_post
    assert _raw(R.E1(), 2, 68, alpha=-1.0) == ERR_UNSUPPORTED
    assert _raw(R.E2(), 2, 68, split_row=100) == ERR_UNSUPPORTED                     # a multiple of 32
    assert _raw(R.E2(), 2, 68, split_row=96) == 0
    assert _raw(R.E7(2), 2, 68, acc_prev=1) == ERR_UNSUPPORTED                       # LayerNorm of an accumulating destination
    for fields in (dict(K=3), dict(Cin=128), dict(Cout=32), dict(Cout=200), dict(Cout=640), dict(act=1), dict(in_act=1), dict(div=3.0),
                   dict(cond=0x70000), dict(split_f16=0), dict(split_row=96, out2=0x40000)):
        assert _raw(with_(ok, cols=1), 2, 68, **fields) == ERR_UNSUPPORTED, fields
    assert _raw(with_(ok, cols=1), 2, 68) == 0
    for fields in (dict(Cout=96), dict(Cin=96, Cout=96), dict(mask_pre=1), dict(mask_post=1), dict(alpha=-1.0)):
        assert _raw(with_(R.E7(1), mask_in=1), 2, 68, lengths=0x50000, **fields) == ERR_UNSUPPORTED, fields
    assert _raw(with_(R.E7(1), mask_in=1), 2, 68, lengths=0x50000) == 0
    # ---- the 32-bit byte offsets of the epilogues, per tensor: (rows * stride + T) * 4 < 2^31
    big = -(-((1 << 29) - 68) // H)                                                   # the first stride with H * stride + T >= 2^29
    for k in ("x_cs", "o_cs", "r_cs"):
        assert _raw(ok, 1, 68, **{k: big}) == ERR_UNSUPPORTED, k
        assert _raw(ok, 1, 68, **{k: big - 1}) == 0, k
    assert _raw(R.E5_model(), 1, 68, o2_cs=big) == ERR_UNSUPPORTED
    assert _raw(R.E5_model(), 1, 68, o2_cs=big - 1) == 0
    # B = 0 or T = 0: nothing to do
    assert _raw(ok, 0, 68) == 0 and _raw(ok, 2, 0) == 0
