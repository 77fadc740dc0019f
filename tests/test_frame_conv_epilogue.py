"""The fused epilogues of the frame-rate convolutions on EVERY kernel form launch_conv can pick (conv_mfma.hip, conv_cols.hip),
through the stand-alone operator vsp_conv1d_ex, against the whole epilogue in torch fp64 (frame_conv_ref.reference).

The model reaches these epilogues (api_frame.hip: WN in_layer + cond under the gate, res_skip with two destinations, the
last layer's accumulated skip rows, the flow's in-place post on a channel-offset view, proj's m | logs, the FFN's masked
conv_2, conv_o + LayerNorm, the divided ResBlock sum) at whatever grid size a request happens to have; the pieces of
code that implement them (conv_epi_load / conv_epi_store in its hoisted and per-element forms, conv_tile_lean,
conv_gate_lean, conv_cols_kernel) promise identical results.  (The fifth, the per-element epilogue at the end of
conv1d_f32_mfma, runs for the transposed convolution only: tests/test_upsample_ops.py.)  Every case here names the form
it was written for (frame_conv_ref.FORM_CASES,
with the arithmetic) and asserts that the launch reported it, so a threshold that moves cannot take a case off its kernel
unnoticed (tests/test_conv_form_host.py says the same on a machine without a GPU).

Per case: max|out - ref| / max|ref| <= 1e-5 for out and for out2 separately (the project's stage gate; a plain fp32
evaluation of these formulas is 2e-7 .. 8e-7 from fp64); columns at and behind lengths[b] are exactly 0.0 wherever
mask_post / mask_post2 is set; every destination is a window of a larger tensor filled with a sentinel bit pattern, and
every element outside the window is bit-identical afterwards; out2 is compared against a reference that has no cond,
alpha, res, div or mask_pre in it while the launch sets them all.

Worst measured error against fp64 per form (MI355X, out and out2 together; each case prints its own):
  column-tile 3.0e-7, column-tile + LayerNorm 1.9e-7, channel-split 9.6e-7, latency short 1.4e-7, latency 2.2e-6,
  throughput <2,1,1,4> pruned 2.2e-6 / un-pruned 1.6e-6, <2,2,1,4> 6.1e-7, <2,2,2,2> pruned 2.4e-6 / un-pruned 2.1e-7,
  <2,1,1,2> 1.7e-6, <1,1,1,2> 1.8e-7, <1,4,1,4> 1.6e-7, f32 <2,1,1,4> 3.1e-7, <2,4,1,4> 3.1e-7, <2,2,2,2> 3.9e-7.
Everything above 1e-6 is E1, the gate: its pre-activation conv + bias + cond reaches |y| ~ 7, where fp32 values are 4.8e-7
apart, in front of tanh * sigmoid <= 1 (8e-7 .. 2.4e-6 on every form, growing with the number of elements looked at).  Without
E1 the worst figure of any form is 7.5e-7 (E6, 2304 products per element).  No case failed: no kernel was changed.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import frame_conv_ref as R
from frame_conv_ref import ERR_UNSUPPORTED, H, TOL

pytestmark = pytest.mark.gpu

SENTINEL = 0x4B4B4B4B            # as fp32: 13323083.0 -- finite, so a kernel that reads it shows in the comparison


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vispeech_amd import _lib
    return _lib.lib()


def sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


class Window:
    """rows [r0, r0 + rows) x columns [0, T) of a larger sentinel-filled device tensor [B][R][W]"""

    def __init__(self, B, rows, T, r0, R_, W, prev):
        self.full = sentinel((B, R_, W))
        self.r0, self.rows, self.T = r0, rows, T
        win = self.full[:, r0:r0 + rows, :T]
        if prev is None:
            win.fill_(float("nan"))                   # nobody reads it: an element nobody writes fails the comparison
        else:
            win.copy_(torch.from_numpy(np.ascontiguousarray(prev)))
        self.bs, self.cs = R_ * W, W
        self.ptr = self.full.data_ptr() + 4 * r0 * W

    def result(self):
        """the window, after checking that nothing outside it changed"""
        got = self.full.cpu()
        win = got[:, self.r0:self.r0 + self.rows, :self.T].clone()
        got[:, self.r0:self.r0 + self.rows, :self.T] = torch.tensor(SENTINEL, dtype=torch.int32).view(torch.float32)
        assert bool((got.view(torch.int32) == SENTINEL).all()), "an element outside the destination's window changed"
        return win.numpy()


def dest(c, B, rows, T, prev):
    if c["out_view"] == "upper":                       # the upper half of [B][2 rows][T]
        return Window(B, rows, T, rows, 2 * rows, T, prev)
    return Window(B, rows, T, 8, rows + 16, T + 4, prev)


def run_case(lib, c, B, T, seed):
    """-> (rc, form name, out window, out2 window | None, inputs)"""
    from vispeech_amd import _lib
    inp = R.make_inputs(c, B, T, seed)
    rows, rows2 = R.rows_of(c)
    d = R.base_desc(c, B, T)
    keep = []
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # x: rows of T + x_pad floats
    xw = Window(B, c["Cin"], T, 0, c["Cin"], T + c["x_pad"], inp["x"])
    d.x, d.x_cs, d.x_bs = xw.ptr, xw.cs, xw.bs
    reads_out = c["res"] == "out" or c["acc_prev"]
    ow = dest(c, B, rows, T, inp["out_prev"] if reads_out else None)
    d.out, d.o_cs, d.o_bs = ow.ptr, ow.cs, ow.bs
    if c["res"] == "out":
        d.res, d.r_cs, d.r_bs = ow.ptr, ow.cs, ow.bs
    elif c["res"] == "sep":                            # rows [1, rows + 1) of [B][rows + 2][T + 1]
        rw = Window(B, rows, T, 1, rows + 2, T + 1, inp["res"])
        d.res, d.r_cs, d.r_bs = rw.ptr, rw.cs, rw.bs
        keep.append(rw)
    o2w = None
    if rows2:
        o2w = Window(B, rows2, T, 8, rows2 + 16, T + 4, inp["out2_prev"] if c["acc_prev2"] else None)
        d.out2, d.o2_cs, d.o2_bs = o2w.ptr, o2w.cs, o2w.bs
    if c["cond"]:
        # kernel row order (the gate's interleaved tiles), inside a larger array as wn_layer() hands it over
        cond_bs, off = (8 * H, 2 * H) if c["cond"] == "aligned" else (8 * H + 1, 2 * H + 1)
        rows_k = R.gate_rows(c["Cout"]) if c["act"] == 2 else np.arange(c["Cout"])
        arr = sentinel((B * cond_bs + off + 8,))
        for b in range(B):
            arr[b * cond_bs + off:b * cond_bs + off + c["Cout"]] = dev(inp["cond"][b][rows_k])
        d.cond, d.cond_bs = arr.data_ptr() + 4 * off, cond_bs
        keep.append(arr)
    lens = dev(inp["lens"])
    if c["mask_in"] or c["mask_pre"] or c["mask_post"] or c["mask_post2"]:
        d.lengths = lens.data_ptr()
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    d.w, d.bias = hp(inp["w"]), hp(inp["bias"])
    if c["ln"]:
        d.ln_gamma, d.ln_beta = hp(inp["gamma"]), hp(inp["beta"])
    form = _lib.VspConvForm()
    rc = lib.vsp_conv1d_ex(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(d), C.byref(form))
    torch.cuda.synchronize()
    xw.result()                                        # (the input is read, never written)
    return rc, R.form_name(form), ow.result(), None if o2w is None else o2w.result(), inp


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def seed_of(cid):
    return zlib.crc32(cid.split("-")[0].encode())


_RESULTS = {}                    # case id -> (out, out2) of utterance 0: the cross-form test takes what the form cases left


@pytest.mark.parametrize("cid,c,B,T,want", R.FORM_CASES, ids=[x[0] for x in R.FORM_CASES])
def test_epilogue_matches_fp64_on_the_form_the_case_names(lib, cid, c, B, T, want):
    rc, form, out, out2, inp = run_case(lib, c, B, T, seed_of(cid))
    if isinstance(want, int):
        assert rc == want and np.isnan(out).all(), (rc, form)          # refused, nothing written
        return
    assert rc == 0 and form == want, (rc, form)
    ref, ref2 = R.reference(c, inp, B, T)
    behind = np.arange(T)[None, None, :] >= inp["lens"][:, None, None]
    errs = [rel_err(out, ref)]
    if c["mask_post"] and not c["ln"]:
        assert (out[np.broadcast_to(behind, out.shape)] == 0.0).all(), "out behind lengths[b]"
    if ref2 is not None:
        errs.append(rel_err(out2, ref2))
        if c["mask_post2"]:
            assert (out2[np.broadcast_to(behind, out2.shape)] == 0.0).all(), "out2 behind lengths[b]"
    print(f"FORM_ERR {form} {cid} " + " ".join(f"{e:.3e}" for e in errs))
    assert errs[0] <= TOL, ("out", errs)
    assert len(errs) == 1 or errs[1] <= TOL, ("out2", errs)
    _RESULTS[cid] = (out[0], None if out2 is None else out2[0])


def agree_pairwise(results):
    """utterance 0 of the same data through several forms, on the columns two runs share (K = 1: a column depends on its
    own input column only)"""
    ids = sorted(results)
    for i, a in enumerate(ids):
        for b in ids[i + 1:]:
            for ya, yb in zip(results[a], results[b]):
                n = min(ya.shape[-1], yb.shape[-1])
                assert rel_err(ya[:, :n], yb[:, :n]) <= TOL, (a, b)


@pytest.mark.parametrize("tag", ["E2a1", "E5"])
def test_same_utterance_agrees_across_forms(lib, tag):
    """E2 (res_skip) and E5 (proj) on the same x, weights and previous contents through every form that accepts them;
    utterance 0 is cut out of the larger batches.  Different forms sum in different orders (not bit-identical):
    they agree to the stage tolerance."""
    results = {}
    for cid, c, B, T, want in R.FORM_CASES:
        if cid.split("-")[0] != tag or isinstance(want, int) or c["cols"]:
            continue
        if cid not in _RESULTS:
            rc, form, out, out2, _ = run_case(lib, c, B, T, seed_of(cid))
            assert rc == 0 and form == want, (cid, rc, form)
            _RESULTS[cid] = (out[0], out2[0])
        results[cid] = _RESULTS[cid]
    assert len({cid.split("-")[-1] for cid in results}) >= 5, sorted(results)        # the forms, not the same one five times
    agree_pairwise(results)


@pytest.mark.parametrize("tag,c", [("E2", R.E2_model(1)), ("E5", R.E5_model())])
def test_same_utterance_agrees_between_the_column_tile_kernel_and_the_row_tiled_ones(lib, tag, c):
    """... with the model's own options (the column-tile kernel takes no cond / div): column-tile, channel-split, latency,
    throughput pruned and un-pruned."""
    results = {}
    for name, cc, B, T, want in (("cols-2x68", R.with_(c, cols=1), 2, 68, "cols"), ("cols-5x132", R.with_(c, cols=1), 5, 132, "cols"),
                                 ("splitk", c, 2, 68, "splitk"), ("frame", c, 8, 332, "frame"), ("tile2114p", c, 16, 332, "tile2114p"),
                                 ("tile2114", R.with_(c, x_pad=1), 2, 132, "tile2114")):
        rc, form, out, out2, _ = run_case(lib, cc, B, T, seed_of(tag + "model"))
        assert rc == 0 and form == want, (name, rc, form)
        results[name] = (out[0], out2[0])
    agree_pairwise(results)


def test_fused_and_two_launch_layernorm_agree(lib):
    """E7: conv_o + residual + LayerNorm in the column-tile launch (ln = 1) and as convolution + LayerNorm kernel (ln = 2),
    in place on the residual."""
    for B, T in ((1, 4), (2, 68), (5, 132)):
        outs = []
        for ln in (1, 2):
            rc, form, out, _, inp = run_case(lib, R.E7(ln), B, T, seed_of("E7"))
            assert rc == 0 and form == ("cols_ln" if ln == 1 else "splitk"), (ln, rc, form)
            outs.append(out)
        ref, _ = R.reference(R.E7(2), inp, B, T)
        assert rel_err(outs[0], ref) <= TOL and rel_err(outs[1], ref) <= TOL
        assert rel_err(outs[0], outs[1]) <= TOL


def test_a_length_outside_the_tensor_is_refused(lib):
    from vispeech_amd import _lib
    c = R.E3(0)
    inp = R.make_inputs(c, 2, 8, 1)
    x, out = torch.from_numpy(inp["x"]).cuda(), torch.zeros(2, H, 8, device="cuda")
    for bad in ([8, 9], [-1, 8]):
        lens = torch.tensor(bad, dtype=torch.int64, device="cuda")
        d = R.base_desc(c, 2, 8)
        d.x, d.out, d.lengths = x.data_ptr(), out.data_ptr(), lens.data_ptr()
        d.w = inp["w"].ctypes.data_as(C.c_void_p)
        rc = lib.vsp_conv1d_ex(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(d), C.byref(_lib.VspConvForm()))
        assert rc == R.ERR_ARG, bad
