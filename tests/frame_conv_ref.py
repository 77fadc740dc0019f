"""Shared by tests/test_conv_form_host.py and tests/test_frame_conv_epilogue.py: the epilogues the frame-rate layers fuse
into their convolutions (api_frame.hip) as descriptors of vsp_conv1d_ex, the kernel form a launch reports as a short
name, and the fp64 reference of the whole epilogue.

A case is a plain dict of descriptor fields plus the layout of its tensors:
  cond      None | "aligned" (cond_bs = 8 h, pointer 2 h rows into a larger array, as wn_layer()) | "odd" (pointer one
            float further, cond_bs odd: the kernels' general rather than their lean path)
  res       None | "sep" (a tensor of its own) | "out" (res == out, in place)
  out_view  "window" (rows [8, 8 + rows) of a [B][rows + 16][T + 4] tensor) | "upper" (the upper half of a
            [B][2 rows][T] tensor, o_bs = 2 rows T: the flow's x1)
  x_pad     row stride of x = T + x_pad
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from vispeech_amd import _lib

H = 192
TOL = 1e-5            # relative to max|ref|: the project's stage gate (TOL / STAGE_TOL of the other operator tests)
ERR_ARG, ERR_UNSUPPORTED = -1, -7

DEFAULTS = dict(Cin=H, Cout=H, K=1, dil=1, act=0, cond=None, res=None, mask_in=0, in_act=0, in_slope=0.0, mask_pre=0, alpha=1.0,
                acc_prev=0, div=1.0, mask_post=0, split_row=0, acc_prev2=0, mask_post2=0, split_f16=1, cols=0, ln=0,
                out_view="window", x_pad=0)


def case(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


# ---- the epilogues of the model (api_frame.hip), by tag
def E1(cond="aligned"):           # WN in_layer + cond_layer(g) under the gate
    return case(Cout=2 * H, K=5, act=2, cond=cond)


def E2(acc_prev2=1):              # WN res_skip: rows [0, h) update H in place, rows [h, 2 h) accumulate the skip sum
    # (cond, alpha, div, mask_pre act on the first destination only: a leak into out2 would exceed the tolerance)
    return case(Cout=2 * H, split_row=H, res="out", mask_post=1, acc_prev2=acc_prev2, mask_pre=1, alpha=-1.0, div=3.0, cond="aligned")


def E2_model(acc_prev2=1):        # ... with exactly the model's options (the column-tile kernel takes no cond / div)
    return case(Cout=2 * H, split_row=H, res="out", mask_post=1, acc_prev2=acc_prev2)


def E3(acc_prev=1):               # the last WN layer's skip rows
    return case(mask_post=1, acc_prev=acc_prev)


def E4(alpha=-1.0):               # flow post: x1 = (x1 -/+ m) * mask on the upper half of z
    return case(Cout=96, mask_pre=1, alpha=alpha, res="out", out_view="upper", mask_post=1)


def E5():                         # proj of enc_p / enc_q / frame prior: m and logs in one launch
    return case(Cout=2 * H, split_row=H, mask_post=1, mask_post2=1, cond="aligned", alpha=-1.0, div=3.0, mask_pre=1, res="sep")


def E5_model():
    return case(Cout=2 * H, split_row=H, mask_post=1, mask_post2=1)


def E6(ln=0):                     # FFN conv_2 (+ the LayerNorm behind it)
    return case(Cin=768, K=3, mask_in=1, mask_pre=1, res="sep", ln=ln)


def E7(ln):                       # conv_o + residual + LayerNorm
    return case(res="out", ln=ln, cols=1 if ln == 1 else 0)


def E8(split_f16=1):              # the f32 generator's last ResBlock convolution
    return case(Cin=64, Cout=64, K=3, acc_prev=1, div=3.0, split_f16=split_f16)


def E9(cout, split_row, k):       # splits inside a 64-row block / a partial last tile in the second destination
    return case(Cout=cout, split_row=split_row, K=k, acc_prev2=1, mask_post2=1, mask_post=1, res="sep")


def E10(cout):                    # the three kernels of launch_layernorm: C == 192, C < 192, C > 192
    return case(Cout=cout, res="sep", ln=2)


def SMALL():                      # the throughput kernel's 32-row tiles
    return case(Cout=2, mask_pre=1, alpha=-1.0, res="sep")


# ---- the form a launch reports, as a short name
def form_name(f):
    k = f.kernel
    if k == _lib.CONV_FORM_TILE:
        shape = f"{f.mt}{f.nt}{f.wm}{f.wn}"
        if not f.f16s:
            return "f32_" + shape
        return "tile" + shape + ("p" if f.prune else "" if f.ring else "_noring")
    return {_lib.CONV_FORM_NONE: "none", _lib.CONV_FORM_COLS: "cols", _lib.CONV_FORM_COLS_LN: "cols_ln", _lib.CONV_FORM_GEMV: "gemv",
            _lib.CONV_FORM_SPLITK: "splitk", _lib.CONV_FORM_FRAME_SHORT: "frame_short", _lib.CONV_FORM_FRAME: "frame"}[k]


def rows_of(c):
    """(rows of out, rows of out2)"""
    if c["act"] == 2:
        return c["Cout"] // 2, 0
    if c["split_row"]:
        return c["split_row"], c["Cout"] - c["split_row"]
    return c["Cout"], 0


def gate_rows(cout):
    """kernel row r of a gated convolution holds the reference's row gate_rows(cout)[r] (include/vispeech_hip.h)"""
    r = np.arange(cout)
    return (r // 32 % 2) * (cout // 2) + (r // 64) * 32 + r % 32


def base_desc(c, B, T):
    d = _lib.VspConv1dDesc()
    d.B, d.T, d.Cin, d.Cout, d.K, d.dilation = B, T, c["Cin"], c["Cout"], c["K"], c["dil"]
    for k in ("mask_in", "in_act", "in_slope", "act", "mask_pre", "alpha", "acc_prev", "div", "mask_post", "split_row", "acc_prev2",
              "mask_post2", "split_f16", "cols", "ln"):
        setattr(d, k, c[k])
    return d


def plan(c, B, T, x_addr=0x10000):
    """(rc, form name) of a plan-only call: the strides and pointer alignments of the case, addresses nobody dereferences"""
    d = base_desc(c, B, T)
    rows, rows2 = rows_of(c)
    d.plan_only = 1
    d.x, d.x_cs = x_addr, T + c["x_pad"]
    d.out = 0x20000
    if c["out_view"] == "upper":
        d.o_bs = 2 * rows * T
    else:
        d.o_cs, d.o_bs = T + 4, (rows + 16) * (T + 4)
    if c["res"]:
        d.res, d.r_bs, d.r_cs = (d.out, d.o_bs, d.o_cs) if c["res"] == "out" else (0x30000, 0, 0)
    if rows2:
        d.out2, d.o2_cs, d.o2_bs = 0x40000, T + 4, (rows2 + 16) * (T + 4)
    if c["cond"]:
        d.cond, d.cond_bs = (0x50000, 8 * H) if c["cond"] == "aligned" else (0x50004, 8 * H + 1)
    masks = c["mask_in"] or c["mask_pre"] or c["mask_post"] or c["mask_post2"]
    d.lengths = 0x60000 if masks else None
    d.w = d.bias = 0x70000
    if c["ln"]:
        d.ln_gamma = d.ln_beta = 0x70000
    form = _lib.VspConvForm()
    rc = _lib.lib().vsp_conv1d_ex(None, C.byref(d), C.byref(form))
    return rc, form_name(form)


# ---- inputs: every tensor of utterance b is drawn on its own, column by column, so that the first columns of utterance 0
# of a case are the same data at every (B, T)
def _draw(seed, tag, b, rows, T):
    r = np.random.Generator(np.random.PCG64([seed, tag, b]))
    return r.standard_normal((T, rows), dtype=np.float32).T


def make_inputs(c, B, T, seed):
    rows, rows2 = rows_of(c)
    r = np.random.Generator(np.random.PCG64([seed, 99]))
    inp = {
        "w": (r.standard_normal((c["Cout"], c["Cin"], c["K"])) / np.sqrt(c["Cin"] * c["K"])).astype(np.float32),
        "bias": r.standard_normal(c["Cout"]).astype(np.float32),
        "gamma": r.standard_normal(c["Cout"]).astype(np.float32),
        "beta": r.standard_normal(c["Cout"]).astype(np.float32),
        "x": np.stack([_draw(seed, 0, b, c["Cin"], T) for b in range(B)]),
        "out_prev": np.stack([_draw(seed, 1, b, rows, T) for b in range(B)]),
        "lens": np.asarray([max(1, T - 3 * i - (i % 2)) for i in range(B)], dtype=np.int64),
    }
    if rows2:
        inp["out2_prev"] = np.stack([_draw(seed, 2, b, rows2, T) for b in range(B)])
    if c["res"] == "sep":
        inp["res"] = np.stack([_draw(seed, 3, b, rows, T) for b in range(B)])
    if c["cond"]:
        inp["cond"] = np.stack([_draw(seed, 4, b, c["Cout"], 1)[:, 0] for b in range(B)])      # reference row order
    return inp


def reference(c, inp, B, T):
    """The whole epilogue in torch fp64, in the order the kernels document:
    conv + bias -> [rows >= split_row: + out2_prev, mask_post2, store to out2] -> + cond -> relu / gate -> mask_pre -> * alpha
    -> + res -> + out_prev -> / div -> mask_post; ln: LayerNorm over channels (eps 1e-5) of that + res."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    mask = (torch.arange(T)[None, :] < torch.from_numpy(inp["lens"])[:, None]).double()[:, None, :]
    x = t(inp["x"])
    if c["mask_in"]:
        x = x * mask
    if c["in_act"]:
        x = F.leaky_relu(x, c["in_slope"])
    y = F.conv1d(x, t(inp["w"]), t(inp["bias"]), dilation=c["dil"], padding=c["dil"] * (c["K"] - 1) // 2)
    y2 = None
    if c["split_row"]:
        y, y2 = y[:, :c["split_row"]], y[:, c["split_row"]:]
        if c["acc_prev2"]:
            y2 = y2 + t(inp["out2_prev"])
        if c["mask_post2"]:
            y2 = y2 * mask
    if c["cond"]:
        y = y + t(inp["cond"])[:, :y.shape[1], None]
    if c["act"] == 1:
        y = torch.relu(y)
    elif c["act"] == 2:
        h = c["Cout"] // 2
        y = torch.tanh(y[:, :h]) * torch.sigmoid(y[:, h:])
    if c["mask_pre"]:
        y = y * mask
    y = y * c["alpha"]
    res = None
    if c["res"]:
        res = t(inp["out_prev"] if c["res"] == "out" else inp["res"])
    if res is not None and not c["ln"]:
        y = y + res
    if c["acc_prev"]:
        y = y + t(inp["out_prev"])
    y = y / c["div"]
    if c["mask_post"]:
        y = y * mask
    if c["ln"]:
        v = y + res if res is not None else y
        mean = v.mean(dim=1, keepdim=True)
        var = ((v - mean) ** 2).mean(dim=1, keepdim=True)
        y = (v - mean) / torch.sqrt(var + 1e-5) * t(inp["gamma"])[None, :, None] + t(inp["beta"])[None, :, None]
    return y.numpy(), None if y2 is None else y2.numpy()


def with_(c, **kw):
    c = dict(c)
    c.update(kw)
    return c


# ---- (id, case, B, T, the form the case is written for | the error code it must get).  The arithmetic, under launch_conv's
# thresholds (conv_mfma.hip conv_form): rb = ceil(M / 64) row blocks; b32 = B ceil(T / 32) rb, b128 = B ceil(T / 128) rb;
#   channel-split   b32 <= 512 (T <= 96: <= 8 x 512), Cin >= 64, K in {1, 3, 5}, 16-byte aligned rows
#   latency         b32 > 512 and b128 <= 256 (T <= 96: 2 b128 <= 256, reachable only where the channel-split kernel
#                   declines: Cin <= 32)
#   throughput      b128 > 256, or K = 7, or rows that are not 16-byte aligned (then the un-pruned instantiation);
#                   T <= 96: <2,1,1,2>; M <= 32: <1,1,1,2>, T >= 1024 <1,4,1,4>; M % 128 == 0 or M >= 256, T >= 1024:
#                   <2,2,2,2>; else T >= 1024: <2,2,1,4>, T < 1024: <2,1,1,4>
def _form_cases():
    out = []

    def add(tag, c, B, T, want):
        out.append((f"{tag}-{B}x{T}-{want}", c, B, T, want))

    # column-tile (cols = 1): any grid; 1, 2 and 3 column tiles per utterance, one of them partial
    for B, T in ((1, 4), (2, 68), (5, 132)):
        add("E2a0", with_(E2_model(0), cols=1), B, T, "cols")
        add("E2a1", with_(E2_model(1), cols=1), B, T, "cols")
        add("E3a1", with_(E3(1), cols=1), B, T, "cols")
        add("E4m", with_(E4(-1.0), cols=1), B, T, "cols")
        add("E4p", with_(E4(1.0), cols=1), B, T, "cols")
        add("E5", with_(E5_model(), cols=1), B, T, "cols")
        add("E9-160/96", with_(E9(160, 96, 1), cols=1), B, T, ERR_UNSUPPORTED)      # split_row % 192 != 0
        add("E9-200/128", with_(E9(200, 128, 1), cols=1), B, T, ERR_UNSUPPORTED)
        add("E7ln1", E7(1), B, T, "cols_ln")
    # channel-split: (2, 68): b32 = 2 * 3 * rb <= 72; (1, 132): 5 rb <= 60
    for B, T in ((2, 68), (1, 132)):
        for tag, c in (("E1", E1()), ("E1odd", E1("odd")), ("E2a0", E2(0)), ("E2a1", E2(1)), ("E3a0", E3(0)), ("E3a1", E3(1)),
                       ("E4m", E4(-1.0)), ("E4p", E4(1.0)), ("E5", E5()), ("E6", E6()), ("E6ln2", E6(2)), ("E7ln2", E7(2)), ("E8", E8()),
                       ("E9-160/96k1", E9(160, 96, 1)), ("E9-160/96k3", E9(160, 96, 3)), ("E9-200/128k1", E9(200, 128, 1)),
                       ("E9-200/128k3", E9(200, 128, 3)), ("E10-192", E10(192)), ("E10-96", E10(96)), ("E10-100", E10(100)),
                       ("E10-256", E10(256))):
            add(tag, c, B, T, "splitk")
    # latency, short: Cin = 32 is one chunk (the channel-split kernel declines); 2 b128 = 2 * 2 * 3 = 12 <= 256
    short = dict(Cin=32, Cout=H, K=3)
    add("E3short", with_(E3(1), **short), 2, 60, "frame_short")
    add("E6short", with_(E6(), **short), 2, 60, "frame_short")
    add("E6ln2short", with_(E6(2), **short), 2, 60, "frame_short")
    # latency.  M = 384 (rb 6), (8, 332): b32 = 8 * 11 * 6 = 528 > 512, b128 = 8 * 3 * 6 = 144
    for tag, c in (("E1", E1()), ("E1odd", E1("odd")), ("E2a1", E2(1)), ("E5", E5())):
        add(tag, c, 8, 332, "frame")
    # M = 192, 160 (rb 3), (4, 1400): b32 = 4 * 44 * 3 = 528, b128 = 4 * 11 * 3 = 132; M = 200, 256 (rb 4): 704, 176
    for tag, c in (("E3a1", E3(1)), ("E6", E6()), ("E6ln2", E6(2)), ("E7ln2", E7(2)), ("E9-160/96k1", E9(160, 96, 1)),
                   ("E9-200/128k3", E9(200, 128, 3)), ("E10-256", E10(256))):
        add(tag, c, 4, 1400, "frame")
    # M = 96 (rb 2), (8, 1028): b32 = 8 * 33 * 2 = 528, b128 = 8 * 9 * 2 = 144  ((16, 1400) has b128 = 352: throughput)
    add("E4m", E4(-1.0), 8, 1028, "frame")
    # M = 64 (rb 1), (16, 1028): b32 = 16 * 33 = 528, b128 = 16 * 9 = 144
    add("E8", E8(), 16, 1028, "frame")
    # throughput 64-row, pruned <2,1,1,4>: T < 1024.  M = 384, (16, 332): b128 = 16 * 3 * 6 = 288 > 256
    for tag, c in (("E1", E1()), ("E1odd", E1("odd")), ("E2a1", E2(1)), ("E5", E5())):
        add(tag, c, 16, 332, "tile2114p")
    # M = 192, 160, (16, 772): b128 = 16 * 7 * 3 = 336; M = 200: 448
    for tag, c in (("E3a1", E3(1)), ("E6", E6()), ("E7ln2", E7(2)), ("E9-160/96k3", E9(160, 96, 3)), ("E9-200/128k1", E9(200, 128, 1))):
        add(tag, c, 16, 772, "tile2114p")
    # M = 96, 100 (rb 2), (17, 1020): b128 = 17 * 8 * 2 = 272; M = 64, (33, 1020): 33 * 8 = 264
    add("E4p", E4(1.0), 17, 1020, "tile2114p")
    add("E10-100", E10(100), 17, 1020, "tile2114p")
    add("E8", E8(), 33, 1020, "tile2114p")
    # throughput <2,2,1,4>: T >= 1024, M % 128 != 0 and M < 256.  M = 192, 160, (11, 1028): b128 = 11 * 9 * 3 = 297; M = 200: 396
    for tag, c in (("E3a1", E3(1)), ("E6", E6()), ("E7ln2", E7(2)), ("E9-160/96k3", E9(160, 96, 3)), ("E9-200/128k1", E9(200, 128, 1))):
        add(tag, c, 11, 1028, "tile2214")
    add("E3k7", with_(E3(1), K=7), 1, 1028, "tile2214")                 # K = 7: the throughput kernel at every size
    add("E4m", E4(-1.0), 16, 1028, "tile2214")                          # M = 96: b128 = 16 * 9 * 2 = 288
    add("E10-96", E10(96), 16, 1028, "tile2214")
    add("E8", E8(), 29, 1028, "tile2214")                               # M = 64: b128 = 29 * 9 = 261
    # throughput wide <2,2,2,2>, pruned: T >= 1024, M = 384, (5, 1028): b128 = 5 * 9 * 6 = 270; M = 256, (8, 1028): 8 * 9 * 4 = 288
    for tag, c in (("E1", E1()), ("E2a1", E2(1)), ("E5", E5())):
        add(tag, c, 5, 1028, "tile2222p")
    add("E10-256", E10(256), 8, 1028, "tile2222p")
    # throughput short <2,1,1,2>: T <= 96.  K = 7 at any size; K = 1 only past the channel-split kernel's 8 x 512 blocks:
    # M = 384, (683, 4): b32 = 683 * 1 * 6 = 4098 > 4096  ((22, 60) has b32 = 22 * 2 * 6 = 264: channel-split)
    add("E3k7", with_(E3(1), K=7), 2, 60, "tile2112")
    add("E2a1", E2(1), 683, 4, "tile2112")
    add("E2a1", E2(1), 22, 60, "splitk")
    # ... and the other epilogues there, each at its first B with B rb > 4096 (one 32-column tile per utterance):
    # rb 6: 683; rb 3 (M = 192, 160): 1366; rb 4 (M = 200): 1025; rb 2 (M = 96, 100): 2049; rb 1 (M = 64): 4097
    for tag, c, B in (("E1", E1(), 683), ("E1odd", E1("odd"), 683), ("E5", E5(), 683), ("E3a1", E3(1), 1366), ("E6", E6(), 1366),
                      ("E7ln2", E7(2), 1366), ("E9-160/96k3", E9(160, 96, 3), 1366), ("E9-200/128k1", E9(200, 128, 1), 1025),
                      ("E4m", E4(-1.0), 2049), ("E10-100", E10(100), 2049), ("E8", E8(), 4097)):
        add(tag, c, B, 4, "tile2112")
    # throughput, not pruned: rows of T + 1 floats leave the vector staging at every grid size
    for tag, c in (("E1", E1()), ("E2a1", E2(1)), ("E3a1", E3(1)), ("E4m", E4(-1.0)), ("E5", E5()), ("E6", E6()), ("E7ln2", E7(2)),
                   ("E8", E8()), ("E9-160/96k1", E9(160, 96, 1)), ("E9-200/128k3", E9(200, 128, 3)), ("E10-100", E10(100))):
        add(tag + "-xpad", with_(c, x_pad=1), 2, 132, "tile2114")
    add("E2a1-xpad", with_(E2(1), x_pad=1), 1, 1028, "tile2222")
    add("E3a1-xpad", with_(E3(1), x_pad=1), 1, 1028, "tile2214")
    # throughput small: M = 2 <= 32
    add("SMALL", SMALL(), 2, 60, "tile1112")
    add("SMALL", SMALL(), 1, 1028, "tile1414")
    # f32: M = 384 -> <2,2,2,2>; M = 96, 64 -> <2,1,1,4>, T >= 1024 <2,4,1,4>
    for B, T in ((2, 132), (1, 1028)):
        add("E2a1", with_(E2(1), split_f16=0), B, T, "f32_2222")
        add("E4m", with_(E4(-1.0), split_f16=0), B, T, "f32_2114" if T < 1024 else "f32_2414")
        add("E8", E8(0), B, T, "f32_2114" if T < 1024 else "f32_2414")
    return out


FORM_CASES = _form_cases()
