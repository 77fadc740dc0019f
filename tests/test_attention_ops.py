"""Every attention kernel variant as a stand-alone operator (vsp_rel_attention, vsp_rel_attention_fused) against the
oracle's closed form of reference attentions.py:148-179 evaluated in FLOAT64 (oracle.vispeech_oracle.rel_attention is
dtype-generic), on ALL T columns of ALL rows -- the fully masked query rows included, which the reference computes as the
uniform average over the T keys (masked_fill(-1e4) over the whole row, then softmax).

(kernel, variant) names the code that runs:
  (0, 0)  attention.hip      attn_relpos_f32<DK, 4, true>    32-query blocks, four waves split the keys, merge through LDS
  (0, 1)  attention.hip      attn_relpos_f32<DK, 4, false>   128-query blocks, each wave walks every key tile
  (1, 0)  attention_f16s.hip attn_pack_f16s<DK> + attn_relpos_f16s<DK, 4, 1, 2>   64 queries, two key-tile streams merged
  (1, 1)  attention_f16s.hip attn_pack_f16s<DK> + attn_relpos_f16s<DK, 8, 1, 1>   128 queries, one stream
  variant -1 is the launcher's own rule (what the model runs): the 128-query form from 256 (kernel 0) / 512 (kernel 1)
  blocks of 128 queries, the small-grid form below.

Which family reaches what:
  a  test_variants_head_shapes_edges, test_windows: all four pairs at dk 96, 64 and 32 (one to four heads), time lengths
     around the 16 / 32 / 64 / 128 tile edges, T < 2 w + 1, an utterance of length 0 and 1 inside a batch, a far-from-band
     key tile that is only partly valid (3 x 257, lengths 100 and 0: the "tile is inside" shortcut must not take it),
     windows 0, 1, 4 and 7; variant -1 must return the bits of one of the forced forms.
  b  test_block_renumbering: kernel 1, both forms, with 6 (plain block order), 8, 9 and 10 (XCD-aware order, groups padded
     to 8 / 16 / 16) (utterance, head) groups and several query blocks per group; every row also alone as B = 1 (plain
     order) -- the bits must not depend on the numbering.
  c  test_automatic_rule_thresholds: 512 and 256 blocks (both kernels' thresholds from both sides), and dk 32 at 512.
  d  test_moving_maximum: keys that grow / shrink along time, so that the running maximum of the online softmax and the
     maxima of the key streams (kernel 1) / the four key-split waves (kernel 0) differ when they are merged.
  e  test_relative_terms_alone: band scores alone (k = 0), the relative-value term alone (v = 0), neither (emb = 0).
  f  test_fused_projection: attn_qkv_pack_f16s<96 / 64 / 32, 2> + both attention forms reading its packed images.
  g  test_refusals.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.vispeech_oracle import rel_attention

pytestmark = pytest.mark.gpu

TOL = 1e-5          # relative to max|ref| (SURVEY 8c stage gate, tests/test_cl_ops.py TOL, test_hip_parity.py STAGE_TOL)
# measured maxima on the MI355X over every case below (the fp32 oracle itself is 2.8e-7 .. 1.1e-6 from its fp64 self):
#   (0, 0) f32, key-split        ~1.1e-6  (a;   c 9.7e-7, d 1.0e-6, e 1.0e-6)
#   (0, 1) f32, 128 queries      ~2.8e-6  (a, dk 32, T = 1500;   c 1.2e-6, d 1.4e-6, e 1.2e-6)
#   (1, 0) split-f16, 64 x 2     ~1.5e-6  (c, 32 x 500;   a 7.7e-7, b 8.2e-7, d 1.0e-6, e 7.9e-7)
#   (1, 1) split-f16, 128        ~1.6e-6  (c, 32 x 500;   a 1.1e-6, b 9.0e-7, d 1.1e-6, e 8.3e-7)
#   fused projection, 0 and 1    ~6.7e-7  (f, H = 192, 2 x 65)
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]       # (kernel, variant)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vispeech_amd import _lib
    return _lib.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def Hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rng(*key):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(k) for k in key])))


def make_inputs(H, heads, window, B, T, lengths, tag=0):
    """Standard-normal q | k | v [B][3H][T]; asymmetric random tables ~ N(0, 1 / dk); seeded from the parameters."""
    dk = H // heads
    r = rng(H, heads, window, B, T, tag, *lengths)
    qkv = r.standard_normal((B, 3 * H, T)).astype(np.float32)
    ek = (r.standard_normal((2 * window + 1, dk)) / np.sqrt(dk)).astype(np.float32)
    ev = (r.standard_normal((2 * window + 1, dk)) / np.sqrt(dk)).astype(np.float32)
    return qkv, ek, ev


def reference(qkv, ek, ev, lengths, heads, window):
    """The oracle's closed form on float64 tensors, a few batch rows at a time (the [rows][heads][T][T] temporaries)."""
    B, H3, T = qkv.shape
    H = H3 // 3
    t = torch.from_numpy(qkv).double()
    ek64, ev64 = torch.from_numpy(ek).double()[None], torch.from_numpy(ev).double()[None]
    lens = torch.tensor([T] * B if lengths is None else list(lengths), dtype=torch.int64)
    mask = torch.arange(T)[None, :] < lens[:, None]
    rows = max(1, int(4e7 // max(heads * T * T, 1)))
    out = [rel_attention(t[b:b + rows, :H].contiguous(), t[b:b + rows, H:2 * H].contiguous(), t[b:b + rows, 2 * H:].contiguous(),
                         ek64, ev64, mask[b:b + rows], heads, window) for b in range(0, B, rows)]
    return torch.cat(out).numpy()


def lens_dev(lengths):
    return None if lengths is None else torch.tensor(list(lengths), dtype=torch.int64, device="cuda")


def run(lib, qkv_d, ek, ev, lengths, heads, window, kernel, variant):
    """vsp_rel_attention on a device q | k | v; the output starts as NaN: a column nobody writes fails the comparison."""
    B, H3, T = qkv_d.shape
    out = torch.full((B, H3 // 3, T), float("nan"), device="cuda")
    ld = lens_dev(lengths)
    rc = lib.vsp_rel_attention(stream(), B, T, H3 // 3, heads, window, P(qkv_d), Hp(ek), Hp(ev), P(ld), kernel, variant, P(out))
    assert rc == 0, (rc, kernel, variant)
    return out.cpu()


def check_pairs(lib, qkv, ek, ev, lengths, heads, window, what, pairs=PAIRS, auto=True):
    """Every (kernel, variant) of `pairs` against fp64 on all columns; variant -1 returns the bits of a forced form."""
    ref = reference(qkv, ek, ev, lengths, heads, window)
    qd = torch.from_numpy(qkv).cuda()
    got = {}
    for kernel, variant in pairs:
        got[kernel, variant] = o = run(lib, qd, ek, ev, lengths, heads, window, kernel, variant)
        e = rel_err(o.numpy(), ref)
        print(f"att_err kernel={kernel} variant={variant} {e:.3e} {what}")
        assert not torch.isnan(o).any(), (what, kernel, variant, "columns left unwritten")
        assert e <= TOL, (what, kernel, variant, e)
    if auto:
        for kernel in sorted({k for k, _ in pairs}):
            o = run(lib, qd, ek, ev, lengths, heads, window, kernel, -1)
            assert any(torch.equal(o, g) for (k, _), g in got.items() if k == kernel), (what, kernel, "automatic form")
    return got, ref


HEAD_SHAPES = [(192, 2), (96, 1), (128, 2), (192, 3), (64, 2), (128, 4)]        # dk 96, 96, 64, 64, 32, 32
EDGES = [(1, 1, (1,)), (2, 5, (5, 3)), (2, 16, (16, 15)), (2, 17, (17, 1)), (3, 33, (33, 32, 31)), (2, 64, (64, 63)),
         (2, 65, (65, 33)), (3, 129, (129, 128, 97)), (3, 257, (257, 100, 0)), (1, 1500, (1203,))]


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("B,T,lengths", EDGES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("H,heads", HEAD_SHAPES)
def test_variants_head_shapes_edges(lib, H, heads, B, T, lengths):
    qkv, ek, ev = make_inputs(H, heads, 4, B, T, lengths)
    check_pairs(lib, qkv, ek, ev, lengths, heads, 4, f"a H={H} heads={heads} B={B} T={T}")


@pytest.mark.parametrize("B,T,lengths", [(2, 5, (5, 3)), (2, 65, (65, 33)), (3, 257, (257, 100, 0))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("window", [0, 1, 7])
@pytest.mark.parametrize("H,heads", [(192, 2), (64, 2)])
def test_windows(lib, H, heads, window, B, T, lengths):
    qkv, ek, ev = make_inputs(H, heads, window, B, T, lengths)
    check_pairs(lib, qkv, ek, ev, lengths, heads, window, f"a H={H} window={window} T={T}")


# ------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("T", [130, 300])
@pytest.mark.parametrize("B,heads", [(3, 2), (4, 2), (3, 3), (5, 2)])      # 6, 8, 9, 10 (utterance, head) groups
def test_block_renumbering(lib, B, heads, T):
    """The XCD-aware block numbering of attn_relpos_f16s (from 8 groups; the group count padded to a multiple of eight)
    must not change what a group computes: every row of the batch has the bits of that utterance run alone."""
    H = 192
    lengths = tuple(max(1, T - 37 * b) for b in range(B))                  # ragged; different random data per row
    qkv, ek, ev = make_inputs(H, heads, 4, B, T, lengths, tag=1)
    got, _ = check_pairs(lib, qkv, ek, ev, lengths, heads, 4, f"b B={B} heads={heads} T={T}", pairs=[(1, 0), (1, 1)], auto=False)
    for variant in (0, 1):
        for b in range(B):
            alone = run(lib, torch.from_numpy(qkv[b:b + 1]).cuda(), ek, ev, lengths[b:b + 1], heads, 4, 1, variant)
            assert torch.equal(alone[0], got[1, variant][b]), (variant, b)


# ------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("H,heads,window,B,T,expect", [
    (192, 2, 4, 64, 500, {0: 1, 1: 1}),          # 4 * 2 * 64 = 512 blocks of 128 queries: the 128-query form for both
    (192, 2, 4, 32, 500, {0: 1, 1: 0}),          # 256: f32 takes the 128-query form (>= 256), split-f16 the 64-query form (< 512)
    (64, 2, 0, 32, 1000, {0: 1, 1: 1}),          # dk 32 at 8 * 2 * 32 = 512
])
def test_automatic_rule_thresholds(lib, H, heads, window, B, T, expect):
    lengths = tuple(T - (17 * b) % (T // 2) for b in range(B))
    qkv, ek, ev = make_inputs(H, heads, window, B, T, lengths, tag=2)
    got, _ = check_pairs(lib, qkv, ek, ev, lengths, heads, window, f"c H={H} B={B} T={T}")
    qd = torch.from_numpy(qkv).cuda()
    for kernel, variant in expect.items():
        o = run(lib, qd, ek, ev, lengths, heads, window, kernel, -1)
        assert torch.equal(o, got[kernel, variant]), (kernel, "the launcher's rule picks variant", variant)


# ------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("T", [300, 1500])
@pytest.mark.parametrize("ramp", ["up", "down"])
def test_moving_maximum(lib, ramp, T):
    """Keys * (1 + j / (T - 1)): the largest scores sit in the late key tiles, the running maximum keeps moving; keys *
    (1 - 0.5 j / (T - 1)): it stops moving early.  Either way the key-tile streams of a query group (split-f16) and the four
    key-split waves (f32, variant 0) arrive at their merge with different maxima."""
    H, heads, B = 192, 2, 2
    lengths = (T, T - T // 5)
    qkv, ek, ev = make_inputs(H, heads, 4, B, T, lengths, tag=3 + (ramp == "up"))
    j = np.arange(T, dtype=np.float64) / (T - 1)
    scale = 1.0 + j if ramp == "up" else 1.0 - 0.5 * j
    qkv[:, H:2 * H] = (qkv[:, H:2 * H] * scale).astype(np.float32)
    check_pairs(lib, qkv, ek, ev, lengths, heads, 4, f"d ramp={ramp} T={T}", auto=False)


# ------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("mode", ["band_scores_only", "relative_values_only", "no_relative_terms"])
@pytest.mark.parametrize("window", [4, 7])
@pytest.mark.parametrize("T", [5, 37, 300])
@pytest.mark.parametrize("H,heads", [(192, 2), (64, 2)])
def test_relative_terms_alone(lib, H, heads, T, window, mode):
    """k = 0: the scores are the band terms q . Ek[j - i + w] alone; v = 0: the output is the relative-value term
    sum P_ij Ev[j - i + w] alone; emb_k = emb_v = 0: plain masked softmax attention."""
    B, lengths = 2, (T, max(1, T - 3))
    qkv, ek, ev = make_inputs(H, heads, window, B, T, lengths, tag=5)
    if mode == "band_scores_only":
        qkv[:, H:2 * H] = 0
    elif mode == "relative_values_only":
        qkv[:, 2 * H:] = 0
    else:
        ek[:] = 0
        ev[:] = 0
    check_pairs(lib, qkv, ek, ev, lengths, heads, window, f"e {mode} H={H} T={T} window={window}", auto=False)


# ------------------------------------------------------------------------------------------------ f
FUSED = [(1, 1, (1,)), (2, 63, (63, 40)), (2, 64, (64, 0)), (3, 65, (65, 64, 7)), (2, 300, (300, 123)), (2, 65, None)]


@pytest.mark.parametrize("B,T,lengths", FUSED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("H", [192, 128, 64])
def test_fused_projection(lib, H, B, T, lengths):
    """attn_qkv_pack_f16s (conv_q | conv_k | conv_v of x * mask and the operand packing in one launch, the packing code a
    second time on an LDS tile) + the attention on its images, against F.conv1d in fp64 + the oracle."""
    heads, window = 2, 4
    r = rng(H, B, T, 6, *(lengths or (T,)))
    x = r.standard_normal((B, H, T)).astype(np.float32)
    w = (r.standard_normal((3 * H, H)) / np.sqrt(H)).astype(np.float32)
    bias = (0.5 * r.standard_normal(3 * H)).astype(np.float32)
    dk = H // heads
    ek = (r.standard_normal((2 * window + 1, dk)) / np.sqrt(dk)).astype(np.float32)
    ev = (r.standard_normal((2 * window + 1, dk)) / np.sqrt(dk)).astype(np.float32)
    lens = torch.tensor([T] * B if lengths is None else list(lengths))
    mask = (torch.arange(T)[None, :] < lens[:, None]).double()[:, None, :]
    qkv64 = F.conv1d(torch.from_numpy(x).double() * mask, torch.from_numpy(w).double()[:, :, None], torch.from_numpy(bias).double())
    m = mask[:, 0] > 0
    ref = rel_attention(qkv64[:, :H].contiguous(), qkv64[:, H:2 * H].contiguous(), qkv64[:, 2 * H:].contiguous(),
                        torch.from_numpy(ek).double()[None], torch.from_numpy(ev).double()[None], m, heads, window).numpy()
    xd, ld = torch.from_numpy(x).cuda(), lens_dev(lengths)
    for variant in (0, 1):
        out = torch.full((B, H, T), float("nan"), device="cuda")
        rc = lib.vsp_rel_attention_fused(stream(), B, T, H, heads, window, P(xd), Hp(w), Hp(bias), Hp(ek), Hp(ev), P(ld), variant, P(out))
        assert rc == 0, rc
        e = rel_err(out.cpu().numpy(), ref)
        print(f"att_err kernel=fused variant={variant} {e:.3e} f H={H} B={B} T={T}")
        assert not torch.isnan(out).any(), (variant, "columns left unwritten")
        assert e <= TOL, (variant, e)


# ------------------------------------------------------------------------------------------------ g
def test_refusals(lib):
    ARG, UNSUPPORTED = -1, -7
    st, T = stream(), 8
    r = rng(7)
    qkv = torch.from_numpy(r.standard_normal((2, 3 * 192, T)).astype(np.float32)).cuda()
    emb = r.standard_normal((17, 96)).astype(np.float32)
    bias = r.standard_normal(3 * 192).astype(np.float32)
    w = r.standard_normal((3 * 192, 192)).astype(np.float32)
    out = torch.full((2, 192, T), float("nan"), device="cuda")
    good, over, under = lens_dev((T, 3)), lens_dev((T + 1, 3)), lens_dev((T, -1))

    def att(B=2, T_=T, H=192, heads=2, window=4, q=qkv, ek=emb, ev=emb, ln=good, kernel=1, variant=-1, o=out):
        return lib.vsp_rel_attention(st, B, T_, H, heads, window, P(q), Hp(ek), Hp(ev), P(ln), kernel, variant, P(o))

    def fused(B=2, T_=T, H=192, heads=2, window=4, x=qkv, w_=w, b_=bias, ek=emb, ev=emb, ln=good, variant=-1, o=out):
        return lib.vsp_rel_attention_fused(st, B, T_, H, heads, window, P(x), Hp(w_), Hp(b_), Hp(ek), Hp(ev), P(ln), variant, P(o))

    for kernel in (0, 1):
        assert att(heads=4, kernel=kernel) == UNSUPPORTED           # dk = 48
        assert att(window=8, kernel=kernel) == UNSUPPORTED          # 2 w + 1 > 16
        assert att(window=-1, kernel=kernel) == UNSUPPORTED
        assert att(H=100, heads=3, kernel=kernel) == UNSUPPORTED    # H % n_heads
        assert att(q=None, kernel=kernel) == ARG
        assert att(o=None, kernel=kernel) == ARG
        assert att(ek=None, kernel=kernel) == ARG
        assert att(ev=None, kernel=kernel) == ARG
        assert att(variant=2, kernel=kernel) == ARG
        assert att(variant=-2, kernel=kernel) == ARG
        assert att(ln=over, kernel=kernel) == ARG
        assert att(ln=under, kernel=kernel) == ARG
        assert att(B=-1, kernel=kernel) == ARG
        assert att(T_=-1, kernel=kernel) == ARG
    assert att(kernel=2) == ARG
    assert att(kernel=-1) == ARG
    assert fused(H=128, heads=4) == UNSUPPORTED                     # the fused launch: two heads only
    assert fused(H=96, heads=1) == UNSUPPORTED                      # ... and H = 192 / 128 / 64
    assert fused(window=8) == UNSUPPORTED
    assert fused(x=None) == ARG
    assert fused(w_=None) == ARG
    assert fused(b_=None) == ARG
    assert fused(ek=None) == ARG
    assert fused(o=None) == ARG
    assert fused(variant=2) == ARG
    assert fused(ln=over) == ARG
    assert fused(ln=under) == ARG
    # nothing of the above wrote anything; neither do B = 0 and T = 0, which are VSP_OK
    for kernel in (0, 1):
        assert att(B=0, kernel=kernel) == 0
        assert att(T_=0, kernel=kernel) == 0
    assert fused(B=0) == 0
    assert fused(T_=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    # and the same arguments without a fault are accepted
    assert att(kernel=0) == 0 and att(kernel=1) == 0 and fused() == 0
    assert not torch.isnan(out).any()
