"""The generator's up-convolutions (HiFi-GAN's ups, reference models.py:253-256, 277-278: F.leaky_relu + ConvTranspose1d)
through the stand-alone C-ABI operators, against torch's fp64 conv_transpose1d on the same activated input:

- vsp_cl_conv_transpose1d packs the weights as the model packs dec.ups.* and dispatches through the generator's launcher,
  so each shape / grid below reaches the kernel the generator runs there: the streaming g16_ups<2,2,4,1> (64 -> 32
  channels, kernel 4, stride 2) and g16_ups<1,4,4,4> (128 -> 64, kernel 4, stride 4), and the polyphase g16_conv tile at
  128, 64 and 32 rows (picked from the grid size), TERMS 3 and TERMS 1;
- vsp_conv_transpose1d is the f32 generator's form (conv1d_f32_mfma's transposed epilogue), at any channel count.

Covered: tile edges in time, the rows the padding drops at both ends (n = stride q + r - p), every output row written,
small activations and small weights (the operand split of g16_ups is its own code), ragged extents (kernels.h ClConvArgs
glen: rows at and beyond an utterance's own extent read as zero and are never stored), repeatability and refusals."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-5          # relative to max|ref| (tests/test_cl_ops.py)
F16_TOL = 5e-3      # terms = 1: plain f16 operands (tests/test_resblock2_ops.py)

# (Cin, Cout, K, stride)
STAGE0, STAGE1 = (512, 256, 16, 8), (256, 128, 16, 8)      # configs/config.json stages 0, 1: polyphase g16_conv tile
UPS_S4, UPS_S2 = (128, 64, 4, 4), (64, 32, 4, 2)           # stages 2, 3: g16_ups<1,4,4,4>, g16_ups<2,2,4,1>
ALT_LAST = (64, 32, 8, 4)                                   # test_other_configs.py ALT's last stage: 2 taps per phase
SHAPES = [STAGE0, STAGE1, UPS_S4, UPS_S2, ALT_LAST,
          (128, 64, 4, 2), (64, 32, 4, 4),                  # next to the streaming shapes: the tile kernel
          (64, 64, 9, 3), (32, 32, 2, 2), (256, 128, 8, 8), (96, 48, 6, 2)]   # odd stride; k = s; 3 taps per phase
FRAMES = [1, 2, 15, 16, 17, 255, 256, 257, 1000]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vispeech_amd import _lib
    return _lib.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def H(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def data(shape, b, t, seed, x_scale=1.0, w_scale=None, b_scale=1.0):
    cin, cout, k, s = shape
    r = np.random.Generator(np.random.PCG64(seed))
    x = (r.standard_normal((b, t, cin)) * x_scale).astype(np.float32)
    w = r.standard_normal((cin, cout, k))
    w = (w * (w_scale if w_scale is not None else 1.0 / np.sqrt(cin * k / s))).astype(np.float32)
    bias = (r.standard_normal(cout) * b_scale).astype(np.float32)
    return x, w, bias


def ref_ct(x, w, bias, s, slope):
    """fp64 conv_transpose1d(leaky_relu(x)) on channels-last x [B][T][Cin] -> [B][T s][Cout]."""
    k = w.shape[2]
    xt = torch.from_numpy(x).double().transpose(1, 2)
    if slope != 1.0:
        xt = F.leaky_relu(xt, slope)
    y = F.conv_transpose1d(xt, torch.from_numpy(w).double(), None if bias is None else torch.from_numpy(bias).double(),
                           stride=s, padding=(k - s) // 2)
    return y.transpose(1, 2).numpy()


def run_cl(lib, shape, x, w, bias, slope=0.1, terms=3, lengths=None, out=None):
    cin, cout, k, s = shape
    b, t, _ = x.shape
    xd = torch.from_numpy(x).cuda()
    if out is None:
        out = torch.full((b, t * s, cout), float("nan"), device="cuda")
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
    rc = lib.vsp_cl_conv_transpose1d(stream(), b, t, cin, cout, k, s, P(xd), H(w), H(bias), slope, P(ld), terms, P(out))
    assert rc == 0, rc
    return out.cpu()


def err(got, ref, scale=None):
    got = np.asarray(got, dtype=np.float64)
    return float(np.abs(got - ref).max() / (scale if scale is not None else max(np.abs(ref).max(), 1e-30)))


def check_all_rows(got, ref, s, tol, what):
    assert not torch.isnan(got).any(), f"{what}: rows left unwritten"
    g = got.numpy()
    peak = max(float(np.abs(ref).max()), 1e-30)
    assert err(g, ref, peak) <= tol, what
    # the rows next to the ends are where the padding drops n = stride q + r - p < 0 and >= stride T
    assert err(g[:, :s], ref[:, :s], peak) <= tol, f"{what}: first {s} rows"
    assert err(g[:, -s:], ref[:, -s:], peak) <= tol, f"{what}: last {s} rows"


# ------------------------------------------------------------------------------------------------ vsp_cl_conv_transpose1d
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("t", FRAMES)
def test_cl_conv_transpose1d_matches_fp64(lib, shape, b, t):
    x, w, bias = data(shape, b, t, seed=sum(shape) * 1009 + t * 7 + b)
    for slope in (0.1, 1.0):
        check_all_rows(run_cl(lib, shape, x, w, bias, slope), ref_ct(x, w, bias, shape[3], slope), shape[3], TOL,
                       f"slope {slope}")


# grids that move the polyphase tile (gen16.hip launch_g16_conv: col_tiles = B ceil((T + 1) / 256); 128 rows when
# col_tiles rows / 128 >= 200, else 64 when col_tiles rows / 64 >= 200, else 32), and long g16_ups launches whose blocks
# hold several runs of 16 time tiles with a partial last run
GRIDS = [
    (STAGE0, 13, 200, "128-row tile"), (STAGE0, 3, 1000, "64-row tile"), (STAGE0, 1, 1000, "32-row tile"),
    (ALT_LAST, 40, 1279, "128-row tile"), (ALT_LAST, 25, 1000, "64-row tile"), (ALT_LAST, 1, 1000, "32-row tile"),
    (UPS_S2, 1, 2000, "g16_ups, partial last run"), (UPS_S2, 2, 4097, "g16_ups, one-tile last run"),
    (UPS_S4, 1, 2000, "g16_ups, partial last run"), (UPS_S4, 2, 4097, "g16_ups, one-tile last run"),
]


@pytest.mark.parametrize("shape,b,t,what", GRIDS, ids=[f"{'x'.join(map(str, g[0]))}-{g[1]}x{g[2]}" for g in GRIDS])
def test_cl_conv_transpose1d_tile_choices_and_long_runs(lib, shape, b, t, what):
    x, w, bias = data(shape, b, t, seed=t * 31 + b)
    check_all_rows(run_cl(lib, shape, x, w, bias, 0.1), ref_ct(x, w, bias, shape[3], 0.1), shape[3], TOL, what)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("b,t", [(2, 257), (1, 1000)])
def test_cl_conv_transpose1d_plain_f16_operands(lib, shape, b, t):
    """terms = 1 (VSP_GENERATOR=f16): the TERMS = 1 tile at every row tile; the terms = 3 result on the same data stays
    within fp32 accuracy."""
    x, w, bias = data(shape, b, t, seed=sum(shape) + t)
    ref = ref_ct(x, w, bias, shape[3], 0.1)
    check_all_rows(run_cl(lib, shape, x, w, bias, 0.1, terms=1), ref, shape[3], F16_TOL, "terms 1")
    check_all_rows(run_cl(lib, shape, x, w, bias, 0.1, terms=3), ref, shape[3], TOL, "terms 3")


AMP_SHAPES = [UPS_S2, UPS_S4, STAGE1]


@pytest.mark.parametrize("shape", AMP_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_cl_conv_transpose1d_small_amplitude_activations_stay_within_the_documented_bound(lib, shape):
    """Activations of ~1e-5: the split keeps x to within 2^-24 absolute there (g16_common.h), so
    |err| <= 2^-24 max_row sum|w| + 1e-5 max|ref| (test_cl_ops.py's bound), where a row is one (phase, channel)."""
    cin, cout, k, s = shape
    x, w, _ = data(shape, 2, 700, seed=5, x_scale=1e-5)
    bias = np.zeros(cout, dtype=np.float32)
    got = run_cl(lib, shape, x, w, bias, 1.0).numpy()
    ref = ref_ct(x, w, bias, s, 1.0)
    row_sum = np.abs(w.astype(np.float64)).reshape(cin, cout, k // s, s).sum(axis=(0, 2)).max()
    bound = 2.0 ** -24 * float(row_sum) + 1e-5 * float(np.abs(ref).max())
    assert float(np.abs(got - ref).max()) <= bound


@pytest.mark.parametrize("shape", AMP_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_cl_conv_transpose1d_small_weights_keep_fp32_accuracy(lib, shape):
    """Weights of ~1e-3 (packed * 2^8 so that their lo parts stay normal f16 numbers, kernels.h G16_WSCALE): 1e-6 of peak."""
    x, w, bias = data(shape, 2, 700, seed=6, w_scale=1e-3, b_scale=1e-2)
    got = run_cl(lib, shape, x, w, bias, 1.0).numpy()
    ref = ref_ct(x, w, bias, shape[3], 1.0)
    assert float(np.abs(got - ref).max()) <= 1e-6 * float(np.abs(ref).max())


RAGGED = [(UPS_S2, 257, "g16_ups"), (UPS_S4, 257, "g16_ups"), (STAGE1, 255, "32-row tile"), (STAGE1, 1300, "128-row tile")]


@pytest.mark.parametrize("shape,t,what", RAGGED, ids=[f"{'x'.join(map(str, g[0]))}-{g[1]}" for g in RAGGED])
def test_cl_conv_transpose1d_ragged_extents(lib, shape, t, what):
    """lengths[b]: utterance b's tensor ends after lengths[b] input rows.  Rows [0, len s) are the fp64 conv_transpose of
    x[b, :len] (zeros behind it), rows [len s, T s) are never written; all lengths = T is the uniform launch, bit for bit."""
    cin, cout, k, s = shape
    lengths = [0, 1, t - 1, t, t // 2]
    x, w, bias = data(shape, len(lengths), t, seed=t + cin)
    got = run_cl(lib, shape, x, w, bias, 0.1, lengths=lengths)
    refs = [ref_ct(x[i:i + 1, :n], w, bias, s, 0.1)[0] if n else None for i, n in enumerate(lengths)]
    peak = max(float(np.abs(r).max()) for r in refs if r is not None)
    for i, n in enumerate(lengths):
        g = got[i].numpy()
        assert not np.isnan(g[:n * s]).any(), (what, n)
        if n:
            assert err(g[:n * s], refs[i], peak) <= TOL, (what, n)
        assert np.isnan(g[n * s:]).all(), (what, n, "rows behind the utterance's end were written")
    full = run_cl(lib, shape, x, w, bias, 0.1, lengths=[t] * len(lengths))
    uniform = run_cl(lib, shape, x, w, bias, 0.1)
    assert torch.equal(full.view(torch.int32), uniform.view(torch.int32)), what


@pytest.mark.parametrize("shape,b,t", [(UPS_S2, 2, 1000), (UPS_S4, 2, 1000), (STAGE0, 3, 1000), (ALT_LAST, 1, 257)],
                         ids=["g16_ups-s2", "g16_ups-s4", "tile-64", "tile-32"])
def test_cl_conv_transpose1d_repeats_bit_for_bit(lib, shape, b, t):
    x, w, bias = data(shape, b, t, seed=11)
    a = run_cl(lib, shape, x, w, bias, 0.1)
    c = run_cl(lib, shape, x, w, bias, 0.1)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_cl_conv_transpose1d_refuses_what_it_cannot_do(lib):
    x = torch.zeros(1, 8, 64, device="cuda")
    out = torch.zeros(1, 8 * 8, 64, device="cuda")
    st = stream()

    def call(cin, cout, k, s, T=8, xp=x, op=out, w=True, terms=3, lengths=None, B=1):
        wh = np.zeros((cin, cout, k), dtype=np.float32)
        return lib.vsp_cl_conv_transpose1d(st, B, T, cin, cout, k, s, P(xp), H(wh) if w else None, None, 0.1,
                                           P(lengths), terms, P(op))

    assert call(64, 32, 4, 2) == 0
    assert call(64, 32, 5, 2) == -7             # K % stride
    assert call(64, 32, 6, 4) == -7             # K - stride odd
    assert call(48, 32, 4, 2) == -7             # Cin % 32
    assert call(64, 24, 4, 2) == -7             # Cout % 16
    assert call(64, 16, 1, 1) == -7             # stride Cout % 32 (no tile of 16 rows)
    assert call(64, 32, 2 * 66, 2) == -7        # halo: K / stride - 1 > 64
    assert call(512, 32, 4, 2, T=1 << 20) == -7  # an utterance's input beyond 2 GiB (refused before any launch)
    assert call(64, 32, 4, 2, xp=None) == -1
    assert call(64, 32, 4, 2, op=None) == -1
    assert call(64, 32, 4, 2, w=False) == -1
    assert call(64, 32, 4, 2, op=x) == -1       # in place
    assert call(64, 32, 4, 2, terms=2) == -1
    assert call(64, 32, 4, 2, lengths=torch.tensor([9], dtype=torch.int32, device="cuda")) == -1   # length > T
    assert call(64, 32, 4, 2, lengths=torch.tensor([-1], dtype=torch.int32, device="cuda")) == -1
    assert call(64, 32, 4, 2, B=0) == 0
    assert call(64, 32, 4, 2, T=0) == 0


# ------------------------------------------------------------------------------------------------ vsp_conv_transpose1d
F32_SHAPES = SHAPES + [(96, 48, 4, 4), (48, 24, 4, 2), (384, 192, 16, 8), (33, 24, 6, 2)]   # + the fallback's ragged counts


@pytest.mark.parametrize("shape", F32_SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("t", [1, 17, 257, 1000])
def test_conv_transpose1d_f32_matches_fp64(lib, shape, t):
    cin, cout, k, s = shape
    b = 2
    x, w, bias = data(shape, b, t, seed=sum(shape) * 13 + t)
    xc = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()        # channel-major [B][Cin][T]
    for slope in (0.1, 1.0):
        out = torch.full((b, cout, t * s), float("nan"), device="cuda")
        rc = lib.vsp_conv_transpose1d(stream(), b, t, cin, cout, k, s, P(xc), H(w), H(bias), slope, P(out))
        assert rc == 0, rc
        got = out.cpu().transpose(1, 2)
        check_all_rows(got, ref_ct(x, w, bias, s, slope), s, TOL, f"slope {slope}")


def test_conv_transpose1d_f32_refuses_what_it_cannot_do(lib):
    x = torch.zeros(1, 33, 8, device="cuda")
    out = torch.zeros(1, 24, 16, device="cuda")
    w = np.zeros((33, 24, 6), dtype=np.float32)
    st = stream()
    assert lib.vsp_conv_transpose1d(st, 1, 8, 33, 24, 6, 2, P(x), H(w), None, 0.1, P(out)) == 0
    assert lib.vsp_conv_transpose1d(st, 1, 8, 33, 24, 5, 2, P(x), H(w), None, 0.1, P(out)) == -7     # K % stride
    assert lib.vsp_conv_transpose1d(st, 1, 8, 33, 24, 6, 4, P(x), H(w), None, 0.1, P(out)) == -7     # K - stride odd
    assert lib.vsp_conv_transpose1d(st, 1, 8, 33, 24, 2 * 64, 2, P(x), H(w), None, 0.1, P(out)) == -7   # halo
    assert lib.vsp_conv_transpose1d(st, 1, 8, 33, 24, 6, 2, None, H(w), None, 0.1, P(out)) == -1
    assert lib.vsp_conv_transpose1d(st, 1, 8, 33, 24, 6, 2, P(x), None, None, 0.1, P(out)) == -1
    assert lib.vsp_conv_transpose1d(st, 1, 8, 33, 24, 6, 2, P(x), H(w), None, 0.1, P(x)) == -1       # in place
    assert lib.vsp_conv_transpose1d(st, 0, 8, 33, 24, 6, 2, P(x), H(w), None, 0.1, P(out)) == 0
