"""The 16-channel kernel family g16_c16 (gen16_c16.hip: the last stage of a five-stage generator) through the
stand-alone operators: vsp_cl_conv1d at Cin = Cout = 16, vsp_cl_resblock (modes 0 / 1 / 2) and vsp_cl_resblock2
(modes 0 / 1) at C = 16, against torch fp64 and, between the modes, bit for bit.

A block of the kernel owns 512 columns and stores R = 512 - 2 H of them, H = the sum over the launch's convolutions of
(K - 1) d / 2 (kernels.h G16_C16_BT): every shape list below adds R - 1, R, R + 1 and 2 R + 1 for the launches that case
makes, next to the fixed lengths around the other kernels' 256-column tiles."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-5          # relative to max|ref|: the gate of tests/test_cl_ops.py
F16_TOL = 5e-3      # terms = 1: plain f16 operands (the gate of tests/test_resblock2_ops.py)
BT = 512            # columns per block (kernels.h G16_C16_BT)
FIXED_T = (1, 7, 255, 256, 257, 2000)
C16 = 16


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from vispeech_amd import _lib
    return _lib.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def H(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data_as(C.c_void_p) for a in arrs])


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def stored_columns(k, dils):
    """R of one launch that runs convolutions of kernel k at these dilations back to back."""
    return BT - 2 * sum((k - 1) // 2 * d for d in dils)


def lengths(*rs):
    out = list(FIXED_T)
    for r in rs:
        out += [r - 1, r, r + 1, 2 * r + 1]
    return sorted(set(out))


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ one convolution
def run_conv(lib, x, w, bias, k, d, slope, res, terms=3, c_in=C16, c_out=C16):
    b, t, _ = x.shape
    xd = torch.from_numpy(x).cuda()
    rd = None if res is None else torch.from_numpy(res).cuda()
    out = torch.full((b, t, c_out), float("nan"), device="cuda")
    rc = lib.vsp_cl_conv1d(stream(), b, t, c_in, c_out, k, d, P(xd), H(w), H(bias), slope, P(rd), terms, P(out))
    assert rc == 0, rc
    return out.cpu().numpy()


def torch_conv(x, w, bias, k, d, slope, res):
    xt = torch.from_numpy(x).double().transpose(1, 2)
    if slope != 1.0:
        xt = F.leaky_relu(xt, slope)
    ref = F.conv1d(xt, torch.from_numpy(w).double(), None if bias is None else torch.from_numpy(bias).double(), dilation=d,
                   padding=d * (k - 1) // 2).transpose(1, 2)
    if res is not None:
        ref = ref + torch.from_numpy(res).double()
    return ref.numpy()


@pytest.mark.parametrize("k", [1, 3, 7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_conv1d_matches_torch_fp64(lib, k, d):
    b = 2
    for t in lengths(stored_columns(k, (d,))):
        r = np.random.Generator(np.random.PCG64(1000 * k + 100 * d + t))
        x = r.standard_normal((b, t, C16)).astype(np.float32)
        w = (r.standard_normal((C16, C16, k)) / np.sqrt(C16 * k)).astype(np.float32)
        bias = r.standard_normal(C16).astype(np.float32)
        res = r.standard_normal((b, t, C16)).astype(np.float32)
        for slope in (0.1, 1.0):
            for use_res in (True, False):
                for use_bias in (True, False):
                    got = run_conv(lib, x, w, bias if use_bias else None, k, d, slope, res if use_res else None)
                    ref = torch_conv(x, w, bias if use_bias else None, k, d, slope, res if use_res else None)
                    e = rel_err(got, ref)
                    assert e <= TOL, (t, slope, use_res, use_bias, e)


# ------------------------------------------------------------------------------------------------ ResBlock1
def rb1_case(k, n_pairs, b, t, seed, scale=1.0):
    r = np.random.Generator(np.random.PCG64(seed))
    x = (r.standard_normal((b, t, C16)) * scale).astype(np.float32)
    ws = [(r.standard_normal((C16, C16, k)) / np.sqrt(C16 * k)).astype(np.float32) for _ in range(2 * n_pairs)]
    bs = [r.standard_normal(C16).astype(np.float32) * 0.1 for _ in range(2 * n_pairs)]
    return x, ws, bs


def torch_resblock(x, ws, bs, dils, k):
    y = torch.from_numpy(x).double().transpose(1, 2)
    for p, d in enumerate(dils):
        t = F.leaky_relu(y, 0.1)
        t = F.conv1d(t, torch.from_numpy(ws[2 * p]).double(), torch.from_numpy(bs[2 * p]).double(), dilation=d,
                     padding=d * (k - 1) // 2)
        t = F.leaky_relu(t, 0.1)
        t = F.conv1d(t, torch.from_numpy(ws[2 * p + 1]).double(), torch.from_numpy(bs[2 * p + 1]).double(),
                     padding=(k - 1) // 2)
        y = t + y
    return y.transpose(1, 2).numpy()


def run_rb1(lib, x, ws, bs, dils, k, mode, terms=3):
    b, t, c = x.shape
    xd = torch.from_numpy(x).cuda()
    out = torch.full((b, t, c), float("nan"), device="cuda")
    rc = lib.vsp_cl_resblock(stream(), b, t, c, k, len(dils), (C.c_int * len(dils))(*dils), P(xd), host_ptrs(ws),
                             host_ptrs(bs), mode, terms, P(out))
    assert rc == 0, (mode, rc)
    return out.cpu().numpy()


@pytest.mark.parametrize("k", [3, 7, 11])
def test_resblock1_three_forms_agree_bit_for_bit_and_match_fp64(lib, k):
    dils = (1, 3, 5)
    steps = [d for p in dils for d in (p, 1)]
    # the whole block (mode 2), the widest pair (mode 1), the widest single convolution (mode 0)
    ts = lengths(stored_columns(k, steps), stored_columns(k, (5, 1)), stored_columns(k, (5,)))
    assert k != 11 or stored_columns(k, steps) == 392            # (the accumulated halo of K = 11 is 60 per side)
    for t in ts:
        x, ws, bs = rb1_case(k, 3, 2, t, 10 * k + t)
        o = [run_rb1(lib, x, ws, bs, dils, k, mode) for mode in (0, 1, 2)]
        assert same_bits(o[0], o[1]) and same_bits(o[0], o[2]), t
        e = rel_err(o[2], torch_resblock(x, ws, bs, dils, k))
        assert e <= TOL, (t, e)


# ------------------------------------------------------------------------------------------------ ResBlock2
def torch_resblock2(x, ws, bs, dils, k):
    y = torch.from_numpy(x).double().transpose(1, 2)
    for c, d in enumerate(dils):
        t = F.leaky_relu(y, 0.1)
        y = F.conv1d(t, torch.from_numpy(ws[c]).double(), torch.from_numpy(bs[c]).double(), dilation=d,
                     padding=d * (k - 1) // 2) + y
    return y.transpose(1, 2).numpy()


def run_rb2(lib, x, ws, bs, dils, k, mode, terms=3):
    b, t, c = x.shape
    xd = torch.from_numpy(x).cuda()
    out = torch.full((b, t, c), float("nan"), device="cuda")
    rc = lib.vsp_cl_resblock2(stream(), b, t, c, k, (C.c_int * 2)(*dils), P(xd), host_ptrs(ws), host_ptrs(bs), mode, terms,
                              P(out))
    assert rc == 0, (mode, rc)
    return out.cpu().numpy()


@pytest.mark.parametrize("k", [3, 7, 11])
def test_resblock2_two_forms_agree_bit_for_bit_and_match_fp64(lib, k):
    dils = (1, 3)
    for t in lengths(stored_columns(k, dils), stored_columns(k, (3,))):
        x, ws, bs = rb1_case(k, 1, 2, t, 20 * k + t)
        o0 = run_rb2(lib, x, ws, bs, dils, k, 0)
        o1 = run_rb2(lib, x, ws, bs, dils, k, 1)
        assert same_bits(o0, o1), t
        e = rel_err(o1, torch_resblock2(x, ws, bs, dils, k))
        assert e <= TOL, (t, e)


# ------------------------------------------------------------------------------------------------ precision
@pytest.mark.parametrize("k", [3, 11])
def test_reduced_precision_terms_one(lib, k):
    dils = (1, 3, 5)
    x, ws, bs = rb1_case(k, 3, 2, 700, 7 + k)
    ref = torch_resblock(x, ws, bs, dils, k)
    o = [run_rb1(lib, x, ws, bs, dils, k, mode, terms=1) for mode in (0, 1, 2)]
    assert same_bits(o[0], o[1]) and same_bits(o[0], o[2])
    assert rel_err(o[2], ref) <= F16_TOL
    assert rel_err(o[2], ref) > TOL                                      # (one product is NOT the accurate form)
    assert rel_err(run_rb1(lib, x, ws, bs, dils, k, 2), ref) <= TOL      # ... the split form on the same data is
    x2, ws2, bs2 = rb1_case(k, 1, 2, 700, 8 + k)
    ref2 = torch_resblock2(x2, ws2, bs2, (1, 3), k)
    assert same_bits(run_rb2(lib, x2, ws2, bs2, (1, 3), k, 0, terms=1), run_rb2(lib, x2, ws2, bs2, (1, 3), k, 1, terms=1))
    assert rel_err(run_rb2(lib, x2, ws2, bs2, (1, 3), k, 1, terms=1), ref2) <= F16_TOL
    assert rel_err(run_rb2(lib, x2, ws2, bs2, (1, 3), k, 1), ref2) <= TOL


def test_inputs_of_one_thousandth_keep_the_gate(lib):
    """Activations of ~1e-3 have lo parts of ~5e-7: f16 SUBNORMALS, which the matrix core keeps (g16_common.h)."""
    for k in (3, 11):
        x, ws, bs = rb1_case(k, 3, 2, 700, 31 + k, scale=1e-3)
        assert rel_err(run_rb1(lib, x, ws, bs, (1, 3, 5), k, 2), torch_resblock(x, ws, bs, (1, 3, 5), k)) <= TOL
        assert rel_err(run_rb2(lib, x, ws[:2], bs[:2], (1, 3), k, 1), torch_resblock2(x, ws[:2], bs[:2], (1, 3), k)) <= TOL
        got = run_conv(lib, x, ws[0], bs[0], k, 3, 0.1, None)
        assert rel_err(got, torch_conv(x, ws[0], bs[0], k, 3, 0.1, None)) <= TOL


def test_small_amplitude_activations_stay_within_the_documented_bound(lib):
    """tests/test_cl_ops.py's absolute bound at 16 channels: every activation at ~1e-5, no bias, no residual:
    |err| <= 2^-24 sum|w| + 1e-5 max|ref|."""
    k, t = 7, 600
    r = np.random.Generator(np.random.PCG64(3))
    x = (r.standard_normal((1, t, C16)) * 1e-5).astype(np.float32)
    w = (r.standard_normal((C16, C16, k)) / np.sqrt(C16 * k)).astype(np.float32)
    got = run_conv(lib, x, w, None, k, 1, 1.0, None)
    ref = torch_conv(x, w, None, k, 1, 1.0, None)
    bound = 2.0 ** -24 * float(np.abs(w).sum(axis=(1, 2)).max()) + 1e-5 * float(np.abs(ref).max())
    assert float(np.abs(got - ref).max()) <= bound


def test_out_of_range_activations_are_loud(lib):
    """An activation beyond the f16 range splits to inf (vsp_split_pair): the result is non-finite, never a saturated
    number -- what the generator's sticky flag rests on."""
    k, t = 7, 600
    x, ws, bs = rb1_case(k, 3, 1, t, 5)
    x[:] = 1e6
    assert not np.isfinite(run_conv(lib, x, ws[0], bs[0], k, 1, 0.1, None)).any()
    assert not np.isfinite(run_rb1(lib, x, ws, bs, (1, 3, 5), k, 2)).any()
    assert not np.isfinite(run_rb2(lib, x, ws[:2], bs[:2], (1, 3), k, 1)).any()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(lib):
    s = stream()
    x = torch.zeros(1, 8, 64, device="cuda")
    o = torch.zeros(1, 8, 64, device="cuda")
    w = np.zeros(64 * 64 * 12, dtype=np.float32)
    b = np.zeros(64, dtype=np.float32)
    conv = lambda cin, cout, k, d: lib.vsp_cl_conv1d(s, 1, 8, cin, cout, k, d, P(x), H(w), H(b), 0.1, None, 3, P(o))
    assert conv(16, 16, 3, 1) == 0
    assert conv(16, 32, 3, 1) == -7 and conv(32, 16, 3, 1) == -7       # mixed 16 / 32: no kernel
    assert conv(48, 48, 3, 1) == -7 and conv(16, 48, 3, 1) == -7
    assert conv(16, 16, 4, 1) == -7                                    # even K
    assert conv(16, 16, 11, 7) == -7 and conv(16, 16, 3, 33) == -7     # (K - 1) d > 64
    assert conv(16, 16, 3, 32) == 0 and conv(16, 16, 65, 1) == 0       # ... and = 64
    ws, bs = [w] * 6, [b] * 6
    d135, d17, d13 = (C.c_int * 3)(1, 3, 5), (C.c_int * 3)(1, 7, 1), (C.c_int * 2)(1, 3)
    rb1 = lambda c, k, d, mode: lib.vsp_cl_resblock(s, 1, 8, c, k, 3, d, P(x), host_ptrs(ws), host_ptrs(bs), mode, 3, P(o))
    rb2 = lambda c, k, d, mode: lib.vsp_cl_resblock2(s, 1, 8, c, k, d, P(x), host_ptrs(ws), host_ptrs(bs), mode, 3, P(o))
    for mode in (0, 1, 2):
        assert rb1(16, 11, d135, mode) == 0
        assert rb1(48, 3, d135, mode) == -7 and rb1(16, 4, d135, mode) == -7 and rb1(16, 11, d17, mode) == -7
    for mode in (0, 1):
        assert rb2(16, 11, d13, mode) == 0
        assert rb2(48, 3, d13, mode) == -7 and rb2(16, 4, d13, mode) == -7
        assert rb2(16, 11, (C.c_int * 2)(1, 7), mode) == -7
    assert lib.vsp_cl_resblock(s, 1, 8, 16, 3, 3, d135, P(x), host_ptrs(ws), host_ptrs(bs), 2, 3, P(x)) == -1   # in place
    assert lib.vsp_cl_resblock(s, 1, 0, 16, 3, 3, d135, P(x), host_ptrs(ws), host_ptrs(bs), 2, 3, P(o)) == 0    # empty
