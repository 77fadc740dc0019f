"""ResBlock2 (reference modules.py:245-249, without the mask) through the stand-alone operator vsp_cl_resblock2:
mode 0 (one g16_conv launch per convolution, in_act + res) and mode 1 (the fused g16_rb2 launch) return identical bits
on every shape the fused kernel covers, and both are within the stage gate of a torch fp64 ResBlock2."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-5          # relative to max|ref|: the gate of tests/test_cl_ops.py
F16_TOL = 5e-3      # terms = 1 (VSP_GENERATOR=f16): plain f16 operands, one MFMA per product


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vispeech_amd import _lib
    return _lib.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def host_ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data_as(C.c_void_p) for a in arrs])


def torch_resblock2(x, ws, bs, dils, k):
    y = torch.from_numpy(x).double().transpose(1, 2)
    for c, d in enumerate(dils):
        t = F.leaky_relu(y, 0.1)
        y = F.conv1d(t, torch.from_numpy(ws[c]).double(), torch.from_numpy(bs[c]).double(), dilation=d,
                     padding=d * (k - 1) // 2) + y
    return y.transpose(1, 2).numpy()


def case(c, k, dils, b, t, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    x = r.standard_normal((b, t, c)).astype(np.float32)
    ws = [(r.standard_normal((c, c, k)) / np.sqrt(c * k)).astype(np.float32) for _ in range(2)]
    bs = [r.standard_normal(c).astype(np.float32) * 0.1 for _ in range(2)]
    return x, ws, bs


def run(lib, x, ws, bs, dils, k, mode, terms=3):
    b, t, c = x.shape
    xd = torch.from_numpy(x).cuda()
    out = torch.full((b, t, c), float("nan"), device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.vsp_cl_resblock2(stream, b, t, c, k, (C.c_int * 2)(*dils), P(xd), host_ptrs(ws), host_ptrs(bs), mode, terms,
                              P(out))
    assert rc == 0, (mode, rc)
    return out.cpu().numpy()


@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("k", [3, 5, 7, 11])
@pytest.mark.parametrize("dils", [(1, 3), (1, 2), (2, 6), (3, 5)])
def test_fused_equals_per_convolution_bit_for_bit(lib, c, k, dils):
    for b, t in ((1, 1), (3, 7), (1, 255), (3, 256), (1, 257), (3, 2000)):
        x, ws, bs = case(c, k, dils, b, t, c + 10 * k + 100 * dils[1] + t)
        o0 = run(lib, x, ws, bs, dils, k, 0)
        o1 = run(lib, x, ws, bs, dils, k, 1)
        assert np.array_equal(o0.view(np.uint32), o1.view(np.uint32)), (b, t)
        ref = torch_resblock2(x, ws, bs, dils, k)
        assert rel_err(o0, ref) <= TOL and rel_err(o1, ref) <= TOL, (b, t)


@pytest.mark.parametrize("c,k,dils", [(128, 3, (1, 3)), (128, 11, (1, 3)), (256, 7, (1, 3)), (256, 5, (2, 6))])
def test_per_convolution_form_at_128_and_256_channels(lib, c, k, dils):
    for b, t in ((1, 1), (3, 257), (1, 1000)):
        x, ws, bs = case(c, k, dils, b, t, c + k + t)
        assert rel_err(run(lib, x, ws, bs, dils, k, 0), torch_resblock2(x, ws, bs, dils, k)) <= TOL, (b, t)


@pytest.mark.parametrize("c,k,dils", [(32, 11, (1, 3)), (64, 7, (2, 6)), (32, 3, (1, 3))])
def test_reduced_precision_terms_one(lib, c, k, dils):
    x, ws, bs = case(c, k, dils, 2, 700, 7 * c + k)
    ref = torch_resblock2(x, ws, bs, dils, k)
    o0 = run(lib, x, ws, bs, dils, k, 0, terms=1)
    o1 = run(lib, x, ws, bs, dils, k, 1, terms=1)
    assert np.array_equal(o0.view(np.uint32), o1.view(np.uint32))
    assert rel_err(o1, ref) <= F16_TOL
    assert rel_err(run(lib, x, ws, bs, dils, k, 1), ref) <= TOL       # (and the split form is the accurate one)


def test_refusals(lib):
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x48, o48 = torch.zeros(1, 8, 48, device="cuda"), torch.zeros(1, 8, 48, device="cuda")
    w48 = np.zeros((48, 48, 3), dtype=np.float32)
    b48 = np.zeros(48, dtype=np.float32)
    d13 = (C.c_int * 2)(1, 3)
    for mode in (0, 1):                                                                          # channels % 32
        assert lib.vsp_cl_resblock2(stream, 1, 8, 48, 3, d13, P(x48), host_ptrs([w48, w48]), host_ptrs([b48, b48]), mode, 3, P(o48)) == -7
    x, o = torch.zeros(1, 8, 32, device="cuda"), torch.zeros(1, 8, 32, device="cuda")
    w = np.zeros((32, 32, 11), dtype=np.float32)
    b = np.zeros(32, dtype=np.float32)
    d_far = (C.c_int * 2)(1, 7)                                                                  # (K - 1) d = 70 > 64
    for mode in (0, 1):
        assert lib.vsp_cl_resblock2(stream, 1, 8, 32, 11, d_far, P(x), host_ptrs([w, w]), host_ptrs([b, b]), mode, 3, P(o)) == -7
    # one dilation (the second one absent, 0): refused, never read past
    d_one = (C.c_int * 2)(1, 0)
    assert lib.vsp_cl_resblock2(stream, 1, 8, 32, 11, d_one, P(x), host_ptrs([w, w]), host_ptrs([b, b]), 1, 3, P(o)) in (-1, -7)
    assert lib.vsp_cl_resblock2(stream, 1, 8, 32, 11, d13, P(x), host_ptrs([w, w]), host_ptrs([b, b]), 1, 3, P(x)) == -1   # in place
    assert lib.vsp_cl_resblock2(stream, 1, 8, 32, 11, d13, P(x), host_ptrs([w, w]), host_ptrs([b, b]), 2, 3, P(o)) == -1   # mode
    assert lib.vsp_cl_resblock2(stream, 1, 8, 32, 11, d13, P(x), host_ptrs([w, w]), host_ptrs([b, b]), 1, 2, P(o)) == -1   # terms
    w128 = np.zeros((128, 128, 3), dtype=np.float32)
    b128 = np.zeros(128, dtype=np.float32)
    x128, o128 = torch.zeros(1, 8, 128, device="cuda"), torch.zeros(1, 8, 128, device="cuda")
    assert lib.vsp_cl_resblock2(stream, 1, 8, 128, 3, d13, P(x128), host_ptrs([w128, w128]), host_ptrs([b128, b128]), 1, 3,
                                P(o128)) == -7                                                  # fused: 32 / 64 channels
    assert lib.vsp_cl_resblock2(stream, 1, 0, 32, 11, d13, P(x), host_ptrs([w, w]), host_ptrs([b, b]), 1, 3, P(o)) == 0    # empty
