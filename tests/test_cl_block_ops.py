"""The vocoder's fused ResBlock kernels with the launch inputs only the generator's schedule sets otherwise -- acc_prev
(out = result + out), div, the ragged batch glen / grate -- as stand-alone operators (vsp_cl_block_ex, vsp_cl_conv_post)
against torch fp64 on the CPU:  ref = (prev + block(x)) / div,  block = tests/test_cl_ops.py torch_resblock and its ResBlock2
analogue (cl_block_ref.block_f64).  One shape per kernel route (cl_block_ref.ROUTES; tests/test_cl_block_route_host.py checks
without a GPU that each shape reports the route it was written for), T = 2 R + 37 for a route whose tile stores R columns:
  (a) accumulate and divide on a uniform batch, every route against fp64 and bit for bit against mode 0;
  (b) ragged extents [1, pad, R - 1, R, R + 1, 2 R, 2 R + 1, T] with NaN behind every end: fp64 per row, nothing stored behind
      an end, the bits of a B = 1 call on the row alone, all lengths = T equal to lengths = NULL, and the grate = 8 form;
  (c) about 800 tiles over five utterances of very different tile counts on the three persistent kernels;
  (d) terms = 1;  (e) conv_post.

TOL is the gate tests/test_cl_ops.py holds these kernels to; the largest fp64 error measured on an MI355X per route is in
the table under the tolerances (run this file with -s to print it again).  Every bit-for-bit claim holds on every route."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cl_block_ref as R
from cl_block_ref import BY_ID, ERR_ARG

pytestmark = pytest.mark.gpu

TOL = 1e-5          # relative to max|ref| (SURVEY 8c stage gate), the gate of tests/test_cl_ops.py
F16_TOL = 5e-3      # terms = 1: plain f16 operands, the value of tests/test_resblock2_ops.py
POST_TOL = 1e-5     # conv_post, absolute (|tanh| <= 1): a 448-term fp32 chain plus tanhf

# Measured on an MI355X, largest error over a test's cases, relative to the batch's max|ref| (conv_post: absolute):
#   route                 (a) uniform   (b) ragged   (c) persistent   (d) terms 1
#   rw_k7                   3.0e-07      3.1e-07       2.1e-07
#   rw_k11                  2.5e-07      3.5e-07
#   pair_ring_32_k7         2.1e-07      2.4e-07                       2.1e-04
#   pair_64_k3              2.6e-07      2.6e-07
#   rw64                    2.0e-07      2.5e-07       2.1e-07
#   pp_k3                   2.8e-07      2.5e-07
#   pp_k7                   4.4e-07      4.3e-07
#   rc                      2.2e-07      2.2e-07       2.3e-07
#   chain_narrow_32_k3      1.7e-07      2.0e-07
#   chain_wide_32_k11       3.0e-07      3.4e-07
#   chain_64_k3             2.7e-07      2.4e-07                       2.8e-04
#   chain_128_k3            2.3e-07      2.6e-07
#   rb2_32                  2.1e-07      1.7e-07                       2.4e-04
#   rb2_64                  2.7e-07      3.1e-07
#   rb2_32_wide             2.9e-07      3.3e-07
#   c16_rb1                 1.7e-07      2.0e-07                       2.4e-04
#   c16_rb2                 1.3e-07      1.5e-07
#   mode0_f32_64            3.0e-07      2.7e-07
#   mode0_image_128         2.8e-07      2.9e-07
#   (e) conv_post:  C = 16  4.1e-07,  C = 32  5.8e-07,  C = 64  8.2e-07


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vispeech_amd import _lib
    return _lib.lib()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host_ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data_as(C.c_void_p).value for a in arrs])


def hip_ok(rc, what):
    """VSP_ERR_HIP from an operator: the device may have faulted, so the session ends here instead of launching more"""
    if rc == -3:
        pytest.exit(f"{what}: VSP_ERR_HIP -- the session stops", returncode=3)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(lib, route, x, ws, bs, prev, acc, div, lengths=None, grate=1, mode=None, flags=None, terms=3, want_rc=0):
    """one vsp_cl_block_ex call: out prefilled with prev; returns (out, [kernel per launch], [tile_cols per launch])"""
    from vispeech_amd import _lib
    b, t, c = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.from_numpy(np.ascontiguousarray(prev)).cuda()
    ld = None if lengths is None else torch.tensor(list(lengths), dtype=torch.int32, device="cuda")
    d = R.desc(route, b, t, x=xd.data_ptr(), out=out.data_ptr(), w=host_ptrs(ws), bias=host_ptrs(bs),
               lengths=None if ld is None else ld.data_ptr(), grate=grate, acc_prev=acc, div=div, terms=terms, mode=mode,
               flags=R.flags_for(route, acc) if flags is None else flags)
    rt = _lib.VspClBlockRoute()
    rc = lib.vsp_cl_block_ex(stream(), C.byref(d), C.byref(rt))
    hip_ok(rc, route.id)
    assert rc == want_rc, (route.id, rc)
    return out.cpu().numpy(), [l.kernel for l in rt.launch[:rt.n]], [l.tile_cols for l in rt.launch[:rt.n]]


def baseline_flags(route):
    """mode 0 as the older operators run it; for the image-form route itself the fp32-intermediate form"""
    return {"no_image": 1} if route.id == "mode0_image_128" else {}


def combos_for(route, combos):
    """g16_rc has no accumulating form: its cases run acc_prev = 0 in place of 1"""
    return [(a if a in route.acc or route.id == "chain_narrow_32_k3" else 0, d) for a, d in combos]


@functools.lru_cache(maxsize=None)
def uniform_case(rid):
    route = BY_ID[rid]
    r = np.random.Generator(np.random.PCG64(1000 + R.ROUTES.index(route)))
    b, t = 2, 2 * route.R + 37
    x = r.standard_normal((b, t, route.c)).astype(np.float32)
    prev = r.standard_normal((b, t, route.c)).astype(np.float32)
    ws, bs = R.weights(route, 2000 + R.ROUTES.index(route))
    return x, prev, ws, bs, R.block_f64(route, x, ws, bs)


def ragged_case(route, lengths, grate, T, seed):
    """x with NaN at and behind every end, the NaN-free x, prev, weights, and the fp64 block of every row alone"""
    r = np.random.Generator(np.random.PCG64(seed))
    b = len(lengths)
    clean = r.standard_normal((b, T, route.c)).astype(np.float32)
    prev = r.standard_normal((b, T, route.c)).astype(np.float32)
    ws, bs = R.weights(route, seed + 1)
    x = clean.copy()
    refs = []
    for i, l in enumerate(lengths):
        x[i, l * grate:] = np.nan
        refs.append(R.block_f64(route, clean[i:i + 1, :l * grate], ws, bs)[0])
    return x, clean, prev, ws, bs, refs


def check_ragged(lib, route, x, prev, ws, bs, refs, lengths, grate, acc, div, tol, terms=3, alone=True, what=""):
    """fp64 per row, nothing stored behind an end, the bits of the row alone through the same route; returns the largest
    error and the output"""
    ends = [l * grate for l in lengths]
    want = [(acc * prev[i, :e].astype(np.float64) + refs[i]) / div for i, e in enumerate(ends)]
    peak = max(np.abs(w).max() for w in want)
    out, kern, cols = run(lib, route, x, ws, bs, prev, acc, div, lengths=lengths, grate=grate, terms=terms)
    assert kern == route.kernels and all(c == route.R for c in cols), (kern, cols)
    worst = 0.0
    for i, e in enumerate(ends):
        assert np.isfinite(out[i, :e]).all(), (what, i, e, "a NaN leaked across the end")
        err = np.abs(out[i, :e] - want[i]).max() / peak
        worst = max(worst, err)
        assert err <= tol, (what, i, e, err)
        assert np.array_equal(bits(out[i, e:]), bits(prev[i, e:])), (what, i, e, "a row behind the end was written")
        if alone:
            o1, k1, _ = run(lib, route, x[i:i + 1, :e], ws, bs, prev[i:i + 1, :e], acc, div, terms=terms)
            assert k1 == route.kernels
            assert np.array_equal(bits(o1[0]), bits(out[i, :e])), (what, i, e, "differs from the row alone")
    return worst, out


ACC_DIV = [(0, 1.0), (1, 1.0), (1, 3.0), (0, 3.0)]


@pytest.mark.parametrize("route", R.ROUTES, ids=[r.id for r in R.ROUTES])
def test_accumulate_and_divide_on_a_uniform_batch(lib, route):
    """(a): out = (block(x) [+ prev]) / div against fp64, and the bits of mode 0 with the same epilogue"""
    x, prev, ws, bs, blk = uniform_case(route.id)
    worst = 0.0
    for acc, div in ACC_DIV:
        if acc not in route.acc:
            continue
        ref = (acc * prev.astype(np.float64) + blk) / div
        out, kern, cols = run(lib, route, x, ws, bs, prev, acc, div)
        assert kern == route.kernels and all(c == route.R for c in cols), (acc, div, kern, cols)
        err = np.abs(out - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= TOL, (acc, div, err)
        out0, _, _ = run(lib, route, x, ws, bs, prev, acc, div, mode=0, flags=baseline_flags(route))
        assert np.array_equal(bits(out), bits(out0)), (acc, div, "differs from mode 0")
    print(f"\n[measured] (a) {route.id}: {worst:.2e}")


@pytest.mark.parametrize("route", R.ROUTES, ids=[r.id for r in R.ROUTES])
def test_ragged_extents(lib, route):
    """(b)"""
    Rr, pad = route.R, R.pad_of(route)
    T = 2 * Rr + 37
    lengths = [1, pad, Rr - 1, Rr, Rr + 1, 2 * Rr, 2 * Rr + 1, T]
    x, clean, prev, ws, bs, refs = ragged_case(route, lengths, 1, T, 3000 + R.ROUTES.index(route))
    worst = 0.0
    combos = combos_for(route, [(1, 3.0), (0, 1.0)])
    for acc, div in combos:
        worst = max(worst, check_ragged(lib, route, x, prev, ws, bs, refs, lengths, 1, acc, div, TOL, what=(acc, div))[0])
    # every utterance at full length: the bits of the uniform launch
    acc, div = combos[0]
    full, _, _ = run(lib, route, clean, ws, bs, prev, acc, div, lengths=[T] * len(lengths))
    unif, _, _ = run(lib, route, clean, ws, bs, prev, acc, div)
    assert np.array_equal(bits(full), bits(unif))
    # the form the generator produces: frames of grate columns
    l8 = [1, 2, (Rr + 8) // 8, T // 8]
    x, clean, prev, ws, bs, refs = ragged_case(route, l8, 8, T, 4000 + R.ROUTES.index(route))
    worst = max(worst, check_ragged(lib, route, x, prev, ws, bs, refs, l8, 8, acc, div, TOL, what=("grate 8", acc, div))[0])
    print(f"\n[measured] (b) {route.id}: {worst:.2e}")


@pytest.mark.parametrize("rid", ["rw_k7", "rw64", "rc"])
def test_persistent_runs_across_ragged_boundaries(lib, rid):
    """(c): about 800 tiles, more than three per CU -- the persistent blocks' runs start and end inside utterances of
    different tile counts (g16_ragged_run, the T_of / tile_step cursors)"""
    route = BY_ID[rid]
    Rr = route.R
    lengths = [1, Rr, 97 * Rr + 5, 300 * Rr + 1, 410 * Rr - 1]
    T = max(lengths)
    acc, div = combos_for(route, [(1, 3.0)])[0]
    x, clean, prev, ws, bs, refs = ragged_case(route, lengths, 1, T, 5000 + R.ROUTES.index(route))
    del clean
    worst, out = check_ragged(lib, route, x, prev, ws, bs, refs, lengths, 1, acc, div, TOL, alone=False, what="persistent")
    out0, k0, _ = run(lib, route, x, ws, bs, prev, acc, div, lengths=lengths, mode=0, flags={})
    assert len(k0) == 2 * len(route.dils)
    assert np.array_equal(bits(out), bits(out0)), "differs from mode 0"
    print(f"\n[measured] (c) {route.id}: {worst:.2e}")


@pytest.mark.parametrize("rid", ["pair_ring_32_k7", "chain_64_k3", "rb2_32", "c16_rb1"])
def test_reduced_precision_ragged(lib, rid):
    """(d): the ragged case with plain f16 operands (terms = 1) on the kernels that have that instantiation"""
    route = BY_ID[rid]
    Rr, pad = route.R, R.pad_of(route)
    T = 2 * Rr + 37
    lengths = [1, pad, Rr - 1, Rr, Rr + 1, 2 * Rr, 2 * Rr + 1, T]
    x, clean, prev, ws, bs, refs = ragged_case(route, lengths, 1, T, 6000 + R.ROUTES.index(route))
    worst, _ = check_ragged(lib, route, x, prev, ws, bs, refs, lengths, 1, 1, 3.0, F16_TOL, terms=1, what="terms 1")
    print(f"\n[measured] (d) {route.id}: {worst:.2e}")


def test_a_length_outside_the_tensor_is_refused(lib):
    """zero (no route runs one: the persistent cursors step to the next utterance's first tile) and too long, on every kind of
    launch sequence, before anything is launched: out stays as it was"""
    for rid in ("rw_k7", "rc", "chain_64_k3", "rb2_32", "c16_rb1", "mode0_image_128"):
        route = BY_ID[rid]
        x, prev, ws, bs, _ = uniform_case(rid)
        T = x.shape[1]
        acc = route.acc[-1]
        for lengths, grate in (([0, T], 1), ([T, 0], 1), ([T + 1, 1], 1), ([1, -3], 1), ([T // 8 + 1, 1], 8), ([0, 1], 8)):
            out, _, _ = run(lib, route, x, ws, bs, prev, acc, 3.0, lengths=lengths, grate=grate, want_rc=ERR_ARG)
            assert np.array_equal(bits(out), bits(prev)), (rid, lengths, grate)
        run(lib, route, x, ws, bs, prev, acc, 3.0, lengths=[T // 8, 1], grate=8)


# ---- (e) conv_post
def conv_post(lib, x, w, unscale, prev, lengths=None, grate=1, slope=0.01, want_rc=0):
    b, t, c = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.from_numpy(np.ascontiguousarray(prev)).cuda()
    ld = None if lengths is None else torch.tensor(list(lengths), dtype=torch.int32, device="cuda")
    rc = lib.vsp_cl_conv_post(stream(), b, t, c, w.shape[2], C.c_void_p(xd.data_ptr()), w.ctypes.data_as(C.c_void_p), slope, unscale,
                              None if ld is None else C.c_void_p(ld.data_ptr()), grate, C.c_void_p(out.data_ptr()))
    hip_ok(rc, "conv_post")
    assert rc == want_rc, rc
    return out.cpu().numpy()


def conv_post_f64(x, w, slope=0.01):
    xt = F.leaky_relu(torch.from_numpy(np.ascontiguousarray(x)).double().transpose(1, 2), slope)
    return torch.tanh(F.conv1d(xt, torch.from_numpy(w).double(), padding=(w.shape[2] - 1) // 2))[:, 0].numpy()


@pytest.mark.parametrize("c", [16, 32, 64])
def test_conv_post_ragged(lib, c):
    k, T = 7, 600
    r = np.random.Generator(np.random.PCG64(7000 + c))
    w = (r.standard_normal((1, c, k)) / np.sqrt(c * k)).astype(np.float32)      # (the sum stays unsaturated)
    worst = 0.0
    for lengths, grate in (([1, 3, 255, 256, 257, T], 1), ([1, 32, 33, T // 8], 8)):
        b = len(lengths)
        clean = r.standard_normal((b, T, c)).astype(np.float32)
        prev = r.standard_normal((b, T)).astype(np.float32)
        x = clean.copy()
        for i, l in enumerate(lengths):
            x[i, l * grate:] = np.nan
        out = conv_post(lib, x, w, 1.0, prev, lengths, grate)
        for i, l in enumerate(lengths):
            e = l * grate
            ref = conv_post_f64(clean[i:i + 1, :e], w)[0]
            assert np.isfinite(out[i, :e]).all(), (i, e, "a NaN leaked across the end")
            err = np.abs(out[i, :e] - ref).max()
            worst = max(worst, err)
            assert err <= POST_TOL, (grate, i, e, err)
            assert np.array_equal(bits(out[i, e:]), bits(prev[i, e:])), (grate, i, e, "a row behind the end was written")
        # unscale: powers of two are exact
        assert np.array_equal(bits(conv_post(lib, x * np.float32(16.0), w, 2.0 ** -4, prev, lengths, grate)), bits(out))
        # every utterance at full length: the uniform launch
        full = conv_post(lib, clean, w, 1.0, prev, [T // grate] * b, grate)
        unif = conv_post(lib, clean[:, :T // grate * grate], w, 1.0, prev[:, :T // grate * grate])
        assert np.array_equal(bits(full[:, :T // grate * grate]), bits(unif))
        assert np.abs(unif - conv_post_f64(clean[:, :T // grate * grate], w)).max() <= POST_TOL
    for lengths, grate in (([0, 1, 1, 1], 1), ([T + 1, 1, 1, 1], 1), ([T // 8 + 1, 1, 1, 1], 8)):
        out = conv_post(lib, clean, w, 1.0, prev, lengths, grate, want_rc=ERR_ARG)
        assert np.array_equal(bits(out), bits(prev))
    print(f"\n[measured] (e) conv_post C = {c}: {worst:.2e} absolute")
