"""Shared by tests/test_cl_block_route_host.py (no GPU) and tests/test_cl_block_ops.py (GPU): the table of ResBlock routes
those tests cover -- one shape per kernel route of the channels-last vocoder, with the kernel and the stored columns per
tile (R) the shape was written for --, the descriptor of vsp_cl_block_ex, and the fp64 reference of a block.

The expected tile widths are written out from the kernels' constants: RW_BT = 192 (gen16_rw.hip), R6_BT = 96
(gen16_rw64.hip), RC_BT = 192 (gen16_rc.hip), 192 columns of the ping-pong tile (gen16_pp.hip), 256 columns of the LDS-ring
pair tile and of g16_conv, 256 / 512 / 128 columns of the chain and ResBlock2 tiles (gen16.hip, gen16_rb2.hip),
G16_C16_BT = 512 (kernels.h)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from vispeech_amd import _lib

ERR_ARG, ERR_UNSUPPORTED = -1, -7
K_ = _lib   # (the CL_KERNEL_* names)

# kind 1 = ResBlock1 (dils: one per pair), 2 = ResBlock2 (dils: two).  flags: ring / rw64 / chain_ring / no_image.
# acc: the acc_prev values this route exists for (g16_rc refuses acc_prev: the accumulating block takes the chain ring).
# kernels: one per launch.  R: columns one tile stores.
Route = namedtuple("Route", "id kind c k dils mode flags acc kernels R")


def chain_halo(k, dils):
    return sum((d + 1) * ((k - 1) // 2) for d in dils)


def c16_halo(k, step_dils):
    return sum(d * ((k - 1) // 2) for d in step_dils)


ROUTES = [
    Route("rw_k7", 1, 32, 7, (1, 3, 5), 1, {}, (0, 1), [K_.CL_KERNEL_RW] * 3, 192 - 6),
    Route("rw_k11", 1, 32, 11, (1, 5), 1, {}, (0, 1), [K_.CL_KERNEL_RW] * 2, 192 - 10),
    Route("pair_ring_32_k7", 1, 32, 7, (1, 3), 1, {"ring": 1}, (0, 1), [K_.CL_KERNEL_PAIR] * 2, 256 - 6),
    Route("pair_64_k3", 1, 64, 3, (1, 3, 5), 1, {}, (0, 1), [K_.CL_KERNEL_PAIR] * 3, 256 - 2),
    Route("rw64", 1, 64, 3, (1, 3, 5), 1, {"rw64": 1}, (0, 1), [K_.CL_KERNEL_RW64] * 3, 96 - 2),
    Route("pp_k3", 1, 128, 3, (1, 5), 1, {}, (0, 1), [K_.CL_KERNEL_PP] * 2, 192 - 2),
    Route("pp_k7", 1, 128, 7, (1, 3), 1, {}, (0, 1), [K_.CL_KERNEL_PP] * 2, 192 - 6),
    Route("rc", 1, 32, 3, (1, 3, 5), 2, {}, (0,), [K_.CL_KERNEL_RC], 192 - 2 * chain_halo(3, (1, 3, 5))),
    # the same block ACCUMULATING falls back to the ring chain by itself; without acc_prev only the flag keeps it there
    Route("chain_narrow_32_k3", 1, 32, 3, (1, 3, 5), 2, {}, (1,), [K_.CL_KERNEL_CHAIN], 256 - 2 * chain_halo(3, (1, 3, 5))),
    Route("chain_wide_32_k11", 1, 32, 11, (1, 3, 5), 2, {}, (0, 1), [K_.CL_KERNEL_CHAIN_WIDE], 512 - 2 * chain_halo(11, (1, 3, 5))),
    Route("chain_64_k3", 1, 64, 3, (1, 3, 5), 2, {}, (0, 1), [K_.CL_KERNEL_CHAIN], 256 - 2 * chain_halo(3, (1, 3, 5))),
    Route("chain_128_k3", 1, 128, 3, (1,), 2, {}, (0, 1), [K_.CL_KERNEL_CHAIN], 128 - 2 * chain_halo(3, (1,))),
    Route("rb2_32", 2, 32, 3, (1, 3), 1, {}, (0, 1), [K_.CL_KERNEL_RB2], 256 - 2 * 4),
    Route("rb2_64", 2, 64, 5, (1, 3), 1, {}, (0, 1), [K_.CL_KERNEL_RB2], 256 - 2 * 8),
    Route("rb2_32_wide", 2, 32, 11, (1, 6), 1, {}, (0, 1), [K_.CL_KERNEL_RB2], 512 - 2 * 35),
    Route("c16_rb1", 1, 16, 3, (1, 3, 5), 2, {}, (0, 1), [K_.CL_KERNEL_C16], 512 - 2 * c16_halo(3, (1, 1, 3, 1, 5, 1))),
    Route("c16_rb2", 2, 16, 3, (1, 3), 1, {}, (0, 1), [K_.CL_KERNEL_C16], 512 - 2 * c16_halo(3, (1, 3))),
    Route("mode0_f32_64", 1, 64, 7, (1, 3), 0, {"no_image": 1}, (0, 1), [K_.CL_KERNEL_CONV] * 4, 256),
    Route("mode0_image_128", 1, 128, 3, (1, 5), 0, {}, (0, 1), [K_.CL_KERNEL_CONV, K_.CL_KERNEL_CONV_IMG] * 2, 256),
]
BY_ID = {r.id: r for r in ROUTES}


def pad_of(route):
    """half of the largest (K - 1) * dilation of the block"""
    return (route.k - 1) * max(route.dils) // 2


def flags_for(route, acc_prev):
    """the route's flags; the narrow chain without acc_prev needs chain_ring to stay off g16_rc"""
    f = dict(route.flags)
    if route.id == "chain_narrow_32_k3" and not acc_prev:
        f["chain_ring"] = 1
    return f


def desc(route, B, T, x=0x10000, out=0x20000, w=None, bias=None, lengths=None, grate=1, acc_prev=0, div=1.0, terms=3,
         mode=None, plan_only=0, flags=None):
    """vsp_cl_block_desc of a route's shape.  x / out / lengths: addresses (the defaults serve plan-only calls); w / bias:
    ctypes tables of host pointers, one per convolution (default: non-null entries nothing dereferences -- a plan reads the
    tables for NULL entries, never the weights)."""
    d = _lib.VspClBlockDesc()
    d.kind, d.mode, d.B, d.T, d.C, d.K = route.kind, route.mode if mode is None else mode, B, T, route.c, route.k
    d.n_pairs, d.terms = (len(route.dils) if route.kind == 1 else 0), terms
    darr = (C.c_int32 * len(route.dils))(*route.dils)
    d._dilations = darr                      # (the descriptor points into it: same lifetime)
    d.dilations = C.cast(darr, C.c_void_p)
    n = 2 if route.kind == 2 else 2 * len(route.dils)
    d._tables = (w if w is not None else (C.c_void_p * n)(*[0x30000] * n), bias if bias is not None else (C.c_void_p * n)(*[0x40000] * n))
    d.w, d.bias = C.cast(d._tables[0], C.c_void_p), C.cast(d._tables[1], C.c_void_p)
    d.x, d.out, d.lengths = x, out, lengths
    d.grate, d.acc_prev, d.div, d.plan_only = grate, acc_prev, div, plan_only
    for name, v in (route.flags if flags is None else flags).items():
        setattr(d, name, v)
    return d


def plan(route, B, T, **kw):
    """(rc, [(kernel, tile_cols, rows, variant) per launch]) of a plan-only call: no device, no HIP call"""
    d = desc(route, B, T, plan_only=1, **kw)
    rt = _lib.VspClBlockRoute()
    rc = _lib.lib().vsp_cl_block_ex(None, C.byref(d), C.byref(rt))
    return rc, [(l.kernel, l.tile_cols, l.rows, l.variant) for l in rt.launch[:rt.n]]


# ---- the fp64 reference (torch on the CPU): tests/test_cl_ops.py torch_resblock and its ResBlock2 analogue
def block_f64(route, x, ws, bs):
    """x [B][T][C] float32 -> the block in fp64, [B][T][C] (zero padding at both ends of the tensor)"""
    import torch
    import torch.nn.functional as F
    k = route.k
    y = torch.from_numpy(np.ascontiguousarray(x)).double().transpose(1, 2)
    W = [torch.from_numpy(w).double() for w in ws]
    Bv = [torch.from_numpy(b).double() for b in bs]
    if route.kind == 2:
        for c, d in enumerate(route.dils):
            y = F.conv1d(F.leaky_relu(y, 0.1), W[c], Bv[c], dilation=d, padding=d * (k - 1) // 2) + y
    else:
        for p, d in enumerate(route.dils):
            t = F.conv1d(F.leaky_relu(y, 0.1), W[2 * p], Bv[2 * p], dilation=d, padding=d * (k - 1) // 2)
            y = F.conv1d(F.leaky_relu(t, 0.1), W[2 * p + 1], Bv[2 * p + 1], padding=(k - 1) // 2) + y
    return y.transpose(1, 2).numpy()


def weights(route, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    n = 2 if route.kind == 2 else 2 * len(route.dils)
    c, k = route.c, route.k
    ws = [(r.standard_normal((c, c, k)) / np.sqrt(c * k)).astype(np.float32) for _ in range(n)]
    bs = [(r.standard_normal(c) * 0.1).astype(np.float32) for _ in range(n)]
    return ws, bs
