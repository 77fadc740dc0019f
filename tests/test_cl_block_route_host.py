"""Which kernel every launch of a channels-last ResBlock takes (the route functions the launchers of gen16*.hip switch on:
g16_conv_route, g16_pair_route, g16_chain_route, g16_rb2_route, g16_c16_route), checked without a GPU through plan-only
calls of vsp_cl_block_ex: the shapes tests/test_cl_block_ops.py runs report the route they were written for, the flags flip
the kernels they name, an accumulating k3 block of the 32-channel stage leaves g16_rc, a ragged image-form launch never goes
to g16_pipe, the tile widths are the constants' arithmetic, and refusals come back as error codes.  (A length outside
[1, T / grate] needs the device array: tests/test_cl_block_ops.py checks that refusal.)"""
import ctypes as C

import pytest

import cl_block_ref as R
from cl_block_ref import ERR_ARG, ERR_UNSUPPORTED, BY_ID, plan
from vispeech_amd import _lib as L


def kernels(route):
    return [k for k, _, _, _ in route]


@pytest.mark.parametrize("route", R.ROUTES, ids=[r.id for r in R.ROUTES])
def test_every_gpu_test_shape_reports_its_route(route):
    """at the three batch shapes of tests/test_cl_block_ops.py (a), (b) and the grate-8 form, with and without lengths"""
    T = 2 * route.R + 37
    for acc in route.acc:
        for B, lengths in ((2, None), (8, 0x50000), (4, 0x50000), (1, None)):
            rc, rt = plan(route, B, T, acc_prev=acc, div=3.0, lengths=lengths, flags=R.flags_for(route, acc))
            assert rc == 0, (acc, B)
            assert kernels(rt) == route.kernels, (acc, B, rt)
            assert all(cols == route.R for _, cols, _, _ in rt), (acc, B, rt)
    # the bit-for-bit baseline of those tests: mode 0, one g16_conv launch per convolution, 256 stored columns per tile
    rc, rt = plan(route, 2, T, mode=0, flags={})
    n = 2 if route.kind == 2 else 2 * len(route.dils)
    assert rc == 0 and len(rt) == n
    if route.c == 16:
        assert kernels(rt) == [L.CL_KERNEL_C16] * n
    elif route.kind == 2:
        assert kernels(rt) == [L.CL_KERNEL_CONV] * n and all(cols == 256 for _, cols, _, _ in rt)
    else:   # the operator's default hands a pair's intermediate over as an operand image (terms 3, K >= 3)
        assert kernels(rt) == [L.CL_KERNEL_CONV, L.CL_KERNEL_CONV_IMG] * (n // 2) and all(cols == 256 for _, cols, _, _ in rt)


def test_persistent_run_shapes_report_their_route():
    """tests/test_cl_block_ops.py (c): five utterances up to 410 R - 1 columns, one launch per pair / per block"""
    for rid, acc in (("rw_k7", 1), ("rw64", 1), ("rc", 0)):
        route = BY_ID[rid]
        rc, rt = plan(route, 5, 410 * route.R - 1, acc_prev=acc, div=3.0, lengths=0x50000)
        assert rc == 0 and kernels(rt) == route.kernels and all(cols == route.R for _, cols, _, _ in rt), (rid, rt)


def test_reduced_precision_shapes_report_their_route():
    """terms = 1 has no register-weights kernel: the ring tiles, g16_rb2 and g16_c16 (tests/test_cl_block_ops.py (d))"""
    for rid, want in (("pair_ring_32_k7", L.CL_KERNEL_PAIR), ("rw_k7", L.CL_KERNEL_PAIR), ("chain_64_k3", L.CL_KERNEL_CHAIN),
                      ("rc", L.CL_KERNEL_CHAIN), ("rb2_32", L.CL_KERNEL_RB2), ("c16_rb1", L.CL_KERNEL_C16)):
        route = BY_ID[rid]
        rc, rt = plan(route, 8, 2 * route.R + 37, terms=1, acc_prev=1, div=3.0, lengths=0x50000)
        assert rc == 0 and set(kernels(rt)) == {want}, (rid, rt)


def test_flags_flip_the_kernels_they_name():
    rw, p64, rc = BY_ID["rw_k7"], BY_ID["pair_64_k3"], BY_ID["rc"]
    # ring: g16_rw -> the pair ring tile (K = 3, 7 and 11 alike)
    assert kernels(plan(rw, 2, 500, flags={})[1]) == [L.CL_KERNEL_RW] * 3
    assert plan(rw, 2, 500, flags={"ring": 1})[1] == [(L.CL_KERNEL_PAIR, 256 - 6, 0, 8)] * 3
    assert plan(BY_ID["rw_k11"], 2, 500, flags={"ring": 1})[1] == [(L.CL_KERNEL_PAIR, 256 - 10, 0, 8)] * 2
    k3 = rc._replace(mode=1)
    assert plan(k3, 2, 500, flags={})[1] == [(L.CL_KERNEL_RW, 192 - 2, 0, 0)] * 3
    assert plan(k3, 2, 500, flags={"ring": 1})[1] == [(L.CL_KERNEL_PAIR, 256 - 2, 0, 8)] * 3
    # rw64: the 64-channel ring tile -> g16_rw64; ring wins over rw64; rw64 means nothing at 32 channels or kernel 7
    assert kernels(plan(p64, 2, 500, flags={})[1]) == [L.CL_KERNEL_PAIR] * 3
    assert plan(p64, 2, 500, flags={"rw64": 1})[1] == [(L.CL_KERNEL_RW64, 96 - 2, 0, 0)] * 3
    assert kernels(plan(p64, 2, 500, flags={"rw64": 1, "ring": 1})[1]) == [L.CL_KERNEL_PAIR] * 3
    assert kernels(plan(rw, 2, 500, flags={"rw64": 1})[1]) == [L.CL_KERNEL_RW] * 3
    assert kernels(plan(p64._replace(k=7, dils=(1, 3)), 2, 500, flags={"rw64": 1})[1]) == [L.CL_KERNEL_PAIR] * 2
    # chain_ring: g16_rc -> the chain ring tile
    assert plan(rc, 2, 500, flags={})[1] == [(L.CL_KERNEL_RC, 192 - 24, 0, 0)]
    assert plan(rc, 2, 500, flags={"chain_ring": 1})[1] == [(L.CL_KERNEL_CHAIN, 256 - 24, 0, 0)]
    # no_image: the pair's intermediate as an fp32 tensor instead of an operand image
    m0 = BY_ID["mode0_image_128"]
    assert kernels(plan(m0, 2, 500, flags={})[1]) == [L.CL_KERNEL_CONV, L.CL_KERNEL_CONV_IMG] * 2
    assert kernels(plan(m0, 2, 500, flags={"no_image": 1})[1]) == [L.CL_KERNEL_CONV] * 4
    # the flags mean nothing to a ResBlock2 or to 16 channels
    for rid in ("rb2_32", "c16_rb1"):
        r = BY_ID[rid]
        assert plan(r, 2, 500, flags={"ring": 1, "rw64": 1, "chain_ring": 1, "no_image": 1}) == plan(r, 2, 500, flags={})


def test_an_accumulating_k3_block_of_the_32_channel_stage_takes_the_chain_ring():
    rc = BY_ID["rc"]
    assert plan(rc, 2, 500, acc_prev=0)[1] == [(L.CL_KERNEL_RC, 168, 0, 0)]
    assert plan(rc, 2, 500, acc_prev=1)[1] == [(L.CL_KERNEL_CHAIN, 232, 0, 0)]
    assert plan(rc, 2, 500, acc_prev=0, div=3.0)[1] == [(L.CL_KERNEL_RC, 168, 0, 0)]       # (the divide alone stays)
    # g16_rc is that one block: three pairs, kernel 3, dilations <= 8, split products
    assert kernels(plan(rc._replace(dils=(1, 3)), 2, 500)[1]) == [L.CL_KERNEL_CHAIN]
    assert kernels(plan(rc._replace(dils=(1, 3, 9)), 2, 500)[1]) == [L.CL_KERNEL_CHAIN]
    assert kernels(plan(rc._replace(dils=(1, 3, 8)), 2, 500)[1]) == [L.CL_KERNEL_RC]
    assert kernels(plan(rc, 2, 500, terms=1)[1]) == [L.CL_KERNEL_CHAIN]


@pytest.mark.parametrize("c,k,dils", [(128, 3, (1, 5)), (128, 7, (3,)), (256, 3, (1,))])
def test_a_ragged_image_form_launch_never_goes_to_g16_pipe(c, k, dils):
    """g16_convp walks uniform tiles: with lengths the 128-row image-input tile runs one block per tile instead.  The grid
    must be large enough for the 128-row tile (200 column tiles x row groups) for the question to arise at all."""
    r = BY_ID["mode0_image_128"]._replace(c=c, k=k, dils=dils)
    B, T = 64, 2048                                              # 512 column tiles
    rc, rt = plan(r, B, T)
    assert rc == 0 and rt == [(L.CL_KERNEL_CONV, 256, 128, 1), (L.CL_KERNEL_PIPE, 256, 128, 0)] * len(dils), rt
    for grate in (1, 8):
        rc, rt = plan(r, B, T, lengths=0x50000, grate=grate)
        assert rc == 0 and rt == [(L.CL_KERNEL_CONV, 256, 128, 1), (L.CL_KERNEL_CONV_IMG, 256, 128, 0)] * len(dils), rt
    rc, rt = plan(r, B, T, lengths=0x50000, acc_prev=1, div=3.0)
    assert rc == 0 and L.CL_KERNEL_PIPE not in kernels(rt)
    # small grids: the 64- and 32-row tiles, never the persistent kernel
    assert plan(r, 1, 2048)[1][1] == (L.CL_KERNEL_CONV_IMG, 256, 32, 0)             # 8 column tiles x c / 64 row groups < 200
    B = 16 if c == 128 else 8                                                       # 8 B x c / 128 < 200 <= 8 B x c / 64
    assert plan(r, B, 2048)[1][1] == (L.CL_KERNEL_CONV_IMG, 256, 64, 0)


def test_g16_conv_row_tile_follows_the_grid():
    """launch_g16_conv's fill rule: fewer than 200 (column tiles x 128-row groups) -> 64 rows, x 64-row groups too -> 32"""
    r = BY_ID["mode0_f32_64"]._replace(c=128)                    # fp32 intermediate, 128 rows
    rows = lambda B, T: {x[2] for x in plan(r, B, T)[1]}
    assert rows(1, 256 * 99) == {32}                             # 99 x 2 < 200
    assert rows(1, 256 * 100) == {64}                            # 100 x 2 = 200, 100 x 1 < 200
    assert rows(1, 256 * 199) == {64}
    assert rows(1, 256 * 200) == {128}
    assert rows(8, 256 * 25) == {128}                            # B counts
    assert rows(8, 256 * 25 - 256) == {64}
    r64 = BY_ID["mode0_f32_64"]
    assert {x[2] for x in plan(r64, 1, 256 * 199)[1]} == {32} and {x[2] for x in plan(r64, 1, 256 * 200)[1]} == {64}


def test_tile_widths_are_the_constants_arithmetic():
    """tile_cols for K and dilations other than the table's: conv1's columns - (K - 1) for the pair kernels, the block's
    columns - 2 * halo for the chain, ResBlock2 and 16-channel kernels"""
    for k in (3, 7, 11):
        for d in (1, 2, 5):
            r = BY_ID["rw_k7"]._replace(k=k, dils=(d,))
            assert plan(r, 2, 500, flags={})[1] == [(L.CL_KERNEL_RW, 192 - (k - 1), 0, 0)]
            assert plan(r, 2, 500, flags={"ring": 1})[1] == [(L.CL_KERNEL_PAIR, 256 - (k - 1), 0, 8)]
            assert plan(r._replace(c=64), 2, 500, flags={})[1] == [(L.CL_KERNEL_PAIR, 256 - (k - 1), 0, 8)]
    assert plan(BY_ID["rw_k7"]._replace(k=5, dils=(2,)), 2, 500, flags={})[1] == [(L.CL_KERNEL_PAIR, 252, 0, 8)]   # (no K = 5 g16_rw)
    assert plan(BY_ID["rw_k7"]._replace(k=7, dils=(10,)), 2, 500, flags={})[1] == [(L.CL_KERNEL_PAIR, 250, 0, 8)]  # (60 > RW_MAXHALO 56)
    for k, d in ((3, 1), (3, 8), (7, 1), (7, 5)):
        assert plan(BY_ID["pp_k3"]._replace(k=k, dils=(d,)), 2, 500)[1] == [(L.CL_KERNEL_PP, 192 - (k - 1), 0, 0)]
    for c, k, dils in ((32, 3, (1, 3, 5)), (32, 5, (2, 1, 4)), (32, 7, (1, 3, 5)), (32, 11, (1, 3)), (64, 7, (1, 3)), (64, 11, (5,)),
                       (128, 3, (5,)), (128, 7, (3,))):
        halo = R.chain_halo(k, dils)
        wide = c == 32 and 2 * halo > 64
        want = (L.CL_KERNEL_CHAIN_WIDE if wide else L.CL_KERNEL_CHAIN, (512 if wide else 128 if c == 128 else 256) - 2 * halo, 0, 0)
        assert plan(BY_ID["chain_64_k3"]._replace(c=c, k=k, dils=dils), 2, 500, flags={"chain_ring": 1})[1] == [want], (c, k, dils)
    for c, k, dils in ((32, 3, (1, 3)), (32, 7, (2, 6)), (32, 11, (3, 5)), (64, 11, (3, 5)), (64, 3, (1, 2))):
        halo = (dils[0] + dils[1]) * ((k - 1) // 2)
        wide = c == 32 and 2 * halo > 64
        assert plan(BY_ID["rb2_32"]._replace(c=c, k=k, dils=dils), 2, 500)[1] == [(L.CL_KERNEL_RB2, (512 if wide else 256) - 2 * halo, 0, int(wide))]
    for k, dils in ((3, (1, 3, 5)), (7, (1, 3)), (11, (2,))):
        halo = sum((d + 1) * ((k - 1) // 2) for d in dils)
        assert plan(BY_ID["c16_rb1"]._replace(k=k, dils=dils), 2, 500)[1] == [(L.CL_KERNEL_C16, 512 - 2 * halo, 0, 0)]
        # mode 1: a pair per launch; mode 0: a convolution per launch, its own halo each
        assert plan(BY_ID["c16_rb1"]._replace(k=k, dils=dils, mode=1), 2, 500)[1] == \
            [(L.CL_KERNEL_C16, 512 - 2 * (d + 1) * ((k - 1) // 2), 0, 0) for d in dils]
        assert plan(BY_ID["c16_rb1"]._replace(k=k, dils=dils, mode=0), 2, 500)[1] == \
            [(L.CL_KERNEL_C16, 512 - 2 * dd * ((k - 1) // 2), 0, 0) for d in dils for dd in (d, 1)]


def _raw(route, B=2, T=300, route_out=True, **fields):
    """plan-only with descriptor fields overridden after the route's own"""
    d = R.desc(route, B, T, plan_only=1)
    for k, v in fields.items():
        setattr(d, k, v)
    rt = L.VspClBlockRoute()
    return L.lib().vsp_cl_block_ex(None, C.byref(d), C.byref(rt) if route_out else None)


def test_refusals_come_back_as_error_codes():
    lib = L.lib()
    rw, rc, rb2, c16 = BY_ID["rw_k7"], BY_ID["rc"], BY_ID["rb2_32"], BY_ID["c16_rb1"]
    for r in R.ROUTES:
        assert _raw(r) == 0, r.id
    rt = L.VspClBlockRoute()
    assert lib.vsp_cl_block_ex(None, None, C.byref(rt)) == ERR_ARG
    assert _raw(rw, route_out=False) == ERR_ARG                                      # a plan with nowhere to go
    # ---- VSP_ERR_ARG
    for fields in (dict(x=None), dict(out=None), dict(w=None), dict(bias=None), dict(dilations=None), dict(out=0x10000),  # x == out
                   dict(B=-1), dict(T=-1), dict(kind=0), dict(kind=3), dict(mode=-1), dict(mode=3), dict(terms=2), dict(terms=0),
                   dict(n_pairs=0), dict(n_pairs=9), dict(div=0.0), dict(div=-0.0), dict(grate=0), dict(grate=-8)):
        assert _raw(rw, **fields) == ERR_ARG, fields
    assert _raw(rb2, mode=2) == ERR_ARG                                              # a ResBlock2 has modes 0 and 1
    d = R.desc(rw, 2, 300, plan_only=1)
    d._tables[0][3] = None                                                           # a missing weight
    assert lib.vsp_cl_block_ex(None, C.byref(d), C.byref(rt)) == ERR_ARG
    assert _raw(rw, div=-2.0) == 0 and _raw(rw, div=0.5) == 0
    # ---- VSP_ERR_UNSUPPORTED: the shapes vsp_cl_resblock / vsp_cl_resblock2 refuse
    for fields in (dict(C=48), dict(C=0), dict(C=8), dict(K=4), dict(K=0), dict(T=1 << 24)):   # (T C 4 bytes reach 2^31)
        assert _raw(rw, **fields) == ERR_UNSUPPORTED, fields
    assert _raw(rw._replace(dils=(1, 11))) == ERR_UNSUPPORTED                        # (K - 1) dil = 66 > 64
    assert _raw(rw._replace(dils=(1, 0))) == ERR_UNSUPPORTED
    assert _raw(rw._replace(c=128, k=11, dils=(1,))) == ERR_UNSUPPORTED              # pairs: 32 / 64 channels, 128 at kernel 3 / 7
    assert _raw(rw._replace(c=256, k=3, dils=(1,))) == ERR_UNSUPPORTED
    assert _raw(rw._replace(c=256, k=3, dils=(1,), mode=0)) == 0                     # mode 0: any C % 32 == 0
    assert _raw(rc._replace(c=256)) == ERR_UNSUPPORTED                               # chains: 32 / 64 / 128 channels
    assert _raw(rc._replace(dils=(1, 3, 5, 7))) == ERR_UNSUPPORTED                   # ... of at most three pairs
    assert _raw(rc._replace(c=128, k=11, dils=(1, 3, 5))) == ERR_UNSUPPORTED         # ... whose halo leaves 32 columns of a tile
    assert _raw(rb2._replace(c=128)) == ERR_UNSUPPORTED                              # g16_rb2: 32 / 64 channels
    assert _raw(rb2._replace(c=128, mode=0)) == 0
    assert _raw(rb2._replace(k=11, dils=(1, 7))) == ERR_UNSUPPORTED                  # (K - 1) dil = 70 > 64
    assert _raw(rb2._replace(c=48)) == ERR_UNSUPPORTED
    assert _raw(c16._replace(c=16, dils=(1, 3, 5, 7))) == ERR_UNSUPPORTED           # the 16-channel block: at most three pairs too
    # B = 0 or T = 0: nothing to do, an empty route
    for fields in (dict(B=0), dict(T=0)):
        d = R.desc(rw, 2, 300, plan_only=1)
        for k, v in fields.items():
            setattr(d, k, v)
        rt.n = 7
        assert lib.vsp_cl_block_ex(None, C.byref(d), C.byref(rt)) == 0 and rt.n == 0


def test_the_two_older_operators_refuse_what_they_did():
    """vsp_cl_resblock / vsp_cl_resblock2 are wrappers of the same implementation: their argument checks need no device"""
    lib = L.lib()
    one = (C.c_int * 1)(1)
    d13 = (C.c_int * 2)(1, 3)
    tab = (C.c_void_p * 16)(*[0x30000] * 16)
    x, o = 0x10000, 0x20000
    assert lib.vsp_cl_resblock(None, 1, 8, 32, 3, 1, one, x, tab, tab, 2, 3, x) == ERR_ARG             # in place
    assert lib.vsp_cl_resblock(None, 1, 8, 32, 3, 0, one, x, tab, tab, 2, 3, o) == ERR_ARG
    assert lib.vsp_cl_resblock(None, 1, 8, 32, 3, 9, one, x, tab, tab, 0, 3, o) == ERR_ARG
    assert lib.vsp_cl_resblock(None, 1, 8, 32, 3, 1, one, x, tab, tab, 3, 3, o) == ERR_ARG
    assert lib.vsp_cl_resblock(None, 1, 8, 128, 11, 1, one, x, tab, tab, 1, 3, o) == ERR_UNSUPPORTED
    assert lib.vsp_cl_resblock(None, 1, 8, 48, 3, 1, one, x, tab, tab, 0, 3, o) == ERR_UNSUPPORTED
    assert lib.vsp_cl_resblock(None, 1, 0, 32, 3, 1, one, x, tab, tab, 2, 3, o) == 0                   # empty
    assert lib.vsp_cl_resblock2(None, 1, 8, 32, 11, d13, x, tab, tab, 1, 3, x) == ERR_ARG
    assert lib.vsp_cl_resblock2(None, 1, 8, 32, 11, d13, x, tab, tab, 2, 3, o) == ERR_ARG              # mode
    assert lib.vsp_cl_resblock2(None, 1, 8, 32, 11, d13, x, tab, tab, 1, 2, o) == ERR_ARG              # terms
    assert lib.vsp_cl_resblock2(None, 1, 8, 128, 3, d13, x, tab, tab, 1, 3, o) == ERR_UNSUPPORTED
    assert lib.vsp_cl_resblock2(None, 1, 0, 32, 11, d13, x, tab, tab, 1, 3, o) == 0


def test_conv_post_refusals():
    lib = L.lib()
    x, w, o = 0x10000, 0x30000, 0x20000
    for args in ((1, 8, 32, 7, None, w, 0.01, 1.0, None, 1, o), (1, 8, 32, 7, x, None, 0.01, 1.0, None, 1, o),
                 (1, 8, 32, 7, x, w, 0.01, 1.0, None, 1, None), (-1, 8, 32, 7, x, w, 0.01, 1.0, None, 1, o),
                 (1, -8, 32, 7, x, w, 0.01, 1.0, None, 1, o), (1, 8, 32, 7, x, w, 0.01, 1.0, None, 0, o)):
        assert lib.vsp_cl_conv_post(None, *args) == ERR_ARG, args
    for c, k in ((48, 7), (128, 7), (0, 7), (32, 9), (32, 4), (32, 0)):
        assert lib.vsp_cl_conv_post(None, 1, 8, c, k, x, w, 0.01, 1.0, None, 1, o) == ERR_UNSUPPORTED, (c, k)
    assert lib.vsp_cl_conv_post(None, 0, 8, 32, 7, x, w, 0.01, 1.0, None, 1, o) == 0
    assert lib.vsp_cl_conv_post(None, 1, 0, 32, 7, x, w, 0.01, 1.0, None, 1, o) == 0
