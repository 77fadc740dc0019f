"""The scratch overlay through the public ABI, host side (no GPU): a sequence whose stages run one after another on one
stream needs its own tensors (the head) plus the LARGEST of its stages' workspaces, each stage as its own
``vsp_*_workspace_bytes`` sizes it.  A stage left out of that maximum would overflow at run time only for the shapes where
it is the largest, so the cases are chosen -- and checked here -- to make every stage of every identity the strict
maximum at least once.

The heads restate the allocations in front of the overlay (every allocation is rounded up to 256 bytes; a ``t3`` tensor
pads its time axis to 64):
  vsp_infer           x_var [B][h][Tp], g [B][gin], cum_dur int32 [B][Tp]                  (infer_impl, api_frame.hip)
  vsp_voice_conversion  g_src, g_tgt [B][gin]; m_q, logs_q as t3 [B][inter][T] -- the sizing pass has no caller tensors
                                                                                           (vc_impl, api_convert.hip)
  vsp_convert_latent  g_src [B][gin], spec [B][spec][T], z, z_p, m_q, logs_q, drawn [B][inter][T], seeds uint64 [B]
                                                                                           (convert_latent_impl)
"""
import ctypes as C

import pytest

from vispeech_amd import _lib
from vispeech_amd.schema import ModelDims

# a generator smaller than the frame-rate stages, a spectrogram smaller than the posterior encoder, and posterior
# encoders with less / more conditioning than the flow (the default 16 layers tie with the flow's 4 x 4)
SMALL = dict(upsample_rates=[2], upsample_kernel_sizes=[4], upsample_initial_channel=32, resblock_kernel_sizes=[3],
             resblock_dilation_sizes=[[1]], spec_channels=65)
CONFIGS = {"default": {}, "flow_heavy": dict(SMALL, posterior_layers=4), "posterior_heavy": dict(SMALL, posterior_layers=32)}


def r256(n):
    return (n + 255) // 256 * 256


def pad64(t):
    return (t + 63) // 64 * 64


@pytest.fixture(scope="module")
def ctxs():
    lib, out = _lib.lib(), {}
    for name, fields in CONFIGS.items():
        d = ModelDims()
        for k, v in fields.items():
            setattr(d, k, v)
        cfg, h = _lib.make_config(d), C.c_void_p()
        assert lib.vsp_create(C.byref(cfg), 0, C.byref(h)) == 0, lib.vsp_last_error(h)
        out[name] = (h, d)
    yield lib, out
    for h, _ in out.values():
        lib.vsp_destroy(h)


def check(cases, names):
    """cases: (total, head, stage sizes); every stage positive, the identity, and each stage the strict maximum once."""
    strict = set()
    for total, head, stages in cases:
        assert all(s > 0 for s in stages) and total == head + max(stages), (total, head, stages)
        top = [i for i, s in enumerate(stages) if s == max(stages)]
        if len(top) == 1:
            strict.add(names[top[0]])
    assert strict == set(names), f"never the strict maximum: {set(names) - strict}"


def test_infer_is_its_head_plus_the_larger_of_encode_and_decode(ctxs):
    lib, c = ctxs
    h, d = c["default"]
    cases = []
    for B, Tp, Tf in ((1, 301, 1), (3, 40, 65), (2, 7, 64)):
        head = r256(4 * B * d.hidden_channels * Tp) + r256(4 * B * d.gin_channels) + r256(4 * B * Tp)
        cases.append((lib.vsp_infer_workspace_bytes(h, B, Tp, Tf), head,
                      (lib.vsp_encode_workspace_bytes(h, B, Tp), lib.vsp_decode_workspace_bytes(h, B, Tp, Tf))))
    check(cases, ("encode", "decode"))


def test_voice_conversion_is_its_head_plus_the_largest_of_posterior_flow_and_generator(ctxs):
    lib, c = ctxs
    cases = []
    for name in CONFIGS:
        h, d = c[name]
        for B, T in ((1, 1), (3, 65)):
            head = 2 * r256(4 * B * d.gin_channels) + 2 * r256(4 * B * d.inter_channels * pad64(T))
            cases.append((lib.vsp_voice_conversion_workspace_bytes(h, B, T), head,
                          (lib.vsp_posterior_workspace_bytes(h, B, T), lib.vsp_flow_workspace_bytes(h, B, T),
                           lib.vsp_generator_workspace_bytes(h, B, T))))
    check(cases, ("posterior", "flow", "generator"))


def test_convert_latent_is_its_head_plus_the_largest_of_spectrogram_posterior_and_flow(ctxs):
    lib, c = ctxs
    cases = []
    for name, shapes in (("default", ((1, 769, 512), (2, 4096, 512))), ("flow_heavy", ((1, 4096, 64), (2, 300, 4))),
                         ("posterior_heavy", ((1, 4096, 64), (2, 300, 4)))):
        h, d = c[name]
        for B, L_max, hop in shapes:
            T = lib.vsp_convert_frames(h, L_max, hop)
            assert T > 0
            n = B * d.inter_channels * T
            head = r256(4 * B * d.gin_channels) + r256(4 * B * d.spec_channels * T) + 5 * r256(4 * n) + r256(8 * B)
            cases.append((lib.vsp_convert_latent_workspace_bytes(h, B, L_max, hop), head,
                          (lib.vsp_spectrogram_ragged_workspace_bytes(h, B, L_max, hop),
                           lib.vsp_posterior_workspace_bytes(h, B, T), lib.vsp_flow_workspace_bytes(h, B, T))))
    check(cases, ("spectrogram", "posterior", "flow"))
