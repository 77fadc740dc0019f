"""ctypes binding of libvispeech_hip.so (include/vispeech_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C vispeech_amd/csrc``.
There is NO fallback: if the shared object is missing or a symbol is absent, importing
callers get an ImportError -- the synthesis path never silently runs on anything else.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VSP_LIB_PATH") or os.path.join(_HERE, "lib", "libvispeech_hip.so")

VSP_MAX_LIST = 8
ABI_VERSION = 7
DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2, "float64": 3}   # VSP_DTYPE_*
PROF_GENERATOR, PROF_ATTENTION, PROF_FRAME = 0, 1, 2
FLAG_NONFINITE_LATENT, FLAG_NONFINITE_WAVE = 1, 2                    # VSP_FLAG_* (vsp_status)

ERRORS = {0: "VSP_OK", -1: "VSP_ERR_ARG", -2: "VSP_ERR_STATE", -3: "VSP_ERR_HIP", -4: "VSP_ERR_KEY",
          -5: "VSP_ERR_SHAPE", -6: "VSP_ERR_WORKSPACE", -7: "VSP_ERR_UNSUPPORTED"}


class VspConfig(C.Structure):
    """``vsp_config`` of include/vispeech_hip.h (field order is ABI)."""
    _fields_ = [
        ("n_vocab", C.c_int32), ("inter_channels", C.c_int32), ("hidden_channels", C.c_int32),
        ("filter_channels", C.c_int32), ("n_heads", C.c_int32), ("n_layers", C.c_int32),
        ("kernel_size", C.c_int32), ("n_resblock_kernels", C.c_int32),
        ("resblock_kernel_sizes", C.c_int32 * VSP_MAX_LIST), ("n_resblock_dilations", C.c_int32),
        ("resblock_dilation_sizes", (C.c_int32 * VSP_MAX_LIST) * VSP_MAX_LIST),
        ("n_upsamples", C.c_int32), ("upsample_rates", C.c_int32 * VSP_MAX_LIST),
        ("upsample_kernel_sizes", C.c_int32 * VSP_MAX_LIST), ("upsample_initial_channel", C.c_int32),
        ("n_speakers", C.c_int32), ("gin_channels", C.c_int32), ("window_size", C.c_int32),
        ("pitch_layers", C.c_int32), ("dur_filter", C.c_int32), ("energy_filter", C.c_int32),
        ("flow_kernel", C.c_int32), ("flow_layers", C.c_int32), ("n_flows", C.c_int32),
        ("spec_channels", C.c_int32), ("posterior_layers", C.c_int32),
    ]


class VspStreamRow(C.Structure):
    """``vsp_stream_row`` of include/vispeech_hip.h: frames [f0, f1) of an utterance of L frames whose latent is
    ``z[c * z_channel_stride + t]`` (device pointer) with the speaker vector ``g`` (device pointer)."""
    _fields_ = [("z", C.c_void_p), ("z_channel_stride", C.c_int64), ("g", C.c_void_p),
                ("L", C.c_int32), ("f0", C.c_int32), ("f1", C.c_int32)]


class VspStreamRowOut(C.Structure):
    """``vsp_stream_row_out``: a row of ``vsp_generator_stream_rows_output`` -- the stream row and the request's two history
    buffers (device pointers to ``vsp_output_history_samples`` floats each; this call reads one and writes the other)."""
    _fields_ = [("row", VspStreamRow), ("hist_in", C.c_void_p), ("hist_out", C.c_void_p)]


class VspRowControl(C.Structure):
    """``vsp_row_control``: one utterance's own scales and which of its controls are given (``GIVEN_*`` bits)."""
    _fields_ = [("duration_scale", C.c_float), ("pitch_scale", C.c_float), ("energy_scale", C.c_float),
                ("noise_scale", C.c_float), ("given", C.c_uint32)]


class VspConvertRow(C.Structure):
    """``vsp_convert_row``: one window of a live conversion -- the samples ``[first_sample, n_known)`` of a recording at
    ``audio`` (device pointer), the frames ``[e0, e1)`` to deliver, the two speakers and the row's noise."""
    _fields_ = [("audio", C.c_void_p), ("first_sample", C.c_int64), ("n_known", C.c_int64), ("closed", C.c_int32),
                ("e0", C.c_int32), ("e1", C.c_int32), ("sid_src", C.c_int64), ("sid_tgt", C.c_int64), ("seed", C.c_uint64),
                ("noise_scale", C.c_float)]


class VspInputRow(C.Structure):
    """``vsp_input_row``: a window ``[in_first, in_first + in_len)`` of one recording at ``in`` (device pointer, raw samples
    in the call's encoding), the recording's length ``n_total`` (-1 while it is open), and the output samples ``[m0, m1)`` to
    write to ``out`` (device pointer, float32), zeros behind them up to ``out_fill``."""
    _fields_ = [("in_", C.c_void_p), ("in_first", C.c_int64), ("in_len", C.c_int64), ("n_total", C.c_int64),
                ("out", C.c_void_p), ("m0", C.c_int64), ("m1", C.c_int64), ("out_fill", C.c_int64)]


IN_F32, IN_S16, IN_ULAW, IN_ALAW = 0, 1, 2, 3                        # VSP_IN_* (vsp_input_rows)
INPUT_RATES_MAX = 8


class VspOutputRow(C.Structure):
    """``vsp_output_row``: the new input samples ``[x_first, x_first + n)`` of one utterance at ``x`` (device pointer,
    float32 at the model's rate), whether it ends there, the row's own output rate and encoding (``VSP_OUT_*``), its two
    history buffers and where its output samples go (``out_fill`` elements of the encoding, silence behind the samples)."""
    _fields_ = [("x", C.c_void_p), ("x_first", C.c_int64), ("n", C.c_int64), ("ended", C.c_int32),
                ("out_rate", C.c_int32), ("enc", C.c_int32), ("hist_in", C.c_void_p), ("hist_out", C.c_void_p),
                ("out", C.c_void_p), ("out_fill", C.c_int64)]


class VspConvForm(C.Structure):
    """``vsp_conv_form``: the kernel a frame-rate convolution launch takes (``CONV_FORM_*``), the tile tuple and flags of
    the throughput kernel, the tap-count / gate instantiation of the channel-split and latency kernels."""
    _fields_ = [("kernel", C.c_int32), ("mt", C.c_int32), ("nt", C.c_int32), ("wm", C.c_int32), ("wn", C.c_int32),
                ("f16s", C.c_int32), ("ring", C.c_int32), ("prune", C.c_int32), ("k", C.c_int32), ("gate", C.c_int32)]


class VspConv1dDesc(C.Structure):
    """``vsp_conv1d_desc`` of ``vsp_conv1d_ex`` (field order is ABI): shape, element strides (0 = dense), device and host
    pointers, prologue, epilogue and path."""
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("K", C.c_int32),
                ("dilation", C.c_int32),
                ("x_bs", C.c_int64), ("x_cs", C.c_int64), ("o_bs", C.c_int64), ("o_cs", C.c_int64), ("r_bs", C.c_int64),
                ("r_cs", C.c_int64), ("o2_bs", C.c_int64), ("o2_cs", C.c_int64),
                ("x", C.c_void_p), ("out", C.c_void_p), ("res", C.c_void_p), ("out2", C.c_void_p), ("lengths", C.c_void_p),
                ("cond", C.c_void_p), ("cond_bs", C.c_int64),
                ("w", C.c_void_p), ("bias", C.c_void_p), ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p),
                ("mask_in", C.c_int32), ("in_act", C.c_int32), ("in_slope", C.c_float),
                ("act", C.c_int32), ("mask_pre", C.c_int32), ("alpha", C.c_float), ("acc_prev", C.c_int32), ("div", C.c_float),
                ("mask_post", C.c_int32), ("split_row", C.c_int32), ("acc_prev2", C.c_int32), ("mask_post2", C.c_int32),
                ("split_f16", C.c_int32), ("cols", C.c_int32), ("ln", C.c_int32), ("plan_only", C.c_int32)]


# VSP_CONV_FORM_* (vsp_conv_form.kernel)
(CONV_FORM_NONE, CONV_FORM_COLS, CONV_FORM_COLS_LN, CONV_FORM_GEMV, CONV_FORM_SPLITK, CONV_FORM_FRAME_SHORT, CONV_FORM_FRAME,
 CONV_FORM_TILE) = range(8)


class VspClLaunchRoute(C.Structure):
    """``vsp_cl_launch_route``: the kernel one launch of a channels-last block takes (``CL_KERNEL_*``), the columns one of
    its tiles stores, g16_conv's row tile, the instantiation."""
    _fields_ = [("kernel", C.c_int32), ("tile_cols", C.c_int32), ("rows", C.c_int32), ("variant", C.c_int32)]


CL_BLOCK_MAX_LAUNCHES = 16


class VspClBlockRoute(C.Structure):
    """``vsp_cl_block_route``: the launches of one ``vsp_cl_block_ex`` call, in order."""
    _fields_ = [("n", C.c_int32), ("launch", VspClLaunchRoute * CL_BLOCK_MAX_LAUNCHES)]


class VspClBlockDesc(C.Structure):
    """``vsp_cl_block_desc`` of ``vsp_cl_block_ex`` (field order is ABI): a ResBlock1 (kind 1) or ResBlock2 (kind 2) on
    channels-last tensors, the accumulate / divide epilogue of its last launch, the ragged batch and the kernel flags."""
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("B", C.c_int32), ("T", C.c_int32), ("C", C.c_int32),
                ("K", C.c_int32), ("n_pairs", C.c_int32), ("terms", C.c_int32),
                ("dilations", C.c_void_p), ("x", C.c_void_p), ("out", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("lengths", C.c_void_p), ("grate", C.c_int32), ("acc_prev", C.c_int32), ("div", C.c_float),
                ("ring", C.c_int32), ("rw64", C.c_int32), ("chain_ring", C.c_int32), ("no_image", C.c_int32),
                ("plan_only", C.c_int32)]


# VSP_CL_KERNEL_* (vsp_cl_launch_route.kernel)
(CL_KERNEL_NONE, CL_KERNEL_CONV, CL_KERNEL_CONV_IMG, CL_KERNEL_PIPE, CL_KERNEL_PAIR, CL_KERNEL_RW, CL_KERNEL_RW64, CL_KERNEL_PP,
 CL_KERNEL_CHAIN, CL_KERNEL_CHAIN_WIDE, CL_KERNEL_RC, CL_KERNEL_RB2, CL_KERNEL_C16, CL_KERNEL_UPS) = range(14)


class VspProsodyParams(C.Structure):
    """``vsp_prosody_params``: pitch floor and ceiling (Hz), voicing threshold, silence threshold, octave cost."""
    _fields_ = [("floor_hz", C.c_float), ("ceiling_hz", C.c_float), ("voicing_threshold", C.c_float),
                ("silence_threshold", C.c_float), ("octave_cost", C.c_float)]


class VspProsodyPathParams(C.Structure):
    """``vsp_prosody_path_params``: octave-jump cost, voiced/unvoiced cost, candidates per frame (the unvoiced one included)."""
    _fields_ = [("octave_jump_cost", C.c_float), ("voiced_unvoiced_cost", C.c_float), ("max_candidates", C.c_int32)]


class VspAlignParams(C.Structure):
    """``vsp_align_params``: the largest advance of a frame (1 or 2), the cost of staying, the cost of skipping a state."""
    _fields_ = [("max_advance", C.c_int32), ("stay_cost", C.c_float), ("skip_cost", C.c_float)]


class VspLoudnessParams(C.Structure):
    """``vsp_loudness_params``: one row's target (LUFS; NaN: leave the row alone), sample-peak ceiling and largest gain (dB)."""
    _fields_ = [("target_lufs", C.c_float), ("peak_ceiling", C.c_float), ("max_gain_db", C.c_float)]


class VspLoudnessLevelParams(C.Structure):
    """``vsp_loudness_level_params``: one row's leveller -- target (LUFS; NaN: leave the row alone), largest gain and cut (dB),
    slew (dB a second) and the gain it starts from (dB)."""
    _fields_ = [("target_lufs", C.c_float), ("max_gain_db", C.c_float), ("max_cut_db", C.c_float), ("slew_db_per_s", C.c_float),
                ("initial_gain_db", C.c_float)]


class VspLoudnessRow(C.Structure):
    """``vsp_loudness_row``: one row (or stream) of the loudness-over-time calls, by pointers of its own; every table starts at
    the row's segment 0."""
    _fields_ = [("seg", C.c_void_p), ("M", C.c_void_p), ("S", C.c_void_p), ("I", C.c_void_p), ("kept", C.c_void_p),
                ("c_db", C.c_void_p), ("c", C.c_void_p), ("first", C.c_int64), ("count", C.c_int64), ("entries", C.c_int64),
                ("inp", C.c_void_p), ("out", C.c_void_p), ("pos", C.c_int64), ("samples", C.c_int64)]


class VspLimiterRow(C.Structure):
    """``vsp_limiter_row``: a stream's samples ``[first, first + count)`` at ``in``, the outputs ``[out_first, out_first +
    out_count)`` at ``out``, the stream's length (-1: unknown yet) and the row's ceiling (NaN: leave the row alone)."""
    _fields_ = [("inp", C.c_void_p), ("first", C.c_int64), ("count", C.c_int64), ("out", C.c_void_p), ("out_first", C.c_int64),
                ("out_count", C.c_int64), ("total", C.c_int64), ("ceiling", C.c_float)]


class VspDenoiseRow(C.Structure):
    """``vsp_denoise_row``: a stream's samples ``[first, first + count)`` at ``in``, the outputs ``[out_first, out_first +
    out_count)`` at ``out``, the stream's length (-1: unknown yet) and the row's strength (NaN: leave the row alone)."""
    _fields_ = [("inp", C.c_void_p), ("first", C.c_int64), ("count", C.c_int64), ("out", C.c_void_p), ("out_first", C.c_int64),
                ("out_count", C.c_int64), ("total", C.c_int64), ("strength", C.c_float)]


LIMITER_MAX_ATTACK, LIMITER_MAX_HOLD, LIMITER_REACH = 1024, 8192, 12   # samples: A, H and the meter's reach J a side
LOUDNESS_FS_MIN, LOUDNESS_FS_MAX = 8000, 192000                      # the sample rates the loudness calls take
LOUDNESS_HIST_BINS = 1000                                            # VSP_LOUDNESS_HIST_BINS
PROSODY_FS, PROSODY_NFFT = 44100, 1280                             # VSP_PROSODY_*
PROSODY_MAX_CANDIDATES, PROSODY_SLOTS = 15, 16                       # VSP_PROSODY_MAX_CANDIDATES; floats of a frame in a table
OUT_F32, OUT_S16, OUT_ULAW, OUT_ALAW = 0, 1, 2, 3                    # VSP_OUT_* (vsp_output_rows)
OUTPUT_RATES_MAX = 8

GIVEN_DURATION, GIVEN_PITCH, GIVEN_ENERGY = 1, 2, 4                  # VSP_GIVEN_* (vsp_set_row_controls)

STREAM_ROWS_MAX = 64

_P = C.c_void_p
_I = C.c_int
_I64 = C.c_int64
_F = C.c_float
_U64 = C.c_uint64

# name -> (restype, argtypes); every symbol include/vispeech_hip.h declares
STFT_TRANSFORMS = {"dft": 0, "fft": 1}      # VSP_STFT_DFT, VSP_STFT_FFT (vsp_set_stft_transform)

SIGNATURES = {
    "vsp_abi_version": (_I, []),
    "vsp_create": (_I, [C.POINTER(VspConfig), _I, C.POINTER(_P)]),
    "vsp_create_ex": (_I, [C.POINTER(VspConfig), C.c_int32, _I, C.POINTER(_P)]),
    "vsp_destroy": (_I, [_P]),
    "vsp_last_error": (C.c_char_p, [_P]),
    "vsp_status": (_I, [_P, C.POINTER(C.c_uint), _I]),
    "vsp_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I]),
    "vsp_set_weight_typed": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _I, _I]),
    "vsp_begin_weights": (_I, [_P]),
    "vsp_missing_weights": (_I, [_P]),
    "vsp_weight_arena_bytes": (_I64, [_P]),
    "vsp_finalize_weights": (_I, [_P, _P]),
    "vsp_adopt_packed_weights": (_I, [_P, _P]),
    "vsp_commit_adopted_weights": (_I, [_P, _P]),
    "vsp_weight_arena": (_I, [_P, C.POINTER(_P), C.POINTER(_I64)]),
    "vsp_encode_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_encode": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _F, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P, _I64]),
    "vsp_frame_lengths_host": (_I, [_P, _P, _I, _P, C.POINTER(_I64), C.POINTER(_I64)]),
    "vsp_decode_workspace_bytes": (_I64, [_P, _I, _I, _I]),
    "vsp_decode": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _U64, _F, _P, _P, _P, _P, _P, _P, _P, _I64]),
    "vsp_infer_workspace_bytes": (_I64, [_P, _I, _I, _I]),
    "vsp_infer": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _F, _F, _F, _P, _U64, _F,
                       _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64]),
    "vsp_attention_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_attention": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I64]),
    "vsp_wn_layer_workspace_bytes": (_I64, [_P, _I, _I, _I]),
    "vsp_wn_layer": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _I64]),
    "vsp_randn": (_I, [_P, _U64, _I64, _P]),
    "vsp_randn_at": (_I, [_P, _U64, _I64, _I64, _P]),
    "vsp_set_noise_offset": (_I, [_P, _I64]),
    "vsp_set_isolated": (_I, [_P, _I]),
    "vsp_get_isolated": (_I, [_P]),
    "vsp_set_noise_seeds": (_I, [_P, C.POINTER(_U64), _I]),
    "vsp_set_row_controls": (_I, [_P, C.POINTER(VspRowControl), _I]),
    "vsp_encoder_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_encoder": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _I64]),
    "vsp_length_regulate": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "vsp_flow_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_flow_reverse": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _I64]),
    "vsp_generator_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_generator": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _I64]),
    "vsp_generator_ragged": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _I64]),
    "vsp_generator_kind": (_I, [_P]),
    "vsp_generator_halo_frames": (_I, [_P]),
    "vsp_generator_frame_dependence": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "vsp_generator_tail_extents": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "vsp_generator_stream_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_generator_stream_chunk": (_I, [_P, _P, _I, _I, _P, _P, _I, _I, _P, _P, _I64]),
    "vsp_stream_rows_plan": (_I, [_P, _I, C.POINTER(VspStreamRow), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32)]),
    "vsp_generator_stream_rows_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_generator_stream_rows": (_I, [_P, _P, _I, C.POINTER(VspStreamRow), _P, _I64, _I, _P, _I64]),
    "vsp_stream_rows_output_plan": (_I, [_I, _I, _I, _I, _I, C.POINTER(VspStreamRow), C.POINTER(_I64), C.POINTER(_I64),
                                         C.POINTER(_I64), C.POINTER(_I64)]),
    "vsp_output_history_samples": (_I, [_I, _I, _I]),
    "vsp_stream_rows_out_samples": (_I64, [_I, _I, _I, _I, _I]),
    "vsp_generator_stream_rows_output": (_I, [_P, _P, _I, C.POINTER(VspStreamRowOut), _P, _I64, _I, _P, _I64]),
    "vsp_flow_forward": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _I64]),
    "vsp_voice_conversion_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_voice_conversion": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64]),
    "vsp_posterior_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_posterior_encoder": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I64]),
    "vsp_has_voice_conversion": (_I, [_P]),
    "vsp_spectrogram_frames": (_I, [_P, _I, _I]),
    "vsp_spectrogram_workspace_bytes": (_I64, [_P, _I, _I, _I]),
    "vsp_spectrogram": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I64]),
    "vsp_convert_frames": (_I, [_P, _I64, _I]),
    "vsp_spectrogram_ragged_workspace_bytes": (_I64, [_P, _I, _I, _I]),
    "vsp_spectrogram_ragged": (_I, [_P, _P, _I, _I, _I, _P, _I64, _P, _P, _P, _P, _I64]),
    "vsp_convert_latent_workspace_bytes": (_I64, [_P, _I, _I, _I]),
    "vsp_convert_latent": (_I, [_P, _P, _I, _I, _I, _P, _I64, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, _I64]),
    "vsp_convert_halo_frames": (_I, [_P]),
    "vsp_convert_window_plan": (_I, [_I, _I, _I, _I64, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I64),
                                     C.POINTER(_I64)]),
    "vsp_convert_stream_rows_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_convert_stream_rows": (_I, [_P, _P, _I, _I, C.POINTER(VspConvertRow), _I, _P, _P, _P, _I64]),
    "vsp_rq_spline": (_I, [_P, _I64, _I, _P, _P, _P, _P, _I, _F, _P, _P]),
    "vsp_mel_filterbank": (_I, [_I, _I, _I, _F, _F, _P]),
    "vsp_spec_to_mel": (_I, [_P, _I, _I, _I, _I, _I, _F, _F, _P, _P]),
    "vsp_cl_conv1d": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _F, _P, _I, _P]),
    "vsp_conv1d": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _F, _I, _P, _I, _I, _P]),
    "vsp_conv1d_ex": (_I, [_P, C.POINTER(VspConv1dDesc), C.POINTER(VspConvForm)]),
    "vsp_cl_resblock": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    "vsp_cl_resblock2": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    "vsp_cl_block_ex": (_I, [_P, C.POINTER(VspClBlockDesc), C.POINTER(VspClBlockRoute)]),
    "vsp_cl_conv_post": (_I, [_P, _I, _I, _I, _I, _P, _P, _F, _F, _P, _I, _P]),
    "vsp_cl_conv_transpose1d": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _F, _P, _I, _P]),
    "vsp_conv_transpose1d": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _F, _P]),
    "vsp_rel_attention": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    "vsp_rel_attention_fused": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    "vsp_resample_plan": (_I, [_I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "vsp_resample_filter": (_I, [_I, _I, _I, C.c_double, C.c_double, _P]),
    "vsp_resample_out_len": (_I64, [_I64, _I, _I]),
    "vsp_output_configure": (_I, [_P, _I, _I, _I, C.c_double, C.c_double]),
    "vsp_output_chunk": (_I, [_P, _P, _I, _P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _P, _I64, _I]),
    "vsp_input_plan": (_I, [_I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "vsp_input_filter": (_I, [_I, _I, _I, C.c_double, C.c_double, _P]),
    "vsp_input_decode_table": (_I, [_I, _P]),
    "vsp_input_configure": (_I, [_P, _I, _I, _I, C.c_double, C.c_double]),
    "vsp_input_rows": (_I, [_P, _P, _I, _I, _I, C.POINTER(VspInputRow)]),
    "vsp_output_encode": (_I, [_I, _P, _I64, _P]),
    "vsp_output_rate_configure": (_I, [_P, _I, _I, _I, C.c_double, C.c_double]),
    "vsp_output_rows_plan": (_I, [_I, _I, _I, _I64, _I64, _I, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64),
                                  C.POINTER(_I64)]),
    "vsp_output_rows": (_I, [_P, _P, _I, C.POINTER(VspOutputRow)]),
    "vsp_prosody_frames": (_I, [_I64, _I]),
    "vsp_prosody_workspace_bytes": (_I64, [_I, _I64, _I, _I, C.POINTER(VspProsodyParams)]),
    "vsp_prosody_contours": (_I, [_P, _P, _I, _I64, _I, _P, _I64, C.POINTER(_I64), C.POINTER(VspProsodyParams), _P, _P, _P,
                                  _P, _I64]),
    "vsp_prosody_phonemes": (_I, [_P, _P, _I, _I, _I, _P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64), _P, _P, _P,
                                  _I64]),
    "vsp_prosody_path_workspace_bytes": (_I64, [_I, _I64, _I, C.POINTER(VspProsodyParams), C.POINTER(VspProsodyPathParams)]),
    "vsp_prosody_candidates": (_I, [_P, _P, _I, _I64, _I, _P, _I64, C.POINTER(_I64), C.POINTER(VspProsodyParams), _I, _P, _P, _P,
                                    _P, _P, _I64]),
    "vsp_prosody_path": (_I, [_P, _P, _I, _I, _I, _P, _P, C.POINTER(_I64), C.POINTER(VspProsodyPathParams), _P, _P, _I64]),
    "vsp_prosody_contours_path": (_I, [_P, _P, _I, _I64, _I, _P, _I64, C.POINTER(_I64), C.POINTER(VspProsodyParams),
                                       C.POINTER(VspProsodyPathParams), _P, _P, _P, _P, _I64]),
    "vsp_align_max_states": (_I, []),
    "vsp_align_scores_workspace_bytes": (_I64, [_I, _I, _I]),
    "vsp_align_path_workspace_bytes": (_I64, [_I, _I, _I]),
    "vsp_align_workspace_bytes": (_I64, [_I, _I, _I, _I]),
    "vsp_align_scores": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, C.POINTER(_I64), C.POINTER(_I64), _P, _P, _I64]),
    "vsp_align_path": (_I, [_P, _P, _I, _I, _I, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(VspAlignParams), _P, _P, _I64]),
    "vsp_align_durations": (_I, [_P, _P, _I, _I, _I, _P, C.POINTER(_I64), C.POINTER(C.c_int32), C.POINTER(_I64), _P, _P, _I64]),
    "vsp_align": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(C.c_int32),
                       C.POINTER(_I64), C.POINTER(VspAlignParams), _P, _P, _P, _I64]),
    "vsp_loudness_kweighting": (_I, [_I, C.POINTER(C.c_double)]),
    "vsp_loudness_segments_count": (_I64, [_I64, _I]),
    "vsp_loudness_workspace_bytes": (_I64, [_I, _I64, _I]),
    "vsp_loudness_segments": (_I, [_P, _P, _I, _I64, _I, _P, _I64, C.POINTER(_I64), _P, _P, _P, _I64]),
    "vsp_loudness_gate": (_I, [_P, _P, _I, _I, _I, _P, C.POINTER(_I64), _P, C.POINTER(VspLoudnessParams), _P, _P, _P, _P, _I64]),
    "vsp_loudness_apply": (_I, [_P, _P, _I, _I64, _P, _I64, _P, _I64, C.POINTER(_I64), _P, C.POINTER(VspLoudnessParams), _P, _I64]),
    "vsp_loudness_normalize": (_I, [_P, _P, _I, _I64, _I, _P, _I64, _P, _I64, C.POINTER(_I64), C.POINTER(VspLoudnessParams), _P, _P,
                                    _P, _P, _P, _I64]),
    "vsp_loudness_time_workspace_bytes": (_I64, [_I, _I64, _I]),
    "vsp_loudness_segments_from": (_I, [_P, _P, _I, _I64, _I, _P, _I64, C.POINTER(_I64), C.POINTER(_I64), _P, _P, _P, _P, _P, _I64]),
    "vsp_loudness_time": (_I, [_P, _P, _I, _I, C.POINTER(VspLoudnessRow), _P, _P, _P, _I64]),
    "vsp_loudness_level_gains": (_I, [_P, _P, _I, C.POINTER(VspLoudnessRow), C.POINTER(VspLoudnessLevelParams), _P, _I64]),
    "vsp_loudness_level_apply": (_I, [_P, _P, _I, _I, C.POINTER(VspLoudnessRow), C.POINTER(VspLoudnessLevelParams), _P, _I64]),
    "vsp_loudness_level": (_I, [_P, _P, _I, _I64, _I, _P, _I64, _P, _I64, C.POINTER(_I64), C.POINTER(VspLoudnessLevelParams), _P, _P, _P,
                                _P, _P, _P, _I64, _P, _P, _P, _P, _P, _I64]),
    "vsp_loudness_hist_tables": (_I, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vsp_loudness_hist_workspace_bytes": (_I64, [_I, _I64, _I]),
    "vsp_loudness_time_hist": (_I, [_P, _P, _I, _I, C.POINTER(VspLoudnessRow), C.POINTER(_P), _P, _P, _P, _P, _I64]),
    "vsp_loudness_range": (_I, [_P, _P, _I, _I64, _I, _P, _I64, C.POINTER(_I64), _P, _P, _P, _P, _P, _P, _I64, _P, _I64]),
    "vsp_true_peak_filter": (_I, [C.POINTER(C.c_float)]),
    "vsp_limiter_history": (_I, [_I, _I, C.POINTER(_I64), C.POINTER(_I64)]),
    "vsp_limiter_workspace_bytes": (_I64, [_I, _I64, _I, _I]),
    "vsp_true_peak": (_I, [_P, _P, _I, _I64, _P, _I64, C.POINTER(_I64), _P, _P, _I64]),
    "vsp_limiter_rows": (_I, [_P, _P, _I, _I, _I, C.POINTER(VspLimiterRow), _P, _P, _P, _I64]),
    "vsp_denoise_workspace_bytes": (_I64, [_P, _I, _I]),
    "vsp_denoise_bias": (_I, [_P, _P, _I, _P, _P, _P, _I64]),
    "vsp_istft": (_I, [_P, _P, _I, _I, _P, C.POINTER(_I64), _P, _I64, _P, _I64]),
    "vsp_denoise": (_I, [_P, _P, _I, _I, _P, _I64, C.POINTER(_I64), _P, C.POINTER(C.c_float), _P, _I64, _P, _I64]),
    "vsp_denoise_history": (_I, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "vsp_denoise_complete": (_I64, [_P, _I64, _I]),
    "vsp_denoise_rows_workspace_bytes": (_I64, [_P, _I, _I64]),
    "vsp_denoise_rows": (_I, [_P, _P, _I, C.POINTER(VspDenoiseRow), _P, _P, _I64]),
    "vsp_set_stft_transform": (_I, [_P, _I]),
    "vsp_stft_transform": (_I, [_P]),
    "vsp_profile_enable": (_I, [_P, _I]),
    "vsp_profile_read": (_I, [_P, C.POINTER(_I64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _I]),
    "vsp_profile_read_class": (_I, [_P, _I, C.POINTER(_I64), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _I]),
    "vsp_profile_read_families": (_I, [_P, _I, _I, C.POINTER(_I), C.POINTER(_I64), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load (once) and type the shared library.  Raises ImportError loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C vispeech_amd/csrc`). There is no CPU fallback for the synthesis path.")
    # One HIP runtime per process: torch ships its own libamdhip64; loaded AFTER a copy this library pulled in from
    # /opt/rocm, the two runtimes do not share a device context ("no ROCm-capable device" at the first hipMemcpy).
    import torch  # noqa: F401
    try:
        l = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise ImportError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(l, name)
        except AttributeError as e:
            raise ImportError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if l.vsp_abi_version() != ABI_VERSION:
        raise ImportError("libvispeech_hip ABI version mismatch")
    _lib = l
    return l


class VspError(RuntimeError):
    pass


def check(rc: int, ctx=None, what: str = "") -> None:
    if rc == 0:
        return
    msg = ""
    if ctx:
        m = lib().vsp_last_error(ctx)
        msg = m.decode("utf-8", "replace") if m else ""
    raise VspError(f"{what or 'libvispeech_hip'}: {ERRORS.get(rc, rc)}: {msg}")


def make_config(dims) -> VspConfig:
    """``vispeech_amd.schema.ModelDims`` -> ``vsp_config``."""
    c = VspConfig()
    c.n_vocab = dims.n_vocab
    c.inter_channels = dims.inter_channels
    c.hidden_channels = dims.hidden_channels
    c.filter_channels = dims.filter_channels
    c.n_heads = dims.n_heads
    c.n_layers = dims.n_layers
    c.kernel_size = dims.kernel_size
    ks = list(dims.resblock_kernel_sizes)
    ds = [list(x) for x in dims.resblock_dilation_sizes]
    if len(ks) > VSP_MAX_LIST or len(ks) != len(ds) or any(len(d) != len(ds[0]) or len(d) > VSP_MAX_LIST for d in ds):
        raise ValueError("resblock lists: at most 8 kernels, equal dilation counts")
    c.n_resblock_kernels = len(ks)
    c.n_resblock_dilations = len(ds[0])
    for i, k in enumerate(ks):
        c.resblock_kernel_sizes[i] = k
        for j, d in enumerate(ds[i]):
            c.resblock_dilation_sizes[i][j] = d
    ur, uk = list(dims.upsample_rates), list(dims.upsample_kernel_sizes)
    if len(ur) != len(uk) or len(ur) > VSP_MAX_LIST:
        raise ValueError("upsample lists: equal length, at most 8")
    c.n_upsamples = len(ur)
    for i, (u, k) in enumerate(zip(ur, uk)):
        c.upsample_rates[i] = u
        c.upsample_kernel_sizes[i] = k
    c.upsample_initial_channel = dims.upsample_initial_channel
    c.n_speakers = dims.n_speakers
    c.gin_channels = dims.gin_channels
    c.window_size = dims.window_size
    c.pitch_layers = dims.pitch_layers
    c.dur_filter = dims.dur_filter
    c.energy_filter = dims.energy_filter
    c.flow_kernel = dims.flow_kernel
    c.flow_layers = dims.flow_layers
    c.n_flows = dims.n_flows
    c.spec_channels = dims.spec_channels
    c.posterior_layers = dims.posterior_layers
    return c
