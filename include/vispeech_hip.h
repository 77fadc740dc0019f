/*
 * vispeech_hip.h -- C-ABI of the MI355X (gfx950) synthesis path.
 *
 * The reference (innnky/vispeech) has NO native/FFI layer: the only boundary its hot path sits
 * behind is the Python method SynthesizerTrn.infer (reference models.py:672-722) and the
 * checkpoint key schema (reference utils.py:21-51, 67-70).  This header is the C boundary a
 * maintainer binds that method to (ctypes stub in INTEGRATION.md; vispeech_amd/models.py is the
 * shipped binding).  Conventions:
 *   - every entry point returns int: 0 = ok, negative = error class (VSP_ERR_*); nothing throws;
 *     vsp_last_error() gives the message of the last failure on that context.
 *   - plain pointers and sizes only.  "dev" pointers are HIP device pointers owned by the CALLER
 *     (torch tensors' data_ptr()); the library owns only its packed weight arena (unless the
 *     caller supplies one) -- no hidden allocation happens on the infer path.
 *   - all work is enqueued on the caller's stream (void* = hipStream_t); the only host
 *     synchronisation is in vsp_frame_lengths_host (the read of the frame counts, which replaces
 *     the B*T_p .item() syncs of reference models.py:398-427).
 *   - activations are float32, laid out [B][C][T] with T contiguous, exactly like the reference's
 *     tensors; a tensor argument is (ptr, batch_stride, channel_stride) in ELEMENTS.
 *   - one context per device; a context is not thread-safe (the reference serialises infer calls
 *     with a lock, inference_api.py:13,37); different contexts are independent.
 */
#ifndef VISPEECH_HIP_H
#define VISPEECH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6 (round 5): no entry point changed, but (a) the PACKED WEIGHT ARENA holds the split-f16 convolutions' weights and biases
 * scaled by 2^8 with unscaled lo parts (one fp32 accumulator per tile) -- an arena packed by an ABI-5 library must not be
 * adopted (vsp_commit_adopted_weights checks this number in the arena header) -- and (b) vsp_frame_lengths_host no longer
 * implies a full stream synchronisation after a vsp_encode with given durations (see there). */
/* 7 (round 6): (a) vsp_status -- sticky numeric-range flags raised by the kernels (see there); (b) the generator's
 * activations are carried * 2^VSP_ACT_SCALE_LOG2 between conv_pre and conv_post and the packed generator biases carry that
 * factor: an arena packed by an ABI-6 library (or under another VSP_ACT_SCALE_LOG2: the arena's configuration hash covers it)
 * must not be adopted; (c) vsp_profile_read_class / vsp_profile_read_families return one more figure per class / family, the
 * bytes a launch moves AS FUSED (a new trailing out-parameter each: callers of ABI <= 6 must be rebuilt); (d) vsp_conv1d
 * accepts split_f16 = 2 (the column-tile kernel as a stand-alone operator). */
#define VSP_ABI_VERSION 7

enum {
  VSP_OK = 0,
  VSP_ERR_ARG = -1,        /* null / out-of-range argument */
  VSP_ERR_STATE = -2,      /* call order (weights not finalised, ...) */
  VSP_ERR_HIP = -3,        /* a HIP runtime call failed */
  VSP_ERR_KEY = -4,        /* unknown state_dict key */
  VSP_ERR_SHAPE = -5,      /* tensor shape differs from the schema */
  VSP_ERR_WORKSPACE = -6,  /* workspace too small */
  VSP_ERR_UNSUPPORTED = -7 /* configuration outside what the kernels cover */
};

#define VSP_MAX_LIST 8

/* Hyper-parameters that fix tensor shapes: the constructor arguments of the reference's
 * SynthesizerTrn (models.py:537-561) plus the constants its code hard-wires
 * (attentions.py:14 window 4; models.py:498 6 pitch layers; :599 duration filter 256;
 * frame_prior_network.py:65 energy filter 768; models.py:597 WN kernel 5 / 4 layers; :184 4 flows). */
typedef struct vsp_config {
  int32_t n_vocab;
  int32_t inter_channels;
  int32_t hidden_channels;
  int32_t filter_channels;
  int32_t n_heads;
  int32_t n_layers;
  int32_t kernel_size;
  int32_t n_resblock_kernels;
  int32_t resblock_kernel_sizes[VSP_MAX_LIST];
  int32_t n_resblock_dilations;                       /* dilations per ResBlock1 (3) */
  int32_t resblock_dilation_sizes[VSP_MAX_LIST][VSP_MAX_LIST];
  int32_t n_upsamples;
  int32_t upsample_rates[VSP_MAX_LIST];
  int32_t upsample_kernel_sizes[VSP_MAX_LIST];
  int32_t upsample_initial_channel;
  int32_t n_speakers;
  int32_t gin_channels;
  int32_t window_size;
  int32_t pitch_layers;
  int32_t dur_filter;
  int32_t energy_filter;
  int32_t flow_kernel;
  int32_t flow_layers;
  int32_t n_flows;
  /* voice conversion only (ABI 2): input channels of the posterior encoder = filter_length/2+1
   * (reference models.py:596) and its WN depth (16, models.py:596).  spec_channels == 0 builds a
   * context without the posterior encoder (enc_q.* tensors are then accepted and ignored). */
  int32_t spec_channels;
  int32_t posterior_layers;
} vsp_config;

typedef struct vsp_ctx vsp_ctx;

/* ---- lifetime --------------------------------------------------------------------------- */
int vsp_abi_version(void);
/* Replaces SynthesizerTrn.__init__ (reference models.py:537-622) for the infer path. */
int vsp_create(const vsp_config* cfg, int device, vsp_ctx** out);
/* vsp_create_ex (round 7, ABI 7, additive): the same with the generator's ResBlock kind, the reference's `resblock`
 * constructor argument (models.py:251): 1 = ResBlock1 (modules.py:187-229), 2 = ResBlock2 (modules.py:232-256: two
 * convolutions per block, dilation[0] and dilation[1] of each resblock_dilation_sizes row; state_dict keys
 * dec.resblocks.N.convs.{0,1}.*).  vsp_create(cfg, ...) is vsp_create_ex(cfg, 1, ...); any other kind returns
 * VSP_ERR_ARG, and so does kind 2 with n_resblock_dilations < 2.  The packed arena's configuration hash covers kind 2:
 * a context of one kind refuses the other kind's arena in vsp_commit_adopted_weights.  VSP_RB2_FUSE=0 (read here) runs
 * every ResBlock2 convolution as a launch of its own (second implementation, bit-identical). */
int vsp_create_ex(const vsp_config* cfg, int32_t resblock, int device, vsp_ctx** out);
int vsp_destroy(vsp_ctx* ctx);
const char* vsp_last_error(const vsp_ctx* ctx);

/* Sticky numeric-range flags (ABI 7).  The matrix kernels multiply fp32 activations as f16 hi / lo pairs: an activation
 * beyond the f16 range (|x| > 65504; inside the generator |x| > 65504 / 2^VSP_ACT_SCALE_LOG2 = 4094 by default) cannot be
 * split.  It becomes +-inf in the operand (round 5 clamped it silently), so the affected outputs are inf / NaN rather than
 * plausible wrong numbers, and the last kernels of each half raise a flag in a host-visible word of the context:
 *   VSP_FLAG_NONFINITE_LATENT  z_p = m_p + noise * exp(logs_p) * noise_scale is not finite somewhere (phoneme- / frame-rate half)
 *   VSP_FLAG_NONFINITE_WAVE    a waveform sample's pre-tanh sum is not finite (flow or generator)
 * vsp_status copies the word to *flags (no stream synchronisation: it reflects the launches that have COMPLETED; synchronise
 * the stream first for a definitive answer) and clears it when `clear` != 0.  Weights outside the packed range are refused at
 * load time (vsp_finalize_weights); this is the same loudness for activations.  The reference's fp32 path has no such limit.
 * Precision floor of the split, in terms of OUTPUT level: with the default activation scale the waveform stays within
 * 1e-4 * max|o| of the fp32 reference down to a peak level of about -90 dBFS (tests/test_amplitude_floor.py measures it;
 * VSP_ACT_SCALE_LOG2=0, round 5's behaviour, crosses that bound near -68 dBFS). */
#define VSP_FLAG_NONFINITE_LATENT 1u
#define VSP_FLAG_NONFINITE_WAVE 2u
int vsp_status(vsp_ctx* ctx, unsigned* flags, int clear);

/* ---- weights: replaces load_state_dict / utils.load_checkpoint (reference utils.py:21-51) - */
/* One call per state_dict tensor, raw reference keys ("dec.ups.0.weight_v", ...), float32 HOST
 * data (copied).  weight_g/weight_v pairs are folded by vsp_finalize_weights exactly as
 * torch.nn.utils.weight_norm does (reference modules.py:128,135,145,191-206; models.py:255: for
 * ConvTranspose1d the norm is per INPUT channel).  Keys that infer never reads (enc_q.*,
 * enc_p.proj.*, frame_prior_net.emb.*, energy_predictor.predictor.proj.*) are accepted and
 * ignored; unknown keys return VSP_ERR_KEY. */
int vsp_set_weight(vsp_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim);
/* The same for a checkpoint held in another type or on the device (ABI 3; SURVEY 8b's contract): dtype is one of
 * VSP_DTYPE_*, on_device != 0 means `data` is a HIP device pointer (copied to the host first).  Values are
 * widened to float32 exactly (f16 / bf16) or rounded once (f64). */
#define VSP_DTYPE_F32 0
#define VSP_DTYPE_F16 1
#define VSP_DTYPE_BF16 2
#define VSP_DTYPE_F64 3
int vsp_set_weight_typed(vsp_ctx* ctx, const char* key, const void* data, const int64_t* shape, int ndim, int dtype,
                         int on_device);
/* Forget every tensor set so far (start of a new load on a context that was loaded before).  Within one load,
 * setting "<x>.weight" drops an earlier "<x>.weight_g" / "<x>.weight_v" pair and vice versa. */
int vsp_begin_weights(vsp_ctx* ctx);
/* Number of infer-path tensors still missing (0 = ready to finalise). */
int vsp_missing_weights(const vsp_ctx* ctx);
/* Size of the packed device arena (depends on the config only). */
int64_t vsp_weight_arena_bytes(const vsp_ctx* ctx);
/* Fold + pack (MFMA fragment order) + upload.  dev_arena may be NULL (the library allocates).  VSP_ERR_STATE while a
 * required tensor is missing; VSP_ERR_UNSUPPORTED when a folded convolution weight does not fit the packed split-f16 form
 * (|w| < 253: the images hold w * 2^8 as f16 pairs -- ABI 6).  Both this call and vsp_commit_adopted_weights then build
 * the context's per-speaker silence table (vsp_generator_tail_extents) on the device and return when it is finished; a
 * table that cannot be built (memory) is not an error: the generator then runs without one. */
int vsp_finalize_weights(vsp_ctx* ctx, void* dev_arena);
/* Multi-GPU: a non-root rank adopts an arena that receives rank 0's packed bytes by an RCCL broadcast; no host
 * weights needed.  vsp_adopt_packed_weights only records the pointer (the bytes may still be in flight): the context
 * is NOT ready until vsp_commit_adopted_weights, called after the broadcast has completed, has read the arena's
 * header (one small device-to-host copy + stream sync) and checked magic, ABI version, size and configuration hash.
 * What rank 0 packed travels in that header -- in particular whether the posterior encoder (voice conversion) is
 * there -- instead of being inferred from the local config. */
int vsp_adopt_packed_weights(vsp_ctx* ctx, void* dev_arena);
int vsp_commit_adopted_weights(vsp_ctx* ctx, void* stream);
/* The arena this context reads its weights from (for the broadcast on rank 0). */
int vsp_weight_arena(const vsp_ctx* ctx, void** dev_arena, int64_t* bytes);

/* ---- the path: replaces SynthesizerTrn.infer (reference models.py:672-722) ---------------- */
/* Phoneme-rate half, models.py:674-708 + the prefix sum of LengthRegulator (models.py:398-427):
 *   speaker embedding, TextEncoder, duration / F0 / energy (predicted, or the *_ctl tensor when
 *   non-NULL -- the reference's isinstance(.., torch.Tensor) branches), pitch/energy prenets.
 * Inputs (device): phonemes[B*Tp] int64, lengths[B] int64, sid[B] int64; *_ctl [B*Tp] float or NULL
 *   with the scalar controls used instead (reference defaults 1.0).  With a row table (vsp_set_row_controls, isolated
 *   mode) the choice and the scale are row b's own and the three scalar arguments are not read.
 * Outputs (device): x_var [B][H][Tp] (text encoding + prenets, the length regulator's input),
 *   g [B][gin], duration/f0/energy [B*Tp], frame_lengths[B] int64, cum_dur [B*Tp] int32.
 * workspace: >= vsp_encode_workspace_bytes(ctx,B,Tp). */
int64_t vsp_encode_workspace_bytes(const vsp_ctx* ctx, int B, int Tp);
int vsp_encode(vsp_ctx* ctx, void* stream, int B, int Tp,
               const int64_t* phonemes, const int64_t* lengths, const int64_t* sid,
               const float* duration_ctl, const float* pitch_ctl, const float* energy_ctl,
               float duration_scale, float pitch_scale, float energy_scale,
               float* x_var, float* g, float* duration, float* f0, float* energy,
               int64_t* frame_lengths, int32_t* cum_dur,
               void* workspace, int64_t workspace_bytes);
/* Copies frame_lengths[B] to the host and returns max(frame_lengths): the one host wait of an infer call.  After a
 * vsp_encode with duration_ctl != NULL (given durations: the counts depend on nothing vsp_encode computes) it waits only
 * for the copy vsp_encode started before its first launch -- the text encoder may still be running on the stream when it
 * returns, and vsp_decode enqueued behind it finds no idle GPU between the two halves; otherwise (predicted durations,
 * or a frame_lengths_dev that is not the last vsp_encode's) it is a copy + one stream synchronisation.  The pinned
 * B x int64 host buffer and the event behind this are created by the first such vsp_encode and kept with the context. */
int vsp_frame_lengths_host(vsp_ctx* ctx, void* stream, int B, const int64_t* frame_lengths_dev,
                           int64_t* frame_lengths_host, int64_t* max_frames);

/* Frame-rate half, models.py:711-720: length-regulator expand, FramePriorNet, Projection +
 * reparameterisation with the caller's noise (models.py:718), inverse flow, HiFi-GAN generator.
 * Tf = padded frame count of the batch (>= every frame length; the GLOBAL maximum in a sharded
 * run, SURVEY gotcha G6).  max_len < 0 = no truncation; the generator consumes
 * Tdec = min(Tf, max_len) frames and writes o[B][1][Tdec * prod(upsample_rates)].
 * noise [B][inter][Tf], or NULL: then the library draws it on the device -- vsp_randn(noise_seed) over the same
 * [B][inter][Tf] elements (ABI 4; the torch.randn_like(m_p) of models.py:718 for callers without a generator.  It is a
 * Philox4x32-10 stream of its own, NOT bit-compatible with torch.manual_seed(noise_seed); pass the tensor to
 * reproduce a torch run).  noise_seed is ignored when noise != NULL or noise_scale == 0.  With a row table
 * (vsp_set_row_controls) row b's noise_scale replaces the argument, and noise is drawn iff some row's is non-zero.
 * Outputs (device, contiguous): o, x_mask[B*Tf] uint8, z, z_p, m_p, logs_p [B][inter][Tf]. */
int64_t vsp_decode_workspace_bytes(const vsp_ctx* ctx, int B, int Tp, int Tf);
int vsp_decode(vsp_ctx* ctx, void* stream, int B, int Tp, int Tf, int max_len,
               const float* x_var, const float* g, const int32_t* cum_dur, const int64_t* frame_lengths,
               const float* noise, uint64_t noise_seed, float noise_scale,
               float* o, uint8_t* x_mask, float* z, float* z_p, float* m_p, float* logs_p,
               void* workspace, int64_t workspace_bytes);

/* One-call form of the path for callers that know an upper bound of the frame count up front (supplied
 * durations, or a fixed max_len): vsp_encode + vsp_decode with Tf = tf_pad and NO host synchronisation.
 * tf_pad must be >= every utterance's frame count (frames past it are cut off; frame_lengths is returned
 * so the caller can check afterwards).  Arguments as in vsp_encode / vsp_decode; workspace >=
 * vsp_infer_workspace_bytes(ctx, B, Tp, tf_pad). */
int64_t vsp_infer_workspace_bytes(const vsp_ctx* ctx, int B, int Tp, int tf_pad);
int vsp_infer(vsp_ctx* ctx, void* stream, int B, int Tp, int tf_pad, int max_len,
              const int64_t* phonemes, const int64_t* lengths, const int64_t* sid,
              const float* duration_ctl, const float* pitch_ctl, const float* energy_ctl,
              float duration_scale, float pitch_scale, float energy_scale,
              const float* noise, uint64_t noise_seed, float noise_scale,
              float* o, uint8_t* x_mask, float* z, float* z_p, float* m_p, float* logs_p,
              float* duration, float* f0, float* energy, int64_t* frame_lengths,
              void* workspace, int64_t workspace_bytes);

/* ---- per-stage entry points (unit parity against the oracle) ------------------------------ */
/* MultiHeadAttention.attention (reference attentions.py:148-179 with the relative-position helpers
 * :181-243) of layer `layer` of encoder `which` (0 enc_p.encoder, 1 pitch_predictor.pitch_net,
 * 2 frame_prior_net.fft_block): qkv [B][3H][T] = conv_q | conv_k | conv_v outputs, lengths[B] (attn_mask =
 * mask x mask), out [B][H][T] = the tensor conv_o consumes.  workspace >= vsp_attention_workspace_bytes (the packed
 * f16 operand images; ABI 4: caller-owned like every other workspace -- no allocation behind the ABI).
 * Operand range of the default (split-f16) kernel: q, k, v are packed as f16 hi / lo pairs with fixed power-of-two
 * scales (q * 128 log2(e) / sqrt(d_k), k * 16, v * 16); magnitudes beyond |q| ~ 3.4e3, |k|, |v| ~ 4.0e3 are CLAMPED
 * to the largest finite f16 (the fp32 reference stays exact there; layer-normed encoder activations are O(1..10)).
 * VSP_ATT=f32 selects the f32 kernel, which has no such limit. */
int64_t vsp_attention_workspace_bytes(const vsp_ctx* ctx, int B, int T);
int vsp_attention(vsp_ctx* ctx, void* stream, int which, int layer, int B, int T, const float* qkv,
                  const int64_t* lengths, float* out, void* workspace, int64_t workspace_bytes);
/* attentions.Encoder.forward (reference attentions.py:35-47). which: 0 = enc_p.encoder,
 * 1 = pitch_predictor.pitch_net, 2 = frame_prior_net.fft_block.  x [B][H][T] in, y [B][H][T] out. */
int64_t vsp_encoder_workspace_bytes(const vsp_ctx* ctx, int B, int T);
int vsp_encoder(vsp_ctx* ctx, void* stream, int which, int B, int T, const float* x,
                const int64_t* lengths, float* y, void* workspace, int64_t workspace_bytes);
/* LengthRegulator (reference models.py:398-427) from a ready prefix sum. */
int vsp_length_regulate(vsp_ctx* ctx, void* stream, int B, int C, int Tp, int Tf, const float* x,
                        const int32_t* cum_dur, float* x_frame);
/* ResidualCouplingBlock.forward(reverse=True) (reference models.py:202-209). z_p -> z, in place
 * semantics on a copy: z is written, z_p is read. */
int64_t vsp_flow_workspace_bytes(const vsp_ctx* ctx, int B, int Tf);
int vsp_flow_reverse(vsp_ctx* ctx, void* stream, int B, int Tf, const float* z_p, const float* g,
                     const int64_t* frame_lengths, float* z, void* workspace, int64_t workspace_bytes);
/* One layer of modules.WN.forward (reference modules.py:148-176, dilation_rate 1; the gate is
 * commons.fused_add_tanh_sigmoid_multiply, commons.py:100-107):
 *   a = in_layers[layer](x) + cond_layer(g)[layer * 2h : (layer + 1) * 2h];  acts = tanh(a[:h]) * sigmoid(a[h:])
 *   rs = res_skip_layers[layer](acts)
 *   layer < n - 1:  x = (x + rs[:h]) * mask;  skip (+)= rs[h:]
 *   layer == n - 1: skip = (skip (+) rs) * mask        (the `output * x_mask` of modules.py:176 is folded in)
 * which: 0 .. n_flows-1 = flow.flows[2 * which].enc, -1 = enc_q.enc (needs the posterior-encoder weights).
 * x [B][h][T] is updated in place; skip [B][h][T] is accumulated into when accumulate != 0, else overwritten;
 * g [B][gin]; lengths [B]. */
int64_t vsp_wn_layer_workspace_bytes(const vsp_ctx* ctx, int which, int B, int T);
int vsp_wn_layer(vsp_ctx* ctx, void* stream, int which, int layer, int B, int T, float* x, const float* g,
                 const int64_t* lengths, float* skip, int accumulate, void* workspace, int64_t workspace_bytes);
/* Generator.forward (reference models.py:271-290). z [B][inter][T] (already masked/truncated). */
int64_t vsp_generator_workspace_bytes(const vsp_ctx* ctx, int B, int T);
/* Which generator this context runs (ABI 7, additive): 0 the channel-major f32 kernels -- asked for with
 * VSP_GENERATOR=f32, or because a stage's channel count is outside the channels-last kernels' cover (32, multiples of
 * 64, and a last stage of 16 reached from 32); 1 the split-f16 channels-last kernels; 2 the same with plain f16 operands
 * (VSP_GENERATOR=f16).  Valid once the context exists. */
int vsp_generator_kind(const vsp_ctx* ctx);
int vsp_generator(vsp_ctx* ctx, void* stream, int B, int T, const float* z, const float* g,
                  float* o, void* workspace, int64_t workspace_bytes);
/* The generator with per-utterance ends (ABI 7, additive; round 10): utterance b's waveform samples [0, L_b * up),
 * L_b = min(lengths[b], T), up = prod(upsample_rates), are what vsp_generator returns for a B = 1 call on z[b][:, :L_b] -- its
 * tensors END at L_b in every stage, whatever z holds behind L_b and whoever shares the batch -- and o is exactly 0.0 behind
 * them.  lengths [B] int64 on the device (< 1: the whole row is zero).  Workspace: vsp_generator_workspace_bytes + B *
 * sizeof(int) bytes (an upper bound kept for callers' arithmetic: vsp_generator_workspace_bytes itself holds the per-utterance
 * plan, so the extra ints are not touched).  It is the generator call vsp_decode / vsp_infer / vsp_voice_conversion make in isolated mode. */
int vsp_generator_ragged(vsp_ctx* ctx, void* stream, int B, int T, const float* z, const float* g,
                         const int64_t* lengths, float* o, void* workspace, int64_t workspace_bytes);

/* Streamed vocoder (BASELINE config 5; the chunked output loop of reference inference_api.py:50-60 applied to the
 * vocoder itself): the waveform samples of frames [f0, f1) of z [B][inter][T], computed from those frames plus
 * vsp_generator_halo_frames() frames on each side -- bit-identical to the same samples of one vsp_generator call.
 * o_chunk [B][1][(f1 - f0) * prod(upsample_rates)] contiguous; workspace >= vsp_generator_stream_workspace_bytes
 * for the largest f1 - f0 used. */
int vsp_generator_halo_frames(const vsp_ctx* ctx);
/* ABI 5: the SAMPLE-EXACT dependence of the vocoder's output frames on its input frames, from the configuration's kernel
 * sizes, strides and dilations: output frame F depends on input frames [F - *back, F + *fwd] (13 / 13 for
 * configs/config.json; the halo above is the coarser per-stage bound).  It is what the trimmed tails of a ragged batch
 * rest on (VSP_TRIM_TAILS): an utterance of L frames is computed to L + back + 1 + fwd frames -- frames [0, L + back) as in
 * the padded run, frame L + back the steady state of the zero input behind the utterance (periodic in one frame), the
 * last fwd frames the tensor end's -- and the rest of the padded waveform is filled from those, bit for bit. */
int vsp_generator_frame_dependence(const vsp_ctx* ctx, int* back, int* fwd);
/* The same two extents and *reach1: output frame F depends on frames up to F + *reach1 of the FIRST stage's output tensor
 * (the second up-convolution through conv_post; 2 for configs/config.json, *fwd + 1 for a generator of one stage).  An
 * utterance whose speaker vector is a row of emb_g takes its steady-state frame and the tensor end's frames from the
 * context's per-speaker silence table (built when weights are committed; VSP_TAIL_TABLE=0: none), so the stages behind
 * the first compute it to L + back + reach1 frames only, where L + back + fwd <= T.  Additive; needs no weights. */
int vsp_generator_tail_extents(const vsp_ctx* ctx, int* back, int* fwd, int* reach1);
int64_t vsp_generator_stream_workspace_bytes(const vsp_ctx* ctx, int B, int chunk_frames);
int vsp_generator_stream_chunk(vsp_ctx* ctx, void* stream, int B, int T, const float* z, const float* g, int f0, int f1,
                               float* o_chunk, void* workspace, int64_t workspace_bytes);

/* Streaming for batched requests (ABI 7, additive; round 11): ONE set of generator launches advances up to 64 requests by one
 * chunk each, every request at its own position of its own utterance.  Row b is frames [f0, f1) of an utterance of L frames
 * whose latent is z[c * z_channel_stride + t], c < inter_channels, t < L (a DEVICE pointer: rows may point into different
 * tensors); g is its speaker vector, gin_channels floats on the device.  The row's window is lo = max(0, f0 - halo),
 * hi = min(L, f1 + halo), halo = vsp_generator_halo_frames().  The rows array itself is HOST memory, read before the call
 * returns; it reaches the device as a kernel argument.
 *
 * vsp_generator_stream_rows writes to out[b][0 .. (f1 - f0) * up), up = prod(upsample_rates), the waveform samples
 * [f0 * up, f1 * up) of what vsp_generator_ragged returns for a B = 1 call on z[:, :L] -- to the tolerance between two launch
 * shapes of this library, not bit for bit: kernels are chosen by launch size -- as float32 (pcm == 0) or as int16 by the rule of
 * vsp_output_chunk (pcm == 1); the rest of the row, out[b][(f1 - f0) * up .. out_stride), is exactly 0.  out [B][out_stride],
 * out_stride in ELEMENTS; chunk_frames = out_stride / up is the longest chunk the call accepts.  How: one gather launch packs
 * every row's z[:, lo:hi) (zero behind it), g and hi - lo; the generator runs on the packed tensor with per-utterance ends as
 * in vsp_generator_ragged, so a row's tensors end at hi - lo in every stage -- the utterance's true end where hi == L, else an
 * artificial end a full halo behind the last delivered frame, and the same on the left; one collect launch cuts, quantises
 * and zero-fills.  No allocation, no synchronisation, everything on the caller's stream.
 * Arguments, checked on the host before anything is launched: 1 <= B <= 64, 0 <= f0 < f1 <= L, f1 - f0 <= chunk_frames, z and
 * g non-NULL, z_channel_stride >= L, pcm 0 or 1: VSP_ERR_ARG otherwise.  Workspace: vsp_generator_stream_rows_workspace_bytes
 * for any chunk_frames >= the call's out_stride / up (VSP_ERR_WORKSPACE if too small): vsp_generator_workspace_bytes(B,
 * chunk_frames + 2 halo) plus the packed z, the g rows, the lengths and the span waveform, each rounded to 256 bytes.
 * vsp_stream_rows_plan is the same host arithmetic without a device (z and g are not read): lo[b], hi[b] (each may be NULL)
 * and *span_max = max(hi - lo) (may be NULL); it checks B and every row's 0 <= f0 < f1 <= L. */
typedef struct vsp_stream_row {
  const float* z;
  int64_t z_channel_stride;
  const float* g;
  int32_t L, f0, f1;
} vsp_stream_row;
int vsp_stream_rows_plan(const vsp_ctx* ctx, int B, const vsp_stream_row* rows, int32_t* lo, int32_t* hi, int32_t* span_max);
int64_t vsp_generator_stream_rows_workspace_bytes(const vsp_ctx* ctx, int B, int chunk_frames);
int vsp_generator_stream_rows(vsp_ctx* ctx, void* stream, int B, const vsp_stream_row* rows, void* out, int64_t out_stride,
                              int pcm, void* workspace, int64_t workspace_bytes);

/* ---- voice conversion: replaces SynthesizerTrn.voice_conversion (reference models.py:724-732) */
/* Needs cfg.spec_channels > 0 and every enc_q.* tensor set before vsp_finalize_weights
 * (VSP_ERR_STATE otherwise).  y [B][spec][T] linear spectrogram, y_lengths[B], sid_src/sid_tgt[B]
 * int64, noise [B][inter][T] (the torch.randn_like of models.py:230).  Outputs (device,
 * contiguous): o_hat [B][1][T*prod(upsample_rates)], y_mask [B*T] uint8, z / z_p / z_hat
 * [B][inter][T]; m_q / logs_q [B][inter][T] may be NULL. */
int64_t vsp_voice_conversion_workspace_bytes(const vsp_ctx* ctx, int B, int T);
int vsp_voice_conversion(vsp_ctx* ctx, void* stream, int B, int T, const float* y, const int64_t* y_lengths,
                         const int64_t* sid_src, const int64_t* sid_tgt, const float* noise,
                         float* o_hat, uint8_t* y_mask, float* z, float* z_p, float* z_hat,
                         float* m_q, float* logs_q, void* workspace, int64_t workspace_bytes);
/* PosteriorEncoder.forward (reference models.py:212-241): y, lengths, g [B][gin], noise -> z, m, logs. */
int64_t vsp_posterior_workspace_bytes(const vsp_ctx* ctx, int B, int T);
int vsp_posterior_encoder(vsp_ctx* ctx, void* stream, int B, int T, const float* y, const int64_t* y_lengths,
                          const float* g, const float* noise, float* z, float* m, float* logs,
                          void* workspace, int64_t workspace_bytes);
/* ResidualCouplingBlock.forward(reverse=False) (reference models.py:202-206). z -> z_p. */
int vsp_flow_forward(vsp_ctx* ctx, void* stream, int B, int Tf, const float* z, const float* g,
                     const int64_t* frame_lengths, float* z_p, void* workspace, int64_t workspace_bytes);
/* Linear spectrogram of mel_processing.spectrogram_torch (reference mel_processing.py:50-69), the input of
 * voice_conversion: reflect-pad (n_fft - hop)/2 on both sides, periodic Hann window of n_fft, one-sided DFT
 * (n_fft = 2 * (cfg.spec_channels - 1)), magnitude sqrt(re^2 + im^2 + 1e-6).  audio [B][L] (device),
 * spec [B][spec_channels][T] with T = vsp_spectrogram_frames(L, hop); needs cfg.spec_channels > 0. */
int vsp_spectrogram_frames(const vsp_ctx* ctx, int L, int hop);
int64_t vsp_spectrogram_workspace_bytes(const vsp_ctx* ctx, int B, int L, int hop);
int vsp_spectrogram(vsp_ctx* ctx, void* stream, int B, int L, int hop, const float* audio, float* spec,
                    void* workspace, int64_t workspace_bytes);
/* 1 if the posterior-encoder weights are loaded (voice conversion available), else 0. */
int vsp_has_voice_conversion(const vsp_ctx* ctx);

/* ---- conversion from audio: recordings of different lengths in one batch (additive, ABI 7) */
/* Frames of a recording of n_samples samples, host arithmetic only: with n_fft = 2 * (cfg.spec_channels - 1) and
 * pad = (n_fft - hop) / 2, T(n) = 0 where n <= pad (the reflect padding is undefined) or n + 2 pad < n_fft (no full
 * window), else 1 + (n + 2 pad - n_fft) / hop.  NOT vsp_spectrogram_frames: that one refuses n <= pad and, for
 * n_fft < 3 hop, counts a frame where the padded signal is shorter than a window.  VSP_ERR_ARG: n_samples < 0, hop <= 0,
 * n_fft < hop, or a context without spec_channels. */
int vsp_convert_frames(const vsp_ctx* ctx, int64_t n_samples, int hop);
/* Linear spectrogram of B recordings of different lengths: audio [B][audio_stride] (device, audio_stride >= L_max),
 * n_samples [B] (device, clamped to [0, L_max]).  spec [B][spec_channels][T_max], T_max = vsp_convert_frames(L_max) > 0:
 * row b's columns [0, T(n_b)) are what vsp_spectrogram returns for audio[b][0 .. n_b) alone (the reflect padding is around
 * the row's own two ends), columns [T(n_b), T_max) are exactly 0.0, and frames[b] (device out) = T(n_b).  A sample at or
 * behind n_b is never read: what a padded buffer holds there cannot reach an output.  The host does not read n_samples:
 * grids and shape checks use L_max (the n_valid / n_max convention of vsp_output_chunk).  No allocation, no
 * synchronisation, caller's stream; the DFT is the convolution vsp_spectrogram runs. */
int64_t vsp_spectrogram_ragged_workspace_bytes(const vsp_ctx* ctx, int B, int L_max, int hop);
int vsp_spectrogram_ragged(vsp_ctx* ctx, void* stream, int B, int L_max, int hop, const float* audio, int64_t audio_stride,
                           const int64_t* n_samples, float* spec, int64_t* frames, void* workspace, int64_t workspace_bytes);
/* Audio to the converted latent in one call: ragged spectrogram, posterior encoder and forward flow with emb_g(sid_src),
 * reverse flow with emb_g(sid_tgt) -- voice_conversion (reference models.py:724-732) without its generator, the counterpart
 * of vsp_decode(max_len = 0).  Row b, restricted to T(n_b) frames, is what the reference computes up to z_hat for a B = 1
 * call on spectrogram_torch(audio[b][:n_b]); every float output is exactly 0 behind the row's extent.  Outputs (device,
 * contiguous): z_hat [B][inter][T_max], g_tgt [B][gin] (the row's speaker vector, for a generator call), frames [B],
 * y_mask [B*T_max] uint8; z / z_p [B][inter][T_max] may be NULL.  noise [B][inter][T_max]: row b uses noise[b][:, :T(n_b)];
 * NULL: row b's tensor is the first inter * T(n_b) elements of the Philox stream keyed seeds[b], laid out [inter][T(n_b)]
 * (vsp_set_noise_seeds for exactly B rows first, VSP_ERR_STATE otherwise).  noise_scale multiplies the posterior's noise,
 * z = m_q + noise * exp(logs_q) * noise_scale: 1.0 is the reference; with 0 nothing is drawn or read, no seeds are needed and
 * z = m_q.  The isolated flag of the context is neither read nor changed (these stages mask by length already).  Needs the
 * enc_q.* tensors (VSP_ERR_STATE otherwise).  No allocation, no synchronisation. */
int64_t vsp_convert_latent_workspace_bytes(const vsp_ctx* ctx, int B, int L_max, int hop);
int vsp_convert_latent(vsp_ctx* ctx, void* stream, int B, int L_max, int hop, const float* audio, int64_t audio_stride,
                       const int64_t* n_samples, const int64_t* sid_src, const int64_t* sid_tgt, const float* noise,
                       float noise_scale, float* z_hat, float* g_tgt, int64_t* frames, uint8_t* y_mask, float* z, float* z_p,
                       void* workspace, int64_t workspace_bytes);

/* ---- live conversion: audio fed while it is recorded, exact chunks out (additive, ABI 7) */
/* The conversion path is convolutional throughout (enc_q's WN, the two flow directions), so z_hat[:, t] of a recording
 * depends on its spectrogram columns [t - H, t + H] only, H = vsp_convert_halo_frames() =
 * posterior_layers (k - 1) / 2 + 2 n_flows flow_layers (k - 1) / 2 with k = flow_kernel: 96 for configs/config.json.
 * Column t reads the samples [t hop - pad, t hop - pad + n_fft) of the recording, pad = (n_fft - hop) / 2, reflected at
 * its two TRUE ends.  A recording can therefore be converted window by window while it arrives, and the result is not an
 * approximation: a frame is delivered once every sample it depends on is there, and it never changes later.
 *
 * vsp_convert_window_plan is that arithmetic without a device or a context.  To deliver the frames [e0, e1) of a
 * recording of which n_known samples have arrived, the window of frames is *w0 = max(0, e0 - halo) and *w1 = e1 + halo
 * while the recording is open, min(T(n_known), e1 + halo) once it is closed (T = vsp_convert_frames); [*s_lo, *s_hi) are
 * the samples the window's frames read, after reflection -- at sample 0 always, at the end only when closed.  Returns 1 if
 * every one of them is below n_known (the window can run), 0 if not yet, and VSP_ERR_ARG for e0 < 0, e1 <= e0, a closed
 * recording with e1 > T, hop <= 0, n_fft < hop, halo < 0 or n_known < 0.  The outputs (each may be NULL) are written
 * whenever the result is not an error.  An open window reads no sample at or behind n_known -- the condition under which
 * the one-shot front end does not reflect for its frames either: what is delivered early is what vsp_convert_latent
 * computes for the finished recording.
 *
 * vsp_convert_stream_rows runs up to 64 such windows in one set of launches.  Row b (HOST memory, read before the call
 * returns; it reaches the device as a kernel argument) holds the samples [first_sample, n_known) of its recording at
 * `audio` (DEVICE: sample s is audio[s - first_sample]) and asks for the frames [e0, e1), e1 - e0 <= span_frames.
 * z_hat [B][inter_channels][span_frames]: row b's columns [0, e1 - e0) are the frames [e0, e1) of what the reference
 * computes up to z_hat (voice_conversion, models.py:724-732) on spectrogram_torch of the WHOLE recording alone, to the
 * tolerance between two launch shapes of this library; the rest of the row is exactly 0.0.  g_tgt [B][gin] =
 * emb_g(sid_tgt), for the generator call.  No sample outside [s_lo, s_hi) of the row's plan is read.
 * NOISE LAYOUT: the posterior's noise for (channel c, frame t) of a row is noise_scale times element t * inter_channels + c
 * of the Philox stream keyed `seed` (vsp_randn_at) -- FRAME-major, so that it does not depend on the final length, which
 * an open recording does not have yet.  It is deliberately NOT the [inter][T_b] layout of vsp_convert_latent, which needs
 * T_b: the same seed gives different noise in the two entry points.  With noise_scale == 0 nothing is drawn and z = m_q.
 * How: the window framing (the ragged framing's scheme with a frame offset, a sample base and the end reflection only
 * for closed rows), the DFT convolution of vsp_spectrogram and a magnitude masked by w1 - w0; the chain of
 * vsp_convert_latent on the windows as utterances of w1 - w0 frames -- an artificial end a full halo from every delivered
 * frame, the trick of vsp_generator_stream_rows --; one cut launch.  No per-layer state is kept between calls: the halo is
 * recomputed, (chunk + 2 H) / chunk times the work of the chunk itself.  No allocation, no synchronisation, everything on
 * the caller's stream.  Checked on the host before anything is launched, VSP_ERR_ARG otherwise: 1 <= B <= 64, hop > 0,
 * span_frames >= 1, no null pointer, 0 <= first_sample <= s_lo, a finite noise_scale, speakers in [0, n_speakers), and
 * every row ready by vsp_convert_window_plan.  Needs the enc_q.* tensors (VSP_ERR_STATE).  Workspace:
 * vsp_convert_stream_rows_workspace_bytes -- sized by span_frames + 2 H frames per row, never by a recording's length.
 * ALGORITHMIC DELAY of a live conversion into the streamed vocoder (halo G = vsp_generator_halo_frames): the chunk of
 * frames [f0, f1) can run once sample (f1 + G + H - 1) hop - pad + n_fft - 1 has arrived, so the last frame of a chunk
 * leaves (G + H) hop + n_fft - pad samples after it was spoken, and the first one a chunk later: 57600 samples, about
 * 1.3 s at 44.1 kHz, for configs/config.json (G 14, H 96, hop 512, n_fft 2048). */
typedef struct vsp_convert_row {
  const float* audio;
  int64_t first_sample, n_known;
  int32_t closed, e0, e1;
  int64_t sid_src, sid_tgt;
  uint64_t seed;
  float noise_scale;
} vsp_convert_row;
int vsp_convert_halo_frames(const vsp_ctx* ctx);
int vsp_convert_window_plan(int n_fft, int hop, int halo, int64_t n_known, int closed, int e0, int e1, int* w0, int* w1,
                            int64_t* s_lo, int64_t* s_hi);
int64_t vsp_convert_stream_rows_workspace_bytes(const vsp_ctx* ctx, int B, int span_frames);
int vsp_convert_stream_rows(vsp_ctx* ctx, void* stream, int B, int hop, const vsp_convert_row* rows, int span_frames,
                            float* z_hat, float* g_tgt, void* workspace, int64_t workspace_bytes);

/* piecewise_rational_quadratic_transform with tails='linear' (reference transforms.py:12-193),
 * n elements, nb bins; uw/uh [n][nb], ud [n][nb-1]; outputs y[n], logabsdet[n]. */
int vsp_rq_spline(void* stream, int64_t n, int nb, const float* x, const float* uw, const float* uh,
                  const float* ud, int inverse, float tail_bound, float* y, float* logabsdet);

/* n standard-normal draws (device, float32): element i of the Philox4x32-10 stream keyed by `seed` (counter i / 4,
 * word i % 4, Box-Muller pairs).  A function of (seed, i) only.  This is the draw vsp_decode / vsp_infer make when
 * their noise argument is NULL; it replaces torch.randn_like (reference models.py:718, 240) for C callers and is not
 * bit-compatible with torch's generator.
 * STREAM CHANGE (late round 4, first released under ABI 5): the uniforms behind Box-Muller are built from 23 random bits
 * ((x + 0.5) / 2^23, strictly inside (0, 1)) instead of 24 ((x + 0.5) / 2^24 could round to exactly 1.0 in fp32 and
 * give log(1) = 0 radii).  EVERY element of the stream differs from what ABI <= 4 libraries of rounds 1-3 drew for the
 * same seed: audio reproduced from a stored seed is not bit-reproducible across that boundary. */
int vsp_randn(void* stream, uint64_t seed, int64_t n, float* out);
/* The same stream from element `first` on: out[i] = element first + i.  A shard [lo, hi) of a batch whose noise is
 * drawn by the library passes first = lo * inter * Tf and gets exactly the elements the unsharded call would draw for
 * those utterances. */
int vsp_randn_at(void* stream, uint64_t seed, int64_t first, int64_t n, float* out);
/* Where in that stream the noise tensor of vsp_decode / vsp_infer (noise == NULL) starts: element 0 of the context's
 * [B][inter][Tf] tensor is stream element `first_element` (default 0).  A rank that synthesises utterances [lo, hi) of a
 * global batch sets lo * inter * Tf (Tf = the GLOBAL padded frame count): the result no longer depends on the shard
 * layout.  Sticky until changed; 0 restores the default.  (Added in round 4; callers that never set it are unaffected.) */
int vsp_set_noise_offset(vsp_ctx* ctx, int64_t first_element);

/* ---- isolated mode (ABI 7, additive; round 10): batch-invariant synthesis ------------------ */
/* In a padded batch the reference applies no mask in dec, pitch_prenet, energy_prenet and EnergyPredictor (SURVEY gotcha
 * G5): a shorter utterance's audio depends on what it was batched with, and the default mode reproduces that padded call.
 * With the mode ON, every tensor vsp_encode / vsp_decode / vsp_infer / vsp_voice_conversion return, restricted to
 * utterance b's own extent (lengths[b] phonemes, L_b frames, min(L_b, max_len) frames of waveform), is what the reference
 * returns for a B = 1 call on that utterance's unpadded inputs -- independent of B, Tp, Tf, the other utterances and the
 * position in the batch; the controls are read at t < lengths[b] only; every float output is exactly 0.0 behind its extent
 * (x_mask as before).  The guarantee is the usual tolerance against the reference, not bit-identity with a B = 1 call of this
 * library (kernels are chosen by launch size).  Sticky context state, default OFF: nothing changes for callers that never
 * set it.  vsp_get_isolated: 0 / 1. */
int vsp_set_isolated(vsp_ctx* ctx, int on);
int vsp_get_isolated(const vsp_ctx* ctx);
/* Noise in isolated mode.  A caller's noise tensor [B][inter][Tf]: utterance b uses noise[b][:, :L_b].  noise == NULL: the
 * library draws utterance b's tensor as the first inter * L_b elements of the Philox stream keyed seeds[b], laid out
 * [inter][L_b] (element (c, t) = stream element c * L_b + t) -- exactly what a B = 1, Tf = L_b, noise_seed = seeds[b] call
 * draws -- so the sample does not depend on the batch either.  seeds_host [B] (host memory, copied; B = 0 forgets them);
 * a drawing call whose B differs from the seeds set fails with VSP_ERR_STATE.  The noise_seed argument and
 * vsp_set_noise_offset are not read in isolated mode. */
int vsp_set_noise_seeds(vsp_ctx* ctx, const uint64_t* seeds_host, int B);

/* ---- per-row controls (ABI 7, additive; round 13): every utterance of a batch with its own arguments ---------- */
/* Isolated mode makes row b of a batch what the reference returns for a B = 1 call; a row table makes that call's
 * ARGUMENTS per row.  With a table set, every tensor vsp_encode / vsp_decode / vsp_infer return, restricted to utterance
 * b's extent, is what the reference's infer (models.py:672-722) returns for a B = 1 call on b's unpadded inputs with
 *   duration_control = row b of duration_ctl if rows[b].given & VSP_GIVEN_DURATION, else the scalar rows[b].duration_scale
 *   pitch_control    = row b of pitch_ctl    if rows[b].given & VSP_GIVEN_PITCH,    else the scalar rows[b].pitch_scale
 *   energy_control   = row b of energy_ctl   if rows[b].given & VSP_GIVEN_ENERGY,   else the scalar rows[b].energy_scale
 *   noise_scale      = rows[b].noise_scale.
 * A scale whose control is given is not read (the reference's tensor branch has no scalar).  A *_ctl pointer may be NULL
 * only if no row has that bit set (else VSP_ERR_ARG); rows of a *_ctl tensor whose bit is clear may hold anything and are
 * never read.  A predictor runs iff some row lacks its bit; library-drawn noise (noise == NULL, vsp_set_noise_seeds) is
 * drawn iff some row's noise_scale is non-zero, and a row with noise_scale == 0 gets z_p = m_p exactly.
 * State: sticky host state, copied (rows_host [B]; B = 0 forgets the table); each call copies the table into ITS
 * workspace.  While a table is set the scalar duration_scale / pitch_scale / energy_scale / noise_scale arguments of
 * vsp_encode / vsp_decode / vsp_infer are not read; a call whose B differs from the table's, or a call made while the
 * context is not isolated (per-row values have no reference meaning in a padded batch), returns VSP_ERR_STATE.
 * Validation needs no device: a non-finite scale, unknown `given` bits, B < 0, or NULL rows with B > 0: VSP_ERR_ARG.
 * Nothing changes for callers that never set a table: the scalar launches run exactly as before. */
#define VSP_GIVEN_DURATION 1u
#define VSP_GIVEN_PITCH    2u
#define VSP_GIVEN_ENERGY   4u
typedef struct vsp_row_control {
  float duration_scale, pitch_scale, energy_scale, noise_scale;
  uint32_t given;
} vsp_row_control;
int vsp_set_row_controls(vsp_ctx* ctx, const vsp_row_control* rows_host, int B);

/* ---- mel spectrogram (reference mel_processing.py:73-112) --------------------------------- */
/* The mel basis the reference takes from librosa.filters.mel(sampling_rate, n_fft, n_mels, fmin, fmax) with that
 * function's defaults (Slaney mel scale: linear below 1 kHz, logarithmic above; triangles between successive mel
 * points; Slaney area normalisation): basis_host[n_mels][n_fft / 2 + 1], computed on the host in double precision.
 * librosa is a third-party dependency of the reference (requirements.txt, no version pinned) and is not vendored:
 * this restates its published algorithm.  fmax <= 0 means sampling_rate / 2.
 * Pinned (round 5) to a third party's implementation of the same routine: transformers.audio_utils.mel_filter_bank(norm =
 * "slaney", mel_scale = "slaney") -- "adapted from torchaudio and librosa" -- agrees to fp32 rounding for the reference's
 * configuration and three other shapes (tests/test_oracle_golden.py, on the CPU).  librosa itself and torchaudio are not
 * in the build image: the reference's own call has never been run beside it. */
int vsp_mel_filterbank(int sampling_rate, int n_fft, int n_mels, float fmin, float fmax, float* basis_host);
/* spec_to_mel_torch (reference mel_processing.py:73-82): mel = log(clamp(basis @ spec, min = 1e-5)).
 * spec [B][n_fft / 2 + 1][T] and mel [B][n_mels][T] are device pointers; the basis is built and uploaded inside the
 * call.  vsp_spectrogram followed by this call = mel_spectrogram_torch (mel_processing.py:85-112).
 * NOT on the infer path, and unlike it this entry allocates: every call hipMallocs the basis + band tables, uploads
 * them, synchronises the stream and frees them again (the header's "no hidden allocation, no sync" promise covers
 * vsp_encode / vsp_decode / vsp_infer and the per-stage entries that take a workspace, not this metric helper). */
int vsp_spec_to_mel(void* stream, int B, int T, int n_fft, int n_mels, int sampling_rate, float fmin, float fmax,
                    const float* spec, float* mel);

/* ---- vocoder operators, stand-alone (no context) ------------------------------------------ */
/* The channels-last split-f16 convolution kernels of the generator as plain operators, for unit parity
 * and for callers that hold their own weights.  Activations are device pointers, fp32, channels-last
 * [B][T][C]; weights and biases are HOST pointers in the reference's dense layout (torch.nn.Conv1d
 * weight [Cout][Cin][K], weight-norm already folded); they are packed into fragment order and uploaded
 * inside the call, which synchronises the stream before it returns (these are not the fast path:
 * vsp_generator keeps its weights packed in the arena).  terms = 3: fp32-accurate split products,
 * 1: plain f16 operands.
 *
 * vsp_cl_conv1d: out = conv1d(lrelu(x, in_slope), w, dilation, padding = dilation (K - 1) / 2) + bias
 * [+ res]; in_slope = 1 applies no activation (reference modules.py:214-221: F.leaky_relu + Conv1d).
 * Cin % 32 == 0, Cout % 32 == 0, K odd, (K - 1) * dilation <= 64.  Also Cin == Cout == 16 (additive: the last stage
 * of a five-stage generator, g16_c16; x != out there); 16 mixed with another count is VSP_ERR_UNSUPPORTED. */
int vsp_cl_conv1d(void* stream, int B, int T, int Cin, int Cout, int K, int dilation, const float* x,
                  const float* w_host, const float* bias_host, float in_slope, const float* res, int terms,
                  float* out);
/* vsp_conv1d: the frame- / phoneme-rate convolution kernel (conv1d_f32_mfma) as a plain operator on the reference's
 * layout, x [B][Cin][T] -> out [B][Cout][T] (device, fp32, T contiguous):
 *   out = epilogue(conv1d(prologue(x), w, dilation, padding = dilation (K - 1) / 2) + bias)
 * prologue: x * mask (lengths != NULL and mask_in) then leaky_relu(x, in_slope) when in_act; epilogue: act 0 none,
 * 1 relu, 2 WN gate tanh(rows [0, Cout/2)) * sigmoid(rows [Cout/2, Cout)) of interleaved 32-row tiles (then the output
 * has Cout / 2 rows; commons.py:100-107; no residual with the gate); then + res [B][rows][T], then * mask when mask_out.  K odd,
 * (K - 1) * dilation + 3 <= 64, T % 4 == 0 or T == 1 (the cond(g) projections of one time step).  split_f16 = 1: fp32-accurate split-f16 MFMA (the default path of the library),
 * 0: f32 MFMA, 2 (round 6): the split-f16 COLUMN-TILE kernel -- every output row of a 64-column tile in one block, what the
 * path uses for the 1x1 convolutions of mid-size grids -- K = 1, Cin 96 or 192, Cout a multiple of 16 in [64, 576], act 0,
 * no in_act (VSP_ERR_UNSUPPORTED otherwise).  Reference: torch.nn.Conv1d as used in attentions.py:138-145, 277-285,
 * modules.py:148-176. */
int vsp_conv1d(void* stream, int B, int T, int Cin, int Cout, int K, int dilation, const float* x, const float* w_host,
               const float* bias_host, const int64_t* lengths, int mask_in, int in_act, float in_slope, int act,
               const float* res, int mask_out, int split_f16, float* out);
/* vsp_conv1d_ex (ABI 7, additive): the same kernels with the WHOLE fused epilogue the frame-rate layers use, on strided
 * tensors, and a report of which kernel form the launch took -- what tests/test_frame_conv_epilogue.py and
 * tests/test_conv_form_host.py drive.  Like vsp_conv1d: host weights packed per call, no context, synchronises.
 *   y   = conv1d(prologue(x), w, dilation, padding = dilation (K - 1) / 2) + bias
 *   rows >= split_row (split_row > 0):  out2[row - split_row] = (y [+ out2 when acc_prev2]) [* mask when mask_post2]
 *   the other rows:  y + cond[b][row] -> relu (act 1) / WN gate (act 2, as vsp_conv1d: out has Cout / 2 rows)
 *                    -> * mask when mask_pre -> * alpha -> + res -> + out when acc_prev -> / div -> * mask when mask_post
 *   ln 1 / 2:  out = LayerNorm_channels(that + res, eps 1e-5) * ln_gamma + ln_beta   (res enters HERE, not above)
 * out has split_row rows when split_row > 0 and out2 the Cout - split_row others.  res == out and res == x are allowed.
 * Strides are in ELEMENTS; 0 = dense ([B][rows][T]); a channel stride >= T, a batch stride >= rows * channel stride: a
 * tensor may be a channel window of a larger one, or have rows that are not 16-byte aligned.
 * The WN gate reads its tanh / sigmoid halves from interleaved 32-row tiles: kernel row r holds the reference's row
 * (r / 32 % 2) * Cout / 2 + (r / 64) * 32 + r % 32.  w and bias (host) are given in the REFERENCE's order and permuted here;
 * cond is a device array the kernels read in place with the caller's stride and alignment, so the CALLER stores it in
 * kernel row order.
 * split_f16 1: split-f16 MFMA, 0: f32 MFMA.  cols 1: the column-tile kernel (conv_cols.hip) or VSP_ERR_UNSUPPORTED.
 * ln 1: LayerNorm fused into the column-tile launch (needs cols 1; Cin = Cout = 192, no masks, no alpha / acc_prev);
 * ln 2: the convolution into a scratch tensor, then the LayerNorm kernel (any Cout).
 * plan_only: validate and fill *form_out, no device access, no HIP call (x is then any address of the alignment in
 * question: the kernel choice reads it, nothing dereferences it).  form_out may be NULL otherwise.
 * VSP_ERR_ARG: a null or contradictory pointer (out2 without split_row, masks without lengths, ln without gamma / beta
 * or the reverse, ln 1 without cols), a gate with res or split_row, split_row outside (0, Cout), div == 0, a stride
 * below the extent it spans, a length outside [0, T].  VSP_ERR_UNSUPPORTED: what the launchers refuse (even K, the halo,
 * a gate with Cout % 64 or with mask_pre / alpha / acc_prev / div -- its epilogue is cond and mask_post --, split_row % 32,
 * cols outside conv_cols.hip's shapes, ln with the gate, split_row or acc_prev) and a tensor whose largest byte offset
 * (rows * channel stride + T) * 4 reaches 2^31.  B = 0 or T = 0: VSP_OK, nothing launched. */
enum {
  VSP_CONV_FORM_NONE = 0,
  VSP_CONV_FORM_COLS = 1,         /* conv_cols_kernel */
  VSP_CONV_FORM_COLS_LN = 2,      /* conv_cols_kernel with the fused LayerNorm */
  VSP_CONV_FORM_GEMV = 3,         /* conv_t1_gemv: one time step */
  VSP_CONV_FORM_SPLITK = 4,       /* conv_frame_splitk<k, gate> */
  VSP_CONV_FORM_FRAME_SHORT = 5,  /* conv_frame_f16s<2, 1, 1, 2, k>: Nq <= 96 */
  VSP_CONV_FORM_FRAME = 6,        /* conv_frame_f16s<2, 1, 1, 4, k> */
  VSP_CONV_FORM_TILE = 7          /* conv1d_f32_mfma<mt, nt, wm, wn, f16s, ring, prune> */
};
typedef struct vsp_conv_form {
  int32_t kernel;                 /* VSP_CONV_FORM_* */
  int32_t mt, nt, wm, wn;         /* TILE: the tile tuple (rows 32 mt wm, columns 32 nt wn); FRAME*: likewise; else 0 */
  int32_t f16s, ring, prune;      /* TILE: the instantiation's flags */
  int32_t k, gate;                /* SPLITK / FRAME*: the tap-count instantiation; SPLITK: the gate instantiation */
} vsp_conv_form;
typedef struct vsp_conv1d_desc {
  int32_t B, T, Cin, Cout, K, dilation;
  int64_t x_bs, x_cs, o_bs, o_cs, r_bs, r_cs, o2_bs, o2_cs;     /* element strides, 0 = dense */
  const float* x; float* out; const float* res; float* out2;    /* device */
  const int64_t* lengths;                                       /* device [B] or NULL */
  const float* cond; int64_t cond_bs;                           /* device, cond[b * cond_bs + kernel row] or NULL */
  const float *w, *bias, *ln_gamma, *ln_beta;                   /* host: [Cout][Cin][K], [Cout], [Cout], [Cout] */
  int32_t mask_in, in_act; float in_slope;
  int32_t act, mask_pre; float alpha; int32_t acc_prev; float div;
  int32_t mask_post, split_row, acc_prev2, mask_post2;
  int32_t split_f16, cols, ln, plan_only;
} vsp_conv1d_desc;
int vsp_conv1d_ex(void* stream, const vsp_conv1d_desc* d, vsp_conv_form* form_out);
/* vsp_cl_resblock: ResBlock1.forward without the mask (reference modules.py:210-223):
 *   for p < n_pairs:  x = x + conv2_p(lrelu(conv1_p(lrelu(x), dilations[p]))), slope 0.1
 * w_host[2 p], w_host[2 p + 1] = conv1_p, conv2_p dense [C][C][K]; bias_host likewise [C].
 * mode 0: one launch per convolution (g16_conv), any C % 32 == 0;
 * mode 1: one launch per pair (g16_pair), C = 32 or 64;  mode 2: ONE launch (g16_chain), C = 32 or 64,
 * n_pairs <= 3.  The three modes return identical bits.  x != out.
 * C = 16 (additive: g16_c16): mode 0 one launch per convolution, mode 1 a pair's two
 * convolutions per launch, mode 2 the whole block (n_pairs <= 3) -- one kernel, identical bits. */
int vsp_cl_resblock(void* stream, int B, int T, int C, int K, int n_pairs, const int* dilations, const float* x,
                    const float* const* w_host, const float* const* bias_host, int mode, int terms, float* out);
/* vsp_cl_resblock2 (round 7, ABI 7, additive): ResBlock2.forward without the mask (reference modules.py:245-249):
 *   for c < 2:  x = x + conv_c(lrelu(x), dilations[c]), slope 0.1
 * w_host[c] dense [C][C][K], bias_host[c] [C]; x, out [B][T][C] channels-last, x != out.
 * mode 0: one launch per convolution (g16_conv, in_act + res), any C % 32 == 0;  mode 1: ONE launch (g16_rb2),
 * C = 32 or 64, (K - 1) / 2 * dilations[c] <= 32.  The two modes return identical bits.  Outside the kernels' cover:
 * VSP_ERR_UNSUPPORTED.  C = 16 (additive): both modes on g16_c16. */
int vsp_cl_resblock2(void* stream, int B, int T, int C, int K, const int* dilations, const float* x,
                     const float* const* w_host, const float* const* bias_host, int mode, int terms, float* out);
/* vsp_cl_block_ex (ABI 7, additive): the two ResBlock operators above as ONE descriptor-based operator that also takes the
 * launch inputs only the generator's schedule sets otherwise -- the accumulate / divide epilogue of a block's last launch,
 * the ragged batch, the kernel-choice flags -- and reports which kernel every launch of the block took.  What
 * tests/test_cl_block_ops.py and tests/test_cl_block_route_host.py drive; vsp_cl_resblock and vsp_cl_resblock2 are this
 * operator with acc_prev 0, div 1, lengths NULL and the flags read from VSP_PAIR / VSP_RW64 / VSP_CHAIN_RING.
 *   kind 1: ResBlock1 of n_pairs pairs (w[2 p], w[2 p + 1] = conv1_p, conv2_p);  kind 2: ResBlock2 (w[0], w[1]; n_pairs ignored)
 *   mode 0: one launch per convolution;  1: one launch per pair, or the fused ResBlock2;  2: one launch for a ResBlock1
 *   out = (block(x) [+ out when acc_prev]) / div, computed by the block's LAST launch (the generator's sum over a stage's
 *   ResBlocks, reference models.py:276-285); x != out.
 *   lengths: NULL or a DEVICE int32 [B]; utterance b's tensor then ends after lengths[b] * grate columns
 *   (1 <= lengths[b], lengths[b] * grate <= T): the rows at and behind the end read as zero -- whatever they hold -- and
 *   no row of out there is written.  Every launch of the block gets the same ragged extent.
 *   ring: the LDS-ring pair kernel where g16_rw exists;  rw64: g16_rw64 for 64-channel kernel-3 pairs;  chain_ring: the
 *   LDS-ring chain kernel where g16_rc exists;  no_image: mode 0 of a ResBlock1 keeps a pair's intermediate as an fp32
 *   tensor (what the generator's stages below 128 channels do) where the operator otherwise hands it over as an operand
 *   image (terms 3, K >= 3, C >= 32: the >= 128-channel stages).  Identical bits.
 *   plan_only: validate and fill *route, no device access, no HIP call (x, out, lengths are then any non-null addresses,
 *   the lengths are not read; the tables w and bias are read for NULL entries, the weights behind them are not).
 * route (may be NULL unless plan_only): the launches in order, for each the kernel (VSP_CL_KERNEL_*), the columns one of its
 * tiles STORES (tile_cols), for g16_conv the rows of its row tile, and the instantiation (variant: CONV 1 = the image-only
 * epilogue through the LDS; PAIR the waves of a block; RB2 1 = the 512-column block).  The launchers switch on the same
 * route functions (kernels.h: g16_conv_route, g16_pair_route, g16_chain_route, g16_rb2_route, g16_c16_route).
 * VSP_ERR_ARG: a null pointer, x == out, kind / mode / terms out of range, div == 0, grate < 1, a length outside
 * [1, T / grate], plan_only without route.  VSP_ERR_UNSUPPORTED: the shapes vsp_cl_resblock / vsp_cl_resblock2 refuse.
 * B = 0 or T = 0: VSP_OK, nothing launched.  With lengths the call copies them to the host and synchronises first. */
enum {
  VSP_CL_KERNEL_NONE = 0,
  VSP_CL_KERNEL_CONV = 1,         /* g16_conv tile, fp32 input */
  VSP_CL_KERNEL_CONV_IMG = 2,     /* g16_conv tile reading an operand image */
  VSP_CL_KERNEL_PIPE = 3,         /* g16_convp: persistent image-input tiles (uniform batches only) */
  VSP_CL_KERNEL_PAIR = 4,         /* g16_pair: the LDS-ring pair tile */
  VSP_CL_KERNEL_RW = 5,           /* g16_rw<K, ACC> */
  VSP_CL_KERNEL_RW64 = 6,         /* g16_rw64<ACC> */
  VSP_CL_KERNEL_PP = 7,           /* g16_pp: the ping-pong pair tile, 128 channels */
  VSP_CL_KERNEL_CHAIN = 8,        /* g16_chain: the LDS-ring chain tile (32 channels: the 256-column block) */
  VSP_CL_KERNEL_CHAIN_WIDE = 9,   /* g16_chain, 32 channels, the 512-column block */
  VSP_CL_KERNEL_RC = 10,          /* g16_rc */
  VSP_CL_KERNEL_RB2 = 11,         /* g16_rb2 */
  VSP_CL_KERNEL_C16 = 12,         /* g16_c16 */
  VSP_CL_KERNEL_UPS = 13          /* g16_ups: the streaming up-convolution (never part of a ResBlock) */
};
typedef struct vsp_cl_launch_route {
  int32_t kernel;                 /* VSP_CL_KERNEL_* */
  int32_t tile_cols;              /* columns one tile stores */
  int32_t rows;                   /* CONV / CONV_IMG / PIPE: output rows of the row tile (128, 64, 32); else 0 */
  int32_t variant;                /* see above */
} vsp_cl_launch_route;
#define VSP_CL_BLOCK_MAX_LAUNCHES 16
typedef struct vsp_cl_block_route {
  int32_t n;                                               /* launches of the block */
  vsp_cl_launch_route launch[VSP_CL_BLOCK_MAX_LAUNCHES];
} vsp_cl_block_route;
typedef struct vsp_cl_block_desc {
  int32_t kind, mode, B, T, C, K, n_pairs, terms;
  const int32_t* dilations;                                /* host: kind 1 [n_pairs], kind 2 [2] */
  const float* x; float* out;                              /* device [B][T][C] */
  const float* const* w; const float* const* bias;         /* host: dense [C][C][K] and [C] per convolution, execution order */
  const int32_t* lengths;                                  /* device [B] or NULL */
  int32_t grate;
  int32_t acc_prev; float div;
  int32_t ring, rw64, chain_ring, no_image;
  int32_t plan_only;
} vsp_cl_block_desc;
int vsp_cl_block_ex(void* stream, const vsp_cl_block_desc* d, vsp_cl_block_route* route);
/* vsp_cl_conv_post (ABI 7, additive): the channels-last generator's last layer as a plain operator (reference
 * models.py:286-288: F.leaky_relu, conv_post without bias, tanh),
 *   out[b][t] = tanh(unscale * sum_{c, j} w[0][c][j] * lrelu(x[b][t + j - (K - 1) / 2][c], slope))
 * x DEVICE [B][T][C] channels-last, C 16 / 32 / 64; w_host HOST [1][C][K] (the reference's layout), K odd and <= 7;
 * out DEVICE [B][T].  lengths / grate as in vsp_cl_block_ex: utterance b ends after lengths[b] * grate columns, the rows
 * behind read as zero and out behind is not written.  No status word is passed to the kernel.
 * VSP_ERR_ARG: a null pointer, grate < 1, a length outside [1, T / grate];  VSP_ERR_UNSUPPORTED: C or K outside the above. */
int vsp_cl_conv_post(void* stream, int B, int T, int C, int K, const float* x, const float* w_host, float slope, float unscale,
                     const int32_t* lengths, int grate, float* out);
/* vsp_cl_conv_transpose1d (ABI 7, additive): HiFi-GAN's up-convolution as the channels-last generator runs it
 * (reference models.py:253-256, 277-278: F.leaky_relu + ConvTranspose1d),
 *   out = conv_transpose1d(lrelu(x, in_slope), w, bias, stride, padding = (K - stride) / 2)
 * x [B][T][Cin], out [B][T stride][Cout] channels-last; in_slope = 1 applies no activation.  w_host is torch's
 * ConvTranspose1d weight [Cin][Cout][K] (weight-norm folded), bias_host [Cout] or NULL.  They are packed as the model packs
 * dec.ups.* and the launch goes through the generator's launcher, so a shape and grid run the kernel the generator would
 * run (the streaming g16_ups or the polyphase g16_conv tile).  lengths: NULL or a DEVICE int32 [B], 0 <= lengths[b] <= T:
 * utterance b's tensor then ends after lengths[b] input rows (the generator's ragged batch) -- out rows [0, lengths[b]
 * stride) are those of x[b, :lengths[b]], the rows behind them are not written.  Cin % 32 == 0, Cout % 16 == 0, stride Cout
 * a multiple of 32, K % stride == 0, K - stride even, K / stride - 1 <= 64, an utterance's input and output below 2 GiB:
 * VSP_ERR_UNSUPPORTED otherwise; x == out, a bad terms or a length outside [0, T]: VSP_ERR_ARG. */
int vsp_cl_conv_transpose1d(void* stream, int B, int T, int Cin, int Cout, int K, int stride, const float* x,
                            const float* w_host, const float* bias_host, float in_slope, const int32_t* lengths,
                            int terms, float* out);
/* vsp_conv_transpose1d (ABI 7, additive): the same up-convolution on the f32 MFMA kernel (conv1d_f32_mfma's transposed
 * epilogue), as the f32 generator runs it: VSP_GENERATOR=f32, and the configurations whose channel counts the split-f16
 * kernels do not cover.  Channel-major x [B][Cin][T] -> out [B][Cout][T stride] (device, fp32, T contiguous); any Cin and
 * Cout; w_host / bias_host as above.  The generator pads its time rows to a multiple of 64 columns: the call stages x and
 * out through such buffers itself (any T >= 1).  K % stride == 0, K - stride even, K / stride + 2 <= 64:
 * VSP_ERR_UNSUPPORTED otherwise; x == out: VSP_ERR_ARG. */
int vsp_conv_transpose1d(void* stream, int B, int T, int Cin, int Cout, int K, int stride, const float* x,
                         const float* w_host, const float* bias_host, float in_slope, float* out);

/* ---- attention operators, stand-alone (ABI 7, additive) ------------------------------------ */
/* The two windowed relative-position attention kernels (reference attentions.py:148-179) as plain operators on the
 * reference's layout, with every block form selectable: what tests/test_attention_ops.py drives.  Like the vocoder
 * operators above they allocate, upload and synchronise the stream inside the call (not the fast path: vsp_encoder).
 *
 * vsp_rel_attention: qkv DEVICE fp32 [B][3 H][T] (rows [0, H) = q, [H, 2 H) = k, [2 H, 3 H) = v, T contiguous) ->
 * out DEVICE fp32 [B][H][T].  emb_k_host / emb_v_host: HOST fp32 [2 window + 1][H / n_heads], shared over the heads.
 * lengths: NULL or a DEVICE int64 [B], 0 <= lengths[b] <= T; pairs with a query or key at or beyond lengths[b] score
 * -1e4, so a query row at or beyond it (every row of an utterance of length 0) is the uniform average over all T keys,
 * as in the reference; all T columns of out are written.
 * kernel 0: attention.hip (f32 MFMA, two passes), 1: attention_f16s.hip (split-f16, online softmax).
 * variant -1: the launcher's choice from the grid size, as the model runs it; 0: the small-grid form (kernel 0: 32-query
 * blocks whose four waves split the keys; kernel 1: 64-query blocks with two key-tile streams); 1: the 128-query form.
 * VSP_ERR_ARG: a null pointer, B or T negative, kernel or variant out of range, a length outside [0, T].
 * VSP_ERR_UNSUPPORTED: H / n_heads not 32, 64 or 96, H % n_heads != 0, window outside [0, 7].  B = 0 or T = 0: VSP_OK,
 * nothing launched. */
int vsp_rel_attention(void* stream, int B, int T, int H, int n_heads, int window, const float* qkv,
                      const float* emb_k_host, const float* emb_v_host, const int64_t* lengths, int kernel, int variant,
                      float* out);
/* vsp_rel_attention_fused: the projections conv_q | conv_k | conv_v of x * mask (attentions.py:138-146) and the operand
 * packing in ONE launch (attn_qkv_pack_f16s), then the split-f16 attention on the packed images -- an encoder layer's
 * attention as vsp_encoder runs it on mid-size grids.  x DEVICE fp32 [B][H][T]; w_qkv_host HOST fp32 [3 H][H] (the three
 * 1x1 convolution weights stacked q | k | v), bias_qkv_host [3 H]; the rest as above, variant for the attention launch.
 * n_heads = 2 and H = 192, 128 or 64 only: VSP_ERR_UNSUPPORTED otherwise. */
int vsp_rel_attention_fused(void* stream, int B, int T, int H, int n_heads, int window, const float* x,
                            const float* w_qkv_host, const float* bias_qkv_host, const float* emb_k_host,
                            const float* emb_v_host, const int64_t* lengths, int variant, float* out);

/* ---- output stage (round 8, ABI 7, additive) ------------------------------------------------ */
/* The last hop of the reference's /tts handler: it writes the 44.1 kHz waveform and runs `ffmpeg -i c.wav -ar 22050`
 * (inference_api.py:50-52); clients receive 22.05 kHz PCM16.  Here: waveform float32 at the model's rate -> polyphase FIR
 * resampling by L / M -> float32 or PCM16 at the output rate, one launch, on the caller's stream, one-shot or chunked.
 *
 * The filter is specified, not copied, so that anybody can recompute it.  g = gcd(in_rate, out_rate), L = out_rate / g,
 * M = in_rate / g, Q = max(L, M); a Kaiser-windowed sinc at rate in_rate * L:
 *   H    = zeros * Q                                  (half length; 2 H + 1 taps)
 *   fc   = rolloff / Q
 *   h[n] = L fc sinc(fc n) kaiser(2 H + 1, beta)[n + H],  n = -H .. H        (numpy's sinc / kaiser conventions)
 *   y[m] = sum_k h[m M - k L] x[k],  k in [0, n_valid) with |m M - k L| <= H,  m = 0 .. ceil(n_valid L / M) - 1
 * x is zero outside [0, n_valid): y is scipy.signal.resample_poly(x, L, M, window = h / L).  Defaults: zeros 32,
 * beta 9.62 (Kaiser's formula for 96 dB, the floor of a 16-bit output), rolloff 1 - 3.065 / zeros (stop-band edge on the
 * narrower Nyquist frequency).  Supported: L <= 320, M <= 441, 1 <= zeros <= 64 (VSP_ERR_UNSUPPORTED beyond; other bad
 * arguments VSP_ERR_ARG).  L = M = 1 is the pass-through: H = 0, one unit tap -- quantisation only.
 *
 * vsp_resample_plan / vsp_resample_filter / vsp_resample_out_len are host-only (no device, like vsp_mel_filterbank): the
 * plan, the 2 H + 1 taps (computed in double precision, rounded to fp32 once; rolloff <= 0 selects the default) and
 * ceil(n L / M). */
int vsp_resample_plan(int in_rate, int out_rate, int zeros, int* L, int* M, int* half_len);
int vsp_resample_filter(int in_rate, int out_rate, int zeros, double beta, double rolloff, float* taps_host);
int64_t vsp_resample_out_len(int64_t n, int L, int M);
/* Builds the filter of (in_rate -> out_rate) and uploads its table to the context's device; replaces an earlier one.  May
 * allocate and synchronise (like vsp_finalize_weights; needs no weights).  out_rate == in_rate configures the pass-through,
 * out_rate == 0 turns the stage off and frees the table.  zeros == 0: 32; rolloff <= 0: 1 - 3.065 / zeros. */
int vsp_output_configure(vsp_ctx* ctx, int in_rate, int out_rate, int zeros, double beta, double rolloff);
/* No allocation, no synchronisation, caller's stream.  x [B][x_stride] holds input samples [x_first, x_first + x_len) of
 * each utterance; n_valid [B] (DEVICE int64, NULL = n_max for all) is each utterance's TOTAL valid length, n_max (host) an
 * upper bound of them (the padded length: the host cannot read n_valid without a synchronisation, so the shape checks and
 * the grid use n_max; n_valid is clamped to [0, n_max]).  Writes output samples [m0, m1) to out[b][0 .. m1 - m0)
 * (out [B][out_stride]; float32 if pcm == 0, int16 if pcm == 1: clip(rint(y * 32767.0f), -32768, 32767), round half to
 * even, product in fp32 -- the rule of vispeech_amd.service.pcm16).  Samples at and behind ceil(n_valid[b] L / M) are
 * written as 0.  Input positions outside [0, n_valid[b]) are never read: what a padded batch holds there cannot reach
 * the output.  Every input sample of [0, n_max) that a requested output depends on must lie in the passed window, and
 * x_first + x_len <= n_max, x_len <= x_stride, m1 <= ceil(n_max L / M), m1 - m0 <= out_stride: VSP_ERR_SHAPE otherwise,
 * decided on the host before anything is launched.  The one-shot call is x_first = 0, x_len = n_max, m0 = 0,
 * m1 = ceil(n_max L / M).  An output sample's value depends on (x, m) alone -- one thread per sample, fp32 FMAs in ascending
 * k -- not on the window, the tile or the batch layout: outputs computed window by window are the bytes of the one-shot call
 * (which outputs a window completes: vispeech_amd.output_stage.complete_outputs).  Not configured: VSP_ERR_STATE. */
int vsp_output_chunk(vsp_ctx* ctx, void* stream, int B, const float* x, int64_t x_stride, int64_t x_first, int64_t x_len,
                     const int64_t* n_valid, int64_t n_max, int64_t m0, int64_t m1, void* out, int64_t out_stride,
                     int pcm);

/* Streaming for batched requests THROUGH the output stage (ABI 7, additive; round 12): vsp_generator_stream_rows with the
 * ragged output stage in place of the collect launch -- still one launch set per tick, and what crosses to the host is PCM16
 * at the output rate.  Row b delivers frames [f0, f1) of an utterance of Lf frames (`row`, as above); with
 * up = prod(upsample_rates), x_first = f0 up and n = (f1 - f0) up its new INPUT samples are [x_first, x_first + n), and with
 * (L, M, H) of the configured stage (vsp_resample_plan)
 *   complete(s, ended) = ended ? ceil(s L / M) : min(ceil(s L / M), max(0, ceil((L s - H) / M)))
 *   start(m)           = max(0, ceil((m M - H) / L))
 *   m0 = complete(x_first, 0)          m1 = complete(x_first + n, f1 == Lf)
 *   k0 = min(x_first, start(m0))       k1 = min(x_first + n, start(m1))
 * (the rule of vispeech_amd.output_stage: every call delivers every output its input completes, so m0 of a call is m1 of the
 * call that ended at its f0 and no counter travels between calls).  The call writes output samples [m0, m1) of the
 * utterance's one-shot output stage to out[b][0 .. m1 - m0) -- float32 (pcm == 0) or int16 (pcm == 1) by the rule of
 * vsp_output_chunk, the same taps in the same order on the same input samples: the concatenation over an utterance's calls
 * is what vsp_output_chunk returns for the concatenated float rows of vsp_generator_stream_rows, bit for bit -- and exactly 0
 * to out[b][m1 - m0 .. out_stride).  m1 == m0 is legal (a short chunk at a low output rate): the row is all zeros.
 * hist_in holds input samples [k0, x_first) as the row's previous call wrote them (ignored, may be NULL, when f0 == 0 or
 * K == 0); the call writes samples [k1, x_first + n) to hist_out[0 ..).  Both are DEVICE buffers of
 * K = vsp_output_history_samples floats and must differ (blocks of one launch read the one and write the other): a request
 * owns two and alternates.  vsp_stream_rows_output_plan is the host arithmetic without a context (it reads L, f0, f1 of each
 * row; every output may be NULL; it checks 1 <= B <= 64 and 0 <= f0 < f1 <= L like vsp_stream_rows_plan).
 * vsp_output_history_samples = floor(2 H / L), which bounds both x_first - k0 and x_first + n - k1: the first incomplete
 * output m >= (L s - H) / M starts at ceil((m M - H) / L) >= s - 2 H / L.  0 for the pass-through.
 * vsp_stream_rows_out_samples = ceil(n L / M) + ceil(H / M) rounded up to a multiple of 4, n = chunk_frames up: an upper bound
 * of m1 - m0 (reached only by a final call, which flushes the filter's tail); an out_stride of that many ELEMENTS always fits.
 * Checked on the host before anything is launched: the output stage is configured (VSP_ERR_STATE); the arguments of
 * vsp_generator_stream_rows (there is no chunk_frames here: the workspace bounds the windows), hist_out non-NULL when K > 0,
 * hist_in non-NULL when K > 0 and f0 > 0, hist_in != hist_out (VSP_ERR_ARG); every m1 - m0 <= out_stride (VSP_ERR_SHAPE).
 * Workspace: vsp_generator_stream_rows_workspace_bytes.  No allocation, no synchronisation, everything on the caller's stream. */
typedef struct vsp_stream_row_out {
  vsp_stream_row row;
  const float* hist_in;
  float* hist_out;
} vsp_stream_row_out;
int vsp_stream_rows_output_plan(int L, int M, int H, int up, int B, const vsp_stream_row* rows, int64_t* m0, int64_t* m1,
                                int64_t* k0, int64_t* k1);
int vsp_output_history_samples(int L, int M, int H);
int64_t vsp_stream_rows_out_samples(int L, int M, int H, int up, int chunk_frames);
int vsp_generator_stream_rows_output(vsp_ctx* ctx, void* stream, int B, const vsp_stream_row_out* rows, void* out,
                                     int64_t out_stride, int pcm, void* workspace, int64_t workspace_bytes);

/* ---- input stage (round 16, ABI 7, additive) ------------------------------------------------ */
/* The mirror of the output stage, in front of voice conversion: raw samples at the rate and in the encoding a recording
 * arrives in -> float32 at the model's rate, on the GPU, ragged over a batch and exact under any split of a live feed.
 * (The reference brings its data to the model's rate offline, with librosa, in its data preparation.  This filter is
 * ours by specification -- the output stage's published formula with the rates swapped; it is NOT librosa's resample.)
 *
 *   g = gcd(in_rate, model_rate), L = model_rate / g, M = in_rate / g, Q = max(L, M)
 *   H    = zeros * Q                                  (half length; 2 H + 1 taps)
 *   fc   = rolloff / Q
 *   h[n] = L fc sinc(fc n) kaiser(2 H + 1, beta)[n + H],  n = -H .. H        (numpy's sinc / kaiser conventions)
 *   y[m] = sum_k h[m M - k L] x[k],  k in [0, n) with |m M - k L| <= H,  m = 0 .. ceil(n L / M) - 1
 * computed in double precision and rounded to fp32 once.  Defaults: zeros 32, beta 9.62, rolloff 1 - 3.065 / zeros.
 * L = M = 1 is the pass-through: H = 0, one unit tap -- decoding only.  Supported: L <= 441, M <= 640, 1 <= zeros <= 64
 * (VSP_ERR_UNSUPPORTED beyond; other bad arguments VSP_ERR_ARG).  8 / 16 / 32 kHz -> 44.1 kHz are 441 / 80, 441 / 160 and
 * 441 / 320; 48 / 96 / 192 kHz are 147 / 160, 147 / 320 and 147 / 640.
 *
 * x[k] is the decoded sample, float32:
 *   VSP_IN_F32   the float32 taken as it is
 *   VSP_IN_S16   x = s / 32768.0f, s the int16 (exact)
 *   VSP_IN_ULAW  x = v / 32768.0f (exact), v the 16-bit linear value of ITU-T G.711 mu-law for code byte c:
 *                  u = ~c & 0xFF;  e = (u >> 4) & 7;  q = u & 15;  t = (((q << 3) + 0x84) << e) - 0x84;  v = (u & 0x80) ? -t : t
 *                (0xFF -> 0, 0x7F -> 0, 0x80 -> +32124, 0x00 -> -32124)
 *   VSP_IN_ALAW  x = v / 32768.0f (exact), v the 16-bit linear value of ITU-T G.711 A-law for code byte c:
 *                  a = c ^ 0x55;  e = (a >> 4) & 7;  q = a & 15;  t = (q << 4) + 8;  if (e >= 1) t = (t + 0x100) << (e - 1);
 *                  v = (a & 0x80) ? t : -t
 *                (0xD5 -> +8, 0x55 -> -8, 0xAA -> +32256, 0x2A -> -32256)
 *
 * vsp_input_plan / vsp_input_filter / vsp_input_decode_table are host-only (no device): the plan, the 2 H + 1 taps
 * (rolloff <= 0 selects the default; zeros == 0: 32) and the 256 decoded values of a G.711 law as the kernel uses them
 * (VSP_ERR_ARG for VSP_IN_F32 / VSP_IN_S16, which have no table).  ceil(n L / M) is vsp_resample_out_len. */
#define VSP_IN_F32 0
#define VSP_IN_S16 1
#define VSP_IN_ULAW 2
#define VSP_IN_ALAW 3
#define VSP_INPUT_RATES_MAX 8
int vsp_input_plan(int in_rate, int model_rate, int zeros, int* L, int* M, int* half_len);
int vsp_input_filter(int in_rate, int model_rate, int zeros, double beta, double rolloff, float* taps_host);
int vsp_input_decode_table(int enc, float* table256);
/* Builds the filter of (in_rate -> model_rate) and uploads its table [P][L] (the output stage's layout) to the context's
 * device.  A context holds up to VSP_INPUT_RATES_MAX input rates at once (one more: VSP_ERR_STATE); configuring a rate again
 * replaces its table; model_rate == 0 drops the rate (VSP_OK also when it was not configured).  in_rate == model_rate
 * configures the pass-through.  May allocate and synchronise, like vsp_output_configure; the tables are freed by vsp_destroy. */
int vsp_input_configure(vsp_ctx* ctx, int in_rate, int model_rate, int zeros, double beta, double rolloff);
/* One row of vsp_input_rows: a window of one recording and the output samples to compute from it.  The descriptors live in
 * HOST memory, are read before the call returns and reach the device as kernel arguments. */
typedef struct vsp_input_row {
  const void* in;        /* DEVICE: raw samples [in_first, in_first + in_len) of the recording, in `enc` */
  int64_t in_first, in_len;
  int64_t n_total;       /* the recording's length in input samples once it has ended, -1 while it is open */
  float* out;            /* DEVICE: receives output samples [m0, m1) at out[0 .. m1 - m0) */
  int64_t m0, m1;
  int64_t out_fill;      /* >= m1 - m0: out[m1 - m0 .. out_fill) is written as exactly 0.0f */
} vsp_input_row;
/* 1 <= B <= 64 rows of one (in_rate, enc), one launch (two when the descriptors exceed the kernel-argument space; the caller
 * sees no difference).  No allocation, no synchronisation, caller's stream.  With (L, M, H) of the configured rate and
 *   complete(s, ended) = ended ? ceil(s L / M) : min(ceil(s L / M), max(0, ceil((L s - H) / M)))
 * (vispeech_amd.output_stage.complete_outputs), checked on the host before anything is launched:
 *   the rate is configured (VSP_ERR_STATE);
 *   enc is one of VSP_IN_*, rows non-NULL, `in` non-NULL (unless in_len == 0) and aligned to its element, `out` non-NULL
 *   (unless out_fill == 0), in_len >= 0, n_total >= -1 (VSP_ERR_ARG);
 *   0 <= in_first, 0 <= m0 <= m1 <= out_fill; a closed row (n_total >= 0): in_first + in_len <= n_total and
 *   m1 <= ceil(n_total L / M); an open row: m1 <= complete(in_first + in_len, open); every input sample of the recording
 *   that an output of [m0, m1) depends on, k in [0, n_total) with |m M - k L| <= H, lies in the window (VSP_ERR_SHAPE).
 * No sample outside the window and no sample at or behind n_total is read.  An output sample's value depends on (decoded x,
 * m) alone -- one thread per sample, fp32 FMAs in ascending k over the table -- not on the window, the tile or the batch:
 * outputs computed window by window are the bytes of the one-shot call (in_first = 0, in_len = n_total, m0 = 0,
 * m1 = ceil(n_total L / M)).  Between windows a caller keeps the raw samples from
 * vispeech_amd.output_stage.history_start(m1) on: at most vsp_output_history_samples(L, M, H) = floor(2 H / L) of them. */
int vsp_input_rows(vsp_ctx* ctx, void* stream, int in_rate, int enc, int B, const vsp_input_row* rows);

/* ---- output rows (round 17, ABI 7, additive) ------------------------------------------------ */
/* The output-side counterpart of vsp_input_rows: up to 64 rows per call, every row with its OWN output rate and encoding,
 * one launch (two when the descriptors exceed the kernel-argument space; the caller sees no difference).  The rates live in
 * a set of up to VSP_OUTPUT_RATES_MAX tables BESIDE the single stage of vsp_output_configure, which these calls neither read
 * nor change: the same filter formula, limits (L <= 320, M <= 441, 1 <= zeros <= 64), defaults (zeros == 0: 32;
 * rolloff <= 0: 1 - 3.065 / zeros) and table layout.
 *
 * A row is a piece [x_first, x_first + n) of one utterance at the model's rate; with (L, M, H) of its rate and the rule
 * published above for vsp_generator_stream_rows_output,
 *   m0 = complete(x_first, 0)          m1 = complete(x_first + n, ended)
 *   k0 = min(x_first, start(m0))       k1 = min(x_first + n, start(m1))
 * the call writes output samples [m0, m1) to out[0 .. m1 - m0), the encoding's silence to out[m1 - m0 .. out_fill), and input
 * samples [k1, x_first + n) to hist_out[0 ..); it reads input samples [k0, x_first) from hist_in.  Every call delivers
 * everything its input completes: no counter travels between calls.  Both histories hold K = vsp_output_history_samples(L,
 * M, H) floats; a request owns two and alternates.  The one-shot call is x_first = 0, n = total, ended = 1 with both
 * histories NULL (a row with ended == 1 may leave hist_out NULL: nothing follows it).  vsp_output_rows_plan is the host
 * arithmetic (any output may be NULL; VSP_ERR_ARG for L, M < 1, H, x_first, n < 0).
 *
 * Values.  Element j of a VSP_OUT_F32 row is, bit for bit, sample m0 + j of what vsp_output_chunk returns for the same
 * utterance when the single stage is configured with the same (model_rate, out_rate, zeros, beta, rolloff): the same table,
 * fp32 FMAs in ascending k.  VSP_OUT_S16 is the PCM16 rule of vsp_output_chunk on that value, s.  VSP_OUT_ULAW / VSP_OUT_ALAW
 * are the truncating G.711 compressors of s -- the inverses of the expanders published for VSP_IN_ULAW / VSP_IN_ALAW
 * (encode(decode(c)) == c for every code, except that mu-law's negative zero 0x7F comes back as 0xFF):
 *   mu-law  neg = s < 0;  mag = min(|s|, 32635) + 0x84;  e = floor(log2(mag)) - 7;  q = (mag >> (e + 3)) & 15;
 *           c = ~((neg ? 0x80 : 0) | e << 4 | q) & 0xFF
 *   A-law   neg = s < 0;  mag = (neg ? ~s : s) >> 3;  e = mag ? max(floor(log2(mag)) - 4, 0) : 0;
 *           q = e == 0 ? (mag >> 1) & 15 : (mag >> e) & 15;  c = ((neg ? 0 : 0x80) | e << 4 | q) ^ 0x55
 * Silence, the code of 0: 0.0f, 0, 0xFF, 0xD5.  A value depends on (samples, m, rate, enc) alone -- not on the split, the
 * tile, the other rows of the call or their formats.  vsp_output_encode is the compressor on the host (enc VSP_OUT_ULAW or
 * VSP_OUT_ALAW, n PCM16 values -> n code bytes; VSP_ERR_ARG otherwise). */
#define VSP_OUT_F32 0        /* the numbers of VSP_IN_* */
#define VSP_OUT_S16 1
#define VSP_OUT_ULAW 2
#define VSP_OUT_ALAW 3
#define VSP_OUTPUT_RATES_MAX 8
int vsp_output_encode(int enc, const int16_t* pcm, int64_t n, uint8_t* codes);
/* Builds the filter of (model_rate -> out_rate) and uploads its table into the context's set of output rates.  Configuring
 * a rate again replaces its table; model_rate == 0 drops out_rate (VSP_OK also when it was not configured); a ninth rate:
 * VSP_ERR_STATE.  May allocate and synchronise; the tables are freed by vsp_destroy. */
int vsp_output_rate_configure(vsp_ctx* ctx, int model_rate, int out_rate, int zeros, double beta, double rolloff);
typedef struct vsp_output_row {      /* HOST memory, read before the call returns */
  const float* x;                    /* DEVICE: the row's NEW input samples [x_first, x_first + n) at the model's rate */
  int64_t x_first, n;                /* n == 0 is legal only with ended == 1 (flush the tail) */
  int32_t ended;                     /* 1: the utterance ends at x_first + n */
  int32_t out_rate, enc;             /* a configured rate, one of VSP_OUT_* */
  const float* hist_in;              /* DEVICE: samples [k0, x_first) as the row's previous call wrote them */
  float* hist_out;                   /* DEVICE: receives samples [k1, x_first + n); differs from hist_in */
  void* out;                         /* DEVICE: receives output samples [m0, m1) as elements of `enc` */
  int64_t out_fill;                  /* >= m1 - m0 elements; out[m1 - m0 .. out_fill) is written as the encoding's silence */
} vsp_output_row;
int vsp_output_rows_plan(int L, int M, int H, int64_t x_first, int64_t n, int ended, int64_t* m0, int64_t* m1, int64_t* k0,
                         int64_t* k1);
/* 1 <= B <= 64.  No allocation, no synchronisation, caller's stream.  Decided on the host before anything is launched:
 *   rows non-NULL, 1 <= B <= 64, enc one of VSP_OUT_*, n >= 0, n > 0 unless ended, 0 <= x_first, out_fill >= 0 (VSP_ERR_ARG);
 *   the row's rate is configured (VSP_ERR_STATE);
 *   x non-NULL (unless n == 0), out non-NULL (unless out_fill == 0), hist_in non-NULL while x_first > k0, hist_out non-NULL
 *   while x_first + n > k1 and the row has not ended, every pointer aligned to its element, hist_in != hist_out
 *   (VSP_ERR_ARG);  m1 - m0 <= out_fill (VSP_ERR_SHAPE).
 * No sample outside a row's two segments is read; a refused call writes nothing. */
int vsp_output_rows(vsp_ctx* ctx, void* stream, int B, const vsp_output_row* rows);

/* ---- prosody (round 18, ABI 7, additive) ---------------------------------------------------- */
/* Per-phoneme F0 and energy of a recording: the producer of the pitch_control / energy_control tensors vsp_encode reads,
 * what the reference's data preparation (f0energy.py) computes with parselmouth and librosa.  The specification is this
 * project's own (restated in fp64 in tests/prosody_ref.py) and is NOT bit-compatible with parselmouth:
 * no sinc interpolation, and in the three calls of this section every frame decides for itself (the path finder is the
 * next section's, round 19).
 *
 * Constants: fs = VSP_PROSODY_FS, n_fft = VSP_PROSODY_NFFT; `hop` is the model's (512).  A row of n samples has
 * F(n) = n / hop + 1 frames, frame k centred on sample hop * k, and needs n >= n_fft / 2 + 1 (for the reflection).
 *   energy_k   reflect-pad the row by n_fft / 2 a side, s = x_pad[hop k .. hop k + n_fft) times the periodic Hann window;
 *              e_k = sqrt(sum over the n_fft / 2 + 1 one-sided DFT bins of |X|^2), computed without a DFT as
 *              sqrt((n_fft sum s^2 + (sum s)^2 + (sum (-1)^j s_j)^2) / 2).
 *   f0_k       Boersma's autocorrelation method on the W = round(3 fs / floor) (made even) samples around hop k, zeros outside
 *              the row: subtract their mean, lpk = max |s|, a = s w with w_j = 0.5 - 0.5 cos(2 pi (j + 0.5) / W),
 *              r(t) = (r_a(t) / r_a(0)) * fl32(r_w(0) / r_w(t)); candidates are the integer lags t in [floor(fs / ceiling),
 *              ceil(fs / floor)] with r(t) > r(t - 1) and r(t) >= r(t + 1), refined by a parabola (d, R), f = fs / (t + d),
 *              strength S = R + octave_cost log2(f / floor); unvoiced strength U = voicing_threshold + max(0, 2 - (lpk / gpk) /
 *              (silence_threshold / (1 + voicing_threshold))), gpk = the row's max |x - mean(x)|.  f0_k = f of the strongest
 *              candidate (the lowest lag among equals) if S > U, else 0; 0 also when r_a(0) = 0, gpk = 0 or no candidate.
 *   phonemes   F0: unvoiced frames between voiced ones are interpolated linearly, frames before the first voiced frame
 *              take its value, frames behind the last take the last; with fewer than two voiced frames the contour stays.
 *              Phoneme i of d_i > 0 frames gets the mean of its OWN frames [sum_{j<i} d_j, + d_i) of the interpolated
 *              F0 / of the energy, one of d_i = 0 gets 0.  (f0energy.py averages in place and so reads averaged values
 *              where sum_{j<i} d_j < i; this call averages the untouched contour.)
 * params NULL: floor 80 Hz, ceiling 750 Hz, voicing threshold 0.6, silence threshold 0.03, octave cost 0.01.
 * Refused (VSP_ERR_ARG): floor < 40 Hz (the window must fit in LDS), ceiling > fs / 4 or <= floor. */
#define VSP_PROSODY_FS 44100
#define VSP_PROSODY_NFFT 1280
typedef struct vsp_prosody_params {
  float floor_hz, ceiling_hz, voicing_threshold, silence_threshold, octave_cost;
} vsp_prosody_params;
/* F(n), host arithmetic only.  VSP_ERR_ARG: n_samples < n_fft / 2 + 1 or > 2^30, hop outside [1, 2048]. */
int vsp_prosody_frames(int64_t n_samples, int hop);
/* Workspace of either call below for B rows of up to L_max samples and Tp phonemes (VSP_ERR_ARG as a negative size). */
int64_t vsp_prosody_workspace_bytes(int B, int64_t L_max, int hop, int Tp, const vsp_prosody_params* params);
/* audio [B][audio_stride] float32 at fs (device, audio_stride >= L_max); n_samples_host [B]: HOST memory, read before the
 * call returns -- row b is audio[b][0 .. n_b), n_fft / 2 + 1 <= n_b <= L_max, and nothing at or behind n_b is read.
 * Outputs (device): f0_frames, energy_frames [B][F_max], F_max = F(L_max): row b's first F(n_b) columns, exact 0.0 behind;
 * frames [B] = F(n_b).  A row's result does not depend on the rows it is batched with.  Two launches (row peak,
 * contours) behind two small uploads into the workspace (the lengths and about 14 KB of window tables: copies from pageable
 * host memory, which the runtime stages before they return -- they block the host for the copy, and the call cannot be
 * captured into a graph); no allocation, no device synchronisation, caller's stream.
 * Every refusal is decided on the host before anything is launched and names the row. */
int vsp_prosody_contours(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int hop, const float* audio, int64_t audio_stride,
                         const int64_t* n_samples_host, const vsp_prosody_params* params, float* f0_frames,
                         float* energy_frames, int64_t* frames, void* workspace, int64_t workspace_bytes);
/* The contours of the call above (device, [B][F_max]) to per-phoneme means.  HOST memory, read before the call returns:
 * frames_host [B] (F(n_b)), durations_host [B][Tp] (frames per phoneme) and lengths_host [B] (phonemes per row); a row
 * needs 0 <= d and sum d <= frames_host[b] (VSP_ERR_ARG, naming the row).  Outputs (device): f0, energy [B][Tp], exact 0.0
 * for a phoneme of no frames and behind lengths_host[b].  One launch behind one upload of the same kind. */
int vsp_prosody_phonemes(vsp_ctx* ctx, void* stream, int B, int F_max, int Tp, const float* f0_frames, const float* energy_frames,
                         const int64_t* frames_host, const int64_t* durations_host, const int64_t* lengths_host, float* f0,
                         float* energy, void* workspace, int64_t workspace_bytes);

/* ---- prosody: the path finder (round 19, ABI 7, additive) ------------- */
/* The second half of Boersma's method (1993, section 2 step 4): several candidates per frame and the path through them
 * that maximises the summed strengths minus a cost per octave jumped and per voicing change, instead of every frame's own
 * decision.  Restated in fp64 in tests/prosody_path_ref.py.  S and U below are a frame's strengths exactly as above.
 *   candidates  A frame has 16 slots of (f, delta), N <= VSP_PROSODY_MAX_CANDIDATES of them used.  Slot 0 is the unvoiced
 *               candidate (0, U); slots 1 .. max_candidates - 1 are the strongest voiced candidates (f, S) in descending S, the
 *               lower lag first among equals; unused slots (slot 15 always) are (0, -inf).  A frame with r_a(0) = 0 or gpk = 0
 *               has slot 0 alone, with delta = voicing_threshold + 2.  Behind a row's frames both tables are exact 0.
 *   path        For a row of F frames, c_0 .. c_{F-1} maximising sum_k delta_k(c_k) - sum_{k>=1} T(c_{k-1}, c_k): T = 0 between two
 *               unvoiced candidates (f = 0), voiced_unvoiced_cost kappa between a voiced and an unvoiced one,
 *               octave_jump_cost kappa |log2(f_a / f_b)| between two voiced ones; kappa = fs / (100 hop) (0.861 at hop 512).
 *               s_0 = delta_0, s_k(c) = delta_k(c) + max_p (s_{k-1}(p) - T(p, c)), the lowest p among equals; every frame's s_k
 *               is then normalised by subtracting its maximum (the best entry is exactly 0.0f); the end takes the lowest c
 *               among equals.  f0_k = f of the chosen candidate, bit for bit.  With both costs 0 the path is the
 *               per-frame decision of vsp_prosody_contours in every bit.
 * One stated difference from Praat: its voiced strength is R - octave_cost log2(ceiling / f), this one's R + octave_cost
 * log2(f / floor): a constant octave_cost log2(ceiling / floor) (0.032 at the defaults) in favour of voiced.
 * path NULL: octave-jump cost 0.35, voiced/unvoiced cost 0.14, max_candidates 15.  Refused (VSP_ERR_ARG): a negative cost,
 * max_candidates outside [2, 15], and everything vsp_prosody_contours refuses -- on the host, before any launch. */
#define VSP_PROSODY_MAX_CANDIDATES 15
typedef struct vsp_prosody_path_params {
  float octave_jump_cost, voiced_unvoiced_cost;
  int32_t max_candidates;
} vsp_prosody_path_params;
/* Workspace of any of the three calls below (VSP_ERR_ARG as a negative size). */
int64_t vsp_prosody_path_workspace_bytes(int B, int64_t L_max, int hop, const vsp_prosody_params* params,
                                         const vsp_prosody_path_params* path);
/* The candidates alone: vsp_prosody_contours with the tables cand_f, cand_s [B][F_max][16] float32 (device) in place of
 * f0_frames; energy_frames and frames as there.  Two launches. */
int vsp_prosody_candidates(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int hop, const float* audio, int64_t audio_stride,
                           const int64_t* n_samples_host, const vsp_prosody_params* params, int max_candidates, float* cand_f,
                           float* cand_s, float* energy_frames, int64_t* frames, void* workspace, int64_t workspace_bytes);
/* The path alone, a stand-alone operator on any candidate tables [B][F_max][16] (device): delta finite or -inf, at least one
 * finite per frame, f = 0 for an unvoiced candidate.  frames_host [B]: HOST memory, 1 <= frames <= F_max; frames at or behind
 * frames_host[b] are not read.  f0_frames [B][F_max] (device): exact 0.0 behind a row's frames.  One launch, one wave per
 * row, behind one small upload; back-pointers (16 bytes a frame) go through the workspace. */
int vsp_prosody_path(vsp_ctx* ctx, void* stream, int B, int F_max, int hop, const float* cand_f, const float* cand_s,
                     const int64_t* frames_host, const vsp_prosody_path_params* path, float* f0_frames, void* workspace,
                     int64_t workspace_bytes);
/* Both: vsp_prosody_contours' arguments and `path`; the candidate tables live in the workspace.  Three launches. */
int vsp_prosody_contours_path(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int hop, const float* audio, int64_t audio_stride,
                              const int64_t* n_samples_host, const vsp_prosody_params* params, const vsp_prosody_path_params* path,
                              float* f0_frames, float* energy_frames, int64_t* frames, void* workspace, int64_t workspace_bytes);

/* ---- align: durations from a recording (round 20, ABI 7, additive) ---- */
/* Monotonic alignment of a recording to a text, the one control of vsp_encode this library could not produce from audio
 * (the reference takes it from the Montreal Forced Aligner).  Both sides meet in the prior's space: from the text,
 * vsp_encode + vsp_decode(max_len = 0) give m_p, logs_p [B][C][K_max] and cum_dur; from the recording,
 * vsp_convert_latent(noise_scale = 0) gives z_p [B][C][F_max].  The specification is this project's own, restated in fp64 in
 * tests/align_ref.py.  Row b has F_b frames (frames_host) and K_b states (states_host), a state being a frame of the template.
 *   scores     S[b][j][k] = sum_c -0.5 (x[b][c][j] - m[b][c][k])^2 exp(-2 logs[b][c][k]) - sum_c logs[b][c][k] for j < F_b, k < K_b
 *              (the C/2 log 2 pi constant is dropped), computed in the direct form -- the difference, then its square -- in
 *              fp32, c ascending whatever the batch.  S [B][F_max][K_max] float32: exact 0 outside a row's F_b x K_b; nothing
 *              outside a row's extent of x, m or logs is read.
 *   path       k(0) = 0, k(F - 1) = K - 1, k(j) - k(j - 1) in {0 .. max_advance}; the path maximises sum_j S[j][k(j)]
 *              - stay_cost #(advance 0) - skip_cost #(advance 2).  Q_0(0) = S[0][0], Q_0(k > 0) = -inf, Q_j(k) = S[j][k] +
 *              max(Q_{j-1}(k) - stay_cost, Q_{j-1}(k - 1), Q_{j-1}(k - 2) - skip_cost), the LOWEST advance among equals.  Q is
 *              accumulated in fp64 (the fp32 scores and costs widened exactly: subtractions, an exact max, one add), so the
 *              path is the fp64 restatement's on the same scores bit for bit, ties included.  Scores inside a row's extent
 *              must be finite.  states [B][F_max] int32: k(j), exact 0 behind a row's frames; scores behind a row's extent
 *              are not read.  A row needs K_b <= max_advance (F_b - 1) + 1 and K_b <= vsp_align_max_states().
 *   durations  cum_dur_host [B][Tp] int32 (HOST memory): the row's inclusive cumulative template frames as vsp_encode writes
 *              them (read back by the caller).  d_i = #{ j : cum_{i-1} <= k(j) < cum_i } -- the difference of two lower
 *              bounds over the monotone states --, 0 for a phoneme of no template frames and behind lengths_host[b];
 *              sum_i d_i = F_b where cum_dur ends at K_b.  durations [B][Tp] int32 (device).
 * params NULL: max_advance 2, both costs 0.  Refused with VSP_ERR_ARG on the host, before any launch, naming the row: an
 * infeasible row, max_advance outside {1, 2}, a negative cost, K_b above the state limit, F_b < 1 or > F_max, K_b < 1 or >
 * K_max, and (vsp_align) cum_dur[lengths - 1] != K_b; in vsp_align_durations and vsp_align also a row of no phonemes
 * (1 <= lengths_host[b] <= Tp) and a cum_dur that decreases.  frames_host, states_host, lengths_host: HOST arrays [B].
 * Each call runs on `stream` behind an upload of its rows (2 B int32; with durations also the phoneme map, B Tp int32),
 * allocates nothing and does not synchronise the stream.  The uploads read pageable host memory, as the prosody calls' do:
 * the host is held for the copy into the runtime's staging buffer, which is noticeable only for a large B Tp, and the
 * calls cannot be captured into a graph. */
typedef struct vsp_align_params {
  int32_t max_advance;
  float stay_cost, skip_cost;
} vsp_align_params;
/* The most states a row of vsp_align_path / vsp_align may have (4096). */
int vsp_align_max_states(void);
/* Workspaces (VSP_ERR_ARG as a negative size); each is monotone in every argument.  vsp_align_workspace_bytes covers
 * vsp_align and vsp_align_durations. */
int64_t vsp_align_scores_workspace_bytes(int B, int F_max, int K_max);
int64_t vsp_align_path_workspace_bytes(int B, int F_max, int K_max);
int64_t vsp_align_workspace_bytes(int B, int F_max, int K_max, int Tp);
/* The score matrix alone: x [B][C][F_max], m and logs [B][C][K_max] (device, channels first as the library returns
 * them).  One launch. */
int vsp_align_scores(vsp_ctx* ctx, void* stream, int B, int C, int F_max, int K_max, const float* x, const float* m, const float* logs,
                     const int64_t* frames_host, const int64_t* states_host, float* scores, void* workspace, int64_t workspace_bytes);
/* The path alone, a stand-alone operator on any score matrix [B][F_max][K_max] (device).  One launch, one block per row;
 * back-pointers (2 bits a cell) go through the workspace. */
int vsp_align_path(vsp_ctx* ctx, void* stream, int B, int F_max, int K_max, const float* scores, const int64_t* frames_host,
                   const int64_t* states_host, const vsp_align_params* params, int32_t* states, void* workspace,
                   int64_t workspace_bytes);
/* Per-phoneme durations of states [B][F_max] (device).  One launch, one thread per phoneme. */
int vsp_align_durations(vsp_ctx* ctx, void* stream, int B, int F_max, int Tp, const int32_t* states, const int64_t* frames_host,
                        const int32_t* cum_dur_host, const int64_t* lengths_host, int32_t* durations, void* workspace,
                        int64_t workspace_bytes);
/* All three: scores, path, durations; the score matrix and the back-pointers live in the workspace.  Three launches. */
int vsp_align(vsp_ctx* ctx, void* stream, int B, int C, int F_max, int K_max, int Tp, const float* x, const float* m, const float* logs,
              const int64_t* frames_host, const int64_t* states_host, const int32_t* cum_dur_host, const int64_t* lengths_host,
              const vsp_align_params* params, int32_t* states, int32_t* durations, void* workspace, int64_t workspace_bytes);

/* ---- loudness (round 21, ABI 7, additive) ---------------------------- */
/* The integrated loudness of ITU-R BS.1770-4 / EBU R 128 per row of a ragged batch of mono float32 recordings, a gain per
 * row derived from it and applied, all on the device.  The specification is this project's own, restated in fp64 in
 * tests/loudness_ref.py.  Row b is audio[b][0 .. n_b) at sample_rate = fs, 8000 <= fs <= 192000 (an argument: the
 * services pass the model's rate).
 *   K-weighting  two biquads in cascade, designed on the host in double for fs, both from zero state at the row's sample 0.
 *                Shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / fs),
 *                Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2; b = [Vh + Vb K/Q + K^2, 2 (K^2 - Vh),
 *                Vh - Vb K/Q + K^2] / a0, a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0].  High-pass: f0 = 38.13547087602444,
 *                Q = 0.5003270373238773, b = [1, -2, 1], a from its own K as above.  At 48 kHz these are BS.1770's tables.
 *   segments     h = (fs + 5) / 10 in integers (100 ms); S = ceil(n / h); seg[s] = the sum of y^2 over the filtered row's
 *                samples [s h, min((s + 1) h, n)), a double.  States and sums are carried in double.
 *   blocks       n >= 4 h: NB = n / h - 3 (complete 400 ms blocks, 75 % overlap), E_j = ((seg[j] + seg[j+1]) + seg[j+2]) +
 *                seg[j+3], D = 4 h.  n < 4 h: NB = 1, E_0 = the row's segments summed ascending, D = n.
 *   gates        in double, means over ascending j.  Block j passes the absolute gate iff E_j / D > Z_abs = 10^((-70 + 0.691) /
 *                10); mean_abs = the mean E_j of those; j is kept iff it passes and 10 E_j > mean_abs (strict: the relative
 *                gate at -10 LU).  L = -0.691 + 10 log10(mean of the kept E_j / D) as float32; -inf where none is kept.
 *                blocks[b] = (NB, kept); peak[b] = max |x| (float32, exact; the SAMPLE peak).
 *   gain         g = 10^((target_lufs - L) / 20), then min(g, 10^(max_gain_db / 20)), then min(g, peak_ceiling / peak) where
 *                peak > 0; g = 1 exactly for a row with L = -inf and for a row whose target_lufs is NaN ("leave this row
 *                alone": apply neither reads nor writes it).
 *   apply        out[b][i] = fl32(g_b x[b][i]) for i < n_b, in place or into another buffer.
 * Nothing at or behind n_b is read or written (a NaN there changes no output bit); a row's bits do not depend on the rows it
 * is batched with; seg holds exact zeros behind a row's segments.  Refused with VSP_ERR_ARG on the host before any launch,
 * naming the row: n_b < 1 or > L_max (the gate: > S_max h), fs out of range, peak_ceiling <= 0, a negative or NaN
 * max_gain_db; a workspace too small is VSP_ERR_WORKSPACE.  Each call runs on `stream` behind ONE upload of its rows (20
 * bytes a row: the lengths and the params, pageable host memory as the prosody calls'), allocates nothing and does not
 * synchronise.  n_samples_host, params_host: HOST arrays [B].
 * Not computed: true peak (sample peak only; the meter of a later section has it), stereo and channel weights.  Momentary,
 * short-term and running loudness: "loudness over time" below; loudness range: the section behind it. */
typedef struct vsp_loudness_params {
  float target_lufs, peak_ceiling, max_gain_db;
} vsp_loudness_params;
/* coef[10] = the shelf's b0 b1 b2 a1 a2, then the high-pass's.  Host only. */
int vsp_loudness_kweighting(int sample_rate, double* coef);
/* S(n) = ceil(n / h), host only (VSP_ERR_ARG as a negative count: n outside [1, 2^30], fs out of range). */
int64_t vsp_loudness_segments_count(int64_t n_samples, int sample_rate);
/* Workspace of any call below for B rows of up to L_max samples (VSP_ERR_ARG as a negative size); monotone in B and L_max. */
int64_t vsp_loudness_workspace_bytes(int B, int64_t L_max, int sample_rate);
/* audio [B][audio_stride] (device, audio_stride >= L_max) to seg [B][S_max] double, S_max = S(L_max), and peak [B] float32
 * (device).  Three launches: segment end states from zero (one wave per row and segment), the states carried along each row
 * (one wave per row), segment energies from the true states. */
int vsp_loudness_segments(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride,
                          const int64_t* n_samples_host, double* seg, float* peak, void* workspace, int64_t workspace_bytes);
/* The gates alone, a stand-alone operator on ANY double table seg [B][S_max] (device) with the rows' n_samples_host
 * (1 <= n_b <= S_max h): lufs [B] float32, blocks [B][2] int32.  With params_host (else NULL) also gains [B] float32 from
 * peak [B] (device).  One launch, one wave per row. */
int vsp_loudness_gate(vsp_ctx* ctx, void* stream, int B, int S_max, int sample_rate, const double* seg, const int64_t* n_samples_host,
                      const float* peak, const vsp_loudness_params* params_host, float* lufs, int32_t* blocks, float* gains,
                      void* workspace, int64_t workspace_bytes);
/* out = gains[b] in over each row's own samples; in == out is allowed.  params_host (or NULL: every row): a row whose
 * target_lufs is NaN is neither read nor written.  One launch; 16-byte accesses where both rows are 16-byte aligned. */
int vsp_loudness_apply(vsp_ctx* ctx, void* stream, int B, int64_t L_max, const float* in, int64_t in_stride, float* out,
                       int64_t out_stride, const int64_t* n_samples_host, const float* gains, const vsp_loudness_params* params_host,
                       void* workspace, int64_t workspace_bytes);
/* All three behind one upload: segments, gate and gains, apply (five launches); seg lives in the workspace; lufs, peak and
 * gains [B] stay on the device, so no host read sits between measuring and applying.  blocks may be NULL. */
int vsp_loudness_normalize(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride,
                           float* out, int64_t out_stride, const int64_t* n_samples_host, const vsp_loudness_params* params_host,
                           float* lufs, float* peak, float* gains, int32_t* blocks, void* workspace, int64_t workspace_bytes);

/* ---- loudness over time (round 23, ABI 7, additive) ------------------ */
/* Momentary, short-term and running integrated loudness per 100 ms of a row or of a STREAM, and a causal leveller steered
 * by the running level.  The specification is this project's own, restated in fp64 in tests/loudness_time_ref.py.  A row
 * (or stream) is x[0 .. n), mono float32 at fs.  h, the K-weighting, seg[s], the block energy E_j, Z_abs and both gates are
 * those of "loudness" above, unchanged.  F = n / h in integers: the COMPLETE segments.
 *   per complete segment s = 0 .. F - 1, float32:
 *     M[s]     momentary, 400 ms: s >= 3: -0.691 + 10 log10(E_(s-3) / (4 h)); -inf for s < 3 or E = 0.
 *     S[s]     short-term, 3 s: s >= 29: -0.691 + 10 log10(T_s / (30 h)), T_s = seg[s-29] + ... + seg[s] summed ascending
 *              from 0 in double; -inf before that or for T = 0.
 *     I[s]     running integrated: L of "loudness" above over the first (s + 1) h samples (for s < 3 its one-block rule);
 *              kept[s] (int32) that prefix's kept count.
 *   per row    M_max, S_max (-inf where there are none); I_end = L of the whole row.
 *   leveller   per row target_lufs (NaN: the row is neither read nor written), max_gain_db >= 0, max_cut_db >= 0,
 *              slew_db_per_s > 0, initial_gain_db; d = fl32(slew_db_per_s / 10).  The gain in dB per segment, float32 adds,
 *              subtracts, mins and maxes only:
 *                q[s] = c_dB[s-1] if I[s] = -inf, else min(max(fl32(target - I[s]), -max_cut_db), max_gain_db)
 *                c_dB[s] = c_dB[s-1] + min(max(q[s] - c_dB[s-1], -d), d),  c_dB[-1] = initial_gain_db
 *                c[s] = fl32(10^(c_dB[s] / 20))  (the only transcendental; c[-1] likewise from initial_gain_db)
 *   apply      sample i = s h + k, 0 <= k < h, in any segment, the row's partial last one included: c0 = c[s-2], c1 =
 *              c[s-1] (indices below 0 read c[-1]); w = fl32(fl32(k + 1) rh), rh = fl32(1 / h); a = fl32(c0 + fl32(fl32(c1 -
 *              c0) w)); out[i] = fl32(a x[i]).  No product is fused with a sum.  A steady level gives a == c0 exactly.
 * The gain over segment s depends on x[0 .. s h) only: no look-ahead, no added delay, and a sample can leave in the call
 * it arrives in.  The leveller does not clamp; a limiter behind it runs on its output.
 * Nothing at or behind n_b is read or written; a row's bits do not depend on its batch; and a stream's table entries and
 * levelled samples are, bit for bit, those of the one call on the whole row, under ANY split: entry s is computed from
 * seg[0 .. s] in an order that depends on s alone, and the K-weighting's state crosses calls in double, exactly as it
 * crosses segments.  The cost of entry s grows with s (both gate passes run over the prefix's blocks).
 * Rows of time, level_gains and level_apply are described by pointers of their own (streams allocated apart advance in one
 * call); every table starts at the row's segment 0.  Refused with VSP_ERR_ARG on the host before any launch, naming the
 * row: a piece that does not start on a segment boundary, first + count above the table, a negative or NaN max_gain_db or
 * max_cut_db, slew_db_per_s not above 0, a non-finite initial_gain_db, fs out of range; a workspace too small is
 * VSP_ERR_WORKSPACE.  Each call runs on `stream` behind ONE upload, allocates nothing and does not synchronise.
 * Not computed: stereo, steering by the short-term level.  Loudness range, and a running level at a constant cost per
 * entry: "loudness range and the histogram gate" below. */
typedef struct vsp_loudness_level_params {
  float target_lufs, max_gain_db, max_cut_db, slew_db_per_s, initial_gain_db;
} vsp_loudness_level_params;
typedef struct vsp_loudness_row {
  const double* seg;            /* time: the row's segment energies, from segment 0 (device, as every pointer here) */
  float *M, *S, *I;             /* time writes them; level_gains reads I */
  int32_t* kept;                /* time */
  float *c_db, *c;              /* level_gains writes them (and reads c_db[first - 1]); level_apply reads c */
  int64_t first, count;         /* time, level_gains: the entries [first, first + count) */
  int64_t entries;              /* time, level_gains: the entries the row's tables can hold; level_apply: the entries of c that are valid */
  const float* in;              /* level_apply: the stream's samples [pos, pos + samples) */
  float* out;                   /* level_apply: receives them levelled; may be `in` */
  int64_t pos, samples;
} vsp_loudness_row;
/* Workspace of any call of this section for B rows of up to L_max samples (VSP_ERR_ARG as a negative size); monotone in B
 * and L_max.  time, level_gains and level_apply need that of L_max = 1. */
int64_t vsp_loudness_time_workspace_bytes(int B, int64_t L_max, int sample_rate);
/* vsp_loudness_segments carried across calls: row b is the piece audio[b][0 .. n_b) of a stream, starting at the stream's
 * sample first_host[b] (HOST [B]; NULL: 0), which must be a multiple of h.  state_in [B][4] double (device; NULL: zero):
 * the K-weighting's state in front of the piece; state_out [B][4] (device; NULL: not wanted; may be state_in): the state
 * behind the piece's last COMPLETE segment (state_in where it has none).  seg [B][S(L_max)] and peak [B] are those of the
 * piece.  The same three launches; with both states NULL, vsp_loudness_segments in every bit. */
int vsp_loudness_segments_from(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride,
                               const int64_t* n_samples_host, const int64_t* first_host, const double* state_in, double* state_out,
                               double* seg, float* peak, void* workspace, int64_t workspace_bytes);
/* The table operator alone, on ANY double tables: M, S, I, kept [first, first + count) of every row from its seg[0 .. first +
 * count).  m_max, s_max: [B] float32 (device), the largest M and S among THIS call's entries (-inf where none), or both
 * NULL.  One launch, one wave per (row, entry), and one for the maxima.  rows_host: HOST [B]. */
int vsp_loudness_time(vsp_ctx* ctx, void* stream, int B, int sample_rate, const vsp_loudness_row* rows_host, float* m_max, float* s_max,
                      void* workspace, int64_t workspace_bytes);
/* c_db, c [first, first + count) of every row from ANY table I, continuing from c_db[first - 1] of the row's own table
 * (initial_gain_db at first = 0): nothing is read back.  One launch, one lane per row. */
int vsp_loudness_level_gains(vsp_ctx* ctx, void* stream, int B, const vsp_loudness_row* rows_host,
                             const vsp_loudness_level_params* params_host, void* workspace, int64_t workspace_bytes);
/* The samples [pos, pos + samples) of every row against its c table, which must hold (pos + samples - 1) / h entries.  One
 * launch; 16-byte accesses where in and out are 16-byte aligned. */
int vsp_loudness_level_apply(vsp_ctx* ctx, void* stream, int B, int sample_rate, const vsp_loudness_row* rows_host,
                             const vsp_loudness_level_params* params_host, void* workspace, int64_t workspace_bytes);
/* Whole rows audio[b][0 .. n_b) behind one upload: segments, L of the row (i_end), the time tables, and with params_host
 * (else NULL: a meter; out, c_db and c are not used) gains and apply.  M, S, I, kept, c_db, c: [B][table_stride], table_stride >=
 * L_max / h, written for s < F_b only; m_max, s_max, i_end, peak: [B] float32.  seg lives in the workspace. */
int vsp_loudness_level(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride, float* out,
                       int64_t out_stride, const int64_t* n_samples_host, const vsp_loudness_level_params* params_host, float* M, float* S,
                       float* I, int32_t* kept, float* c_db, float* c, int64_t table_stride, float* m_max, float* s_max, float* i_end,
                       float* peak, void* workspace, int64_t workspace_bytes);

/* ---- loudness range and the histogram gate (round 24, ABI 7, additive) */
/* Loudness range (EBU Tech 3342) and a running integrated level whose cost per entry does not grow with the stream, both
 * from histograms of block loudness in 0.1 LU bins over -70 .. +30 LUFS.  The specification is this project's own, restated
 * in numpy in tests/loudness_hist_ref.py.  h, the K-weighting, seg[s], M[s], S[s] and F are those of "loudness over time"
 * above, unchanged and in the same bits.  All arithmetic is in double unless stated.
 *   tables     NB = 1000 bins; edges e_k = pow(10, (k - 693.09) / 100), k = 1 .. 1000, and e_0 = Z_abs by the expression of
 *              "loudness" above (the formula at k = 0 is the same number with its exponent rounded another way, 2e-15 off:
 *              both gates share one absolute gate in every bit); bin k covers [-70 + k/10, -70 + (k+1)/10) LUFS; centres
 *              c_k = pow(10, (k - 692.59) / 100), k = 0 .. 999.  Built on the host; the same bits travel to the device
 *              with every call.
 *   binning    a mean square z is not counted where !(z >= e_0) (the absolute gate); else its bin is the largest k <= 999
 *              with e_k <= z, found by comparisons against the edges only (no logarithm: a bin cannot flip on a
 *              transcendental's last bit).  Everything at or above e_999 lands in bin 999.
 *   histograms two per row, int32 [2][1000]: HB counts the 400 ms blocks -- the one ending at segment s >= 3 has z = E /
 *              (4 h), E as M[s]'s --, HS the 3 s windows -- the one ending at s >= 29 has z = T_s / (30 h).
 *   I_h[s]     float32, from HB after the entries 0 .. s: n_abs = sum HB[k]; mean_abs = sum HB[k] c_k / n_abs; bin k is kept
 *              iff 10 c_k > mean_abs (strict); kept[s] = the kept count; I_h[s] = fl32(-0.691 + 10 log10(sum_kept HB[k] c_k /
 *              kept[s])), -inf with kept[s] = 0 where nothing is kept (always for s < 3: no one-block rule here).  The sums
 *              run in an order that depends on k alone, so I_h[s] is a function of the counts.
 *   range      from HS after the row's last entry: mean = sum HS[k] c_k / sum HS[k]; bin k is kept iff 100 c_k > mean (the
 *              relative gate at -20 LU); N the kept count; in integers lo = (N + 4) / 10, hi = (95 (N - 1) + 50) / 100; k10
 *              (k95) the smallest kept k whose cumulative kept count exceeds lo (hi); LRA = fl32(k95 - k10) / 10.f; 0 for N = 0.
 * The state of a stream is integer counts and every value above a function of them, so any split of a stream gives the bits
 * of the one call; the work of an entry does not depend on s.  Against the exact gate of "loudness over time": where every
 * prefix's blocks stay a factor 1.05 clear of both gates, kept[s] agrees and |I_h[s] - I[s]| <= 0.05 LU for s >= 3 (half a
 * bin).  The exact gate is the default everywhere and is unchanged.
 * Refusals, the ONE upload (here with the tables: 16 KiB), no allocation and no synchronisation: as "loudness over time". */
#define VSP_LOUDNESS_HIST_BINS 1000
/* edges[1001], centres[1000].  Host only. */
int vsp_loudness_hist_tables(double* edges, double* centres);
/* Workspace of any call of this section for B rows of up to L_max samples (VSP_ERR_ARG as a negative size); monotone in B
 * and L_max.  vsp_loudness_time_hist needs that of L_max = 1. */
int64_t vsp_loudness_hist_workspace_bytes(int B, int64_t L_max, int sample_rate);
/* vsp_loudness_time under the histogram gate: the entries [first, first + count) of M, S (its bits), I = I_h and kept.
 * hist_host: a HOST array of B device pointers to [2][1000] int32 (HB, then HS), none NULL; a histogram is read as the
 * state after the entries [0, first) -- at first == 0 it is taken as zero, whatever it holds -- and left as the state after
 * first + count.  lra [B] float32 (device) or NULL: the range after the call's last entry.  m_max, s_max as there.  One
 * launch, one wave per row, and one for the maxima. */
int vsp_loudness_time_hist(vsp_ctx* ctx, void* stream, int B, int sample_rate, const vsp_loudness_row* rows_host, int32_t* const* hist_host,
                           float* m_max, float* s_max, float* lra, void* workspace, int64_t workspace_bytes);
/* Whole rows audio[b][0 .. n_b) behind one upload: the three segment launches, then the histogram launch from zero
 * histograms, which live in the workspace as seg does.  lra [B]; i_hist [B] or NULL: I_h[F - 1], -inf for F = 0; M, S, I,
 * kept [B][table_stride], table_stride >= L_max / h, written for s < F_b only: all four or all four NULL. */
int vsp_loudness_range(vsp_ctx* ctx, void* stream, int B, int64_t L_max, int sample_rate, const float* audio, int64_t audio_stride,
                       const int64_t* n_samples_host, float* lra, float* i_hist, float* M, float* S, float* I, int32_t* kept,
                       int64_t table_stride, void* workspace, int64_t workspace_bytes);

/* ---- true peak and look-ahead limiter (round 22, ABI 7, additive) --- */
/* A true-peak meter and a look-ahead limiter without a recurrence, per row of a ragged batch of mono float32 rows or of a
 * set of streams, on the device.  The specification is this project's own, restated in fp64 in tests/limiter_ref.py.  A
 * row is x[0 .. N), zero outside.
 *   true peak    4x oversampling with the resampling core's filter formula ("output stage" above) at L = 4, M = 1,
 *                zeros = 12, beta = 9.62, the default rolloff: H = 48, 97 taps h[-48 .. 48] computed in double and rounded
 *                to float32 once.  y[m] = sum_k h[m - 4 k] x[k] over |m - 4 k| <= 48, a float32 FMA chain from 0 in
 *                ascending k (reach J = 12 samples a side).  p[n] = max(|x[n]|, |y[4n]|, |y[4n+1]|, |y[4n+2]|, |y[4n+3]|);
 *                TP = max_n p[n].  (|x[n]| is in the max because the low-pass attenuates a lone click.)
 *   gain wanted  e[n] = g p[n]; r[n] = e[n] > c ? c / e[n] : 1 inside the row, 1 outside it (float32, IEEE division).
 *   hold, look-ahead   m[n] = min r[j], j = n - H .. n + A.
 *   smoothing    s[n] = (m[n - A] + ... + m[n]) * fl32(1 / (A + 1)): a float32 sum from 0 in ascending order.
 *   output       o[n] = clamp((g x[n]) s[n], -c, c) in float32.  s[n] <= r[n] in exact arithmetic (every m[k] summed has n
 *                in its own window), so |o[n]| <= c at the samples and the clamp only removes a last-place rounding.
 * A (attack = look-ahead, 0 .. 1024 samples) and H (hold, 0 .. 8192 samples) are per call; the ceiling c > 0 and the static
 * gain g are per row.  o[n] depends on x[n - (A + H + J) .. n + A + J] and on nothing else, so a stream is limited exactly
 * in pieces: vsp_limiter_history gives the two extents.  The true peak of the OUTPUT may exceed c slightly (the varying
 * gain spreads the spectrum; measured about 0.01 dB on the tests' fixtures): the sample ceiling is exact, the true-peak
 * ceiling is not promised.
 * Nothing outside a row's provided samples is read and nothing outside its outputs is written; a row's bits do not depend
 * on the rows it is batched with, nor on how a stream is cut.  Every refusal happens on the host before any launch, naming
 * the row.  Each call runs on `stream` behind ONE upload of its rows (pageable host memory), allocates nothing and does
 * not synchronise. */
typedef struct vsp_limiter_row {
  const float* in;      /* device: the stream's samples [first, first + count) */
  int64_t first, count;
  float* out;           /* device: receives the limited samples [out_first, out_first + out_count); may alias `in` at the same positions */
  int64_t out_first, out_count;
  int64_t total;        /* the stream's length, or -1 while its end is unknown */
  float ceiling;        /* c > 0; NaN: the row is neither read nor written */
} vsp_limiter_row;
/* taps97_host[n + 48] = fl32(h[n]), n = -48 .. 48.  Host only. */
int vsp_true_peak_filter(float* taps97_host);
/* *behind = A + H + J, *ahead = A + J, J = 12: the samples before an output and after it that reach it.  Host only;
 * VSP_ERR_ARG for A outside [0, 1024] or H outside [0, 8192]. */
int vsp_limiter_history(int A, int H, int64_t* behind, int64_t* ahead);
/* Workspace of vsp_limiter_rows for B rows of up to L_max OUTPUTS each (VSP_ERR_ARG as a negative size); monotone in every
 * argument.  vsp_true_peak needs vsp_limiter_workspace_bytes(B, 1, 0, 0). */
int64_t vsp_limiter_workspace_bytes(int B, int64_t L_max, int A, int H);
/* tp[b] = the true peak of audio[b][0 .. n_b), [B] float32 on the device (audio_stride >= L_max >= n_b >= 1).  One launch
 * behind a memset: tiles x rows, the block's maximum folded into tp[b] by an unsigned maximum on the float's bits (exact,
 * independent of the order).  A row whose peak is a sample value reads that value in every bit. */
int vsp_true_peak(vsp_ctx* ctx, void* stream, int B, int64_t L_max, const float* audio, int64_t audio_stride,
                  const int64_t* n_samples_host, float* tp, void* workspace, int64_t workspace_bytes);
/* The limiter over B rows, each at its own position of its own stream; rows_host: HOST array [B].  gains: [B] float32 on
 * the DEVICE (as vsp_loudness_gate leaves them), or NULL for 1.  min_gain: [B] float32 on the device, or NULL: the smallest
 * s[n] among the row's outputs of this call (1 for a row left alone): how hard the row was limited.  Two launches: r into
 * the workspace (with A + H values before and A behind the outputs), then sliding minimum, boxcar, product and clamp.
 * VSP_ERR_ARG when
 *   first > max(0, out_first - behind): history is missing;
 *   first + count < out_first + out_count + ahead while the provided samples do not reach the stream's end (total unknown,
 *   or total > first + count): look-ahead is missing;
 *   the outputs are not among the provided samples, the samples lie behind `total`, a position or count is negative or
 *   above 2^30, a pointer of a row that has samples (outputs) is NULL, the ceiling is not above 0, A or H is out of range.
 * A whole utterance of n samples is first = out_first = 0, count = out_count = total = n. */
int vsp_limiter_rows(vsp_ctx* ctx, void* stream, int B, int A, int H, const vsp_limiter_row* rows_host, const float* gains,
                     float* min_gain, void* workspace, int64_t workspace_bytes);

/* ---- denoiser and inverse STFT (round 25, ABI 7, additive) ----------- */
/* Subtracts the generator's zero-input spectrum (the "bias" of the denoisers shipped with WaveGlow and HiFi-GAN) from
 * every STFT frame of a waveform and returns to audio by weighted overlap-add, per row of a ragged batch.  The
 * specification is this project's own, restated in fp64 in tests/denoiser_ref.py.  Geometry: N = 2 (spec_channels - 1),
 * hop = the generator's total upsampling, the periodic Hann window of the spectrogram front end, pad = (N - hop) / 2 with
 * reflection at the row's own two ends, T(n) = vsp_convert_frames(n, hop).
 *   analysis     X[r][t] = sum_n hann[n] xp[t hop + n] e^{-2 pi i r n / N}, r = 0 .. N / 2: the frames and the convolution
 *                of vsp_spectrogram_ragged.
 *   subtraction  m = sqrt(re^2 + im^2); q = max(m - s_b beta_b[r], 0) / m (0 where m = 0); X' = q X.
 *   synthesis    v_t[n] = hann[n] (1 / N) sum_r w_r Re(X'[r][t] e^{+2 pi i r n / N}), w_0 = w_{N/2} = 1, else 2;
 *                yp[p] = (sum_t v_t[p - t hop]) / W[p], W[p] = sum_t hann^2[p - t hop] over the row's OWN frames covering
 *                p, both sums in ascending t; out[b][i] = yp[pad + i], 0 <= i < n_b.
 * Every call refuses with VSP_ERR_ARG, before any launch, a context without a spectrogram (spec_channels <= 1), one
 * whose hop does not divide N or whose N exceeds what a block of the overlap-add kernel stages; and, naming the row,
 * n_b <= pad, n_b > L_max, a negative or infinite strength, a NULL bias with any finite strength.  A row whose strength
 * is NaN is neither read nor written.  Nothing at or behind n_b is read or written; a row's bits do not depend on its
 * batch; in == out is allowed (the frames live in the workspace).  n_samples_host and strength_host are HOST arrays [B].
 * Each call runs on `stream` behind ONE upload of its rows (pageable host memory), allocates nothing and does not
 * synchronise.  T_max = vsp_convert_frames(L_max, hop). */
/* Frame operand [B][N][T_max], RI [B][2 spec][T_max], synthesis frames [B][N][T_max] (T_max padded to 64 columns) and the
 * upload; covers vsp_istft of the same shape.  VSP_ERR_ARG as a negative size. */
int64_t vsp_denoise_workspace_bytes(const vsp_ctx* ctx, int B, int L_max);
/* bias[s][r] = |sum_n hann[n] period[s][n mod hop] e^{-2 pi i r n / N}|, [S][spec] float32 on the device: each period
 * [hop] tiled to one column of the operand, the model.stft convolution, the exact magnitude (no 1e-6).  Workspace:
 * vsp_denoise_workspace_bytes(ctx, S, N) at least. */
int vsp_denoise_bias(vsp_ctx* ctx, void* stream, int S, const float* period, float* bias, void* workspace,
                     int64_t workspace_bytes);
/* The synthesis half alone: ri [B][2 spec][T_max] dense on the device (rows 0 .. spec - 1 real, then imaginary; columns at
 * or behind T(n_b) are not used) -> out[b][0 .. n_b).  The model.istft convolution, then the overlap-add kernel. */
int vsp_istft(vsp_ctx* ctx, void* stream, int B, int L_max, const float* ri, const int64_t* n_samples_host, float* out,
              int64_t out_stride, void* workspace, int64_t workspace_bytes);
/* bias: [B][spec] float32 on the device, row b's own.  Five launches: framing, the forward convolution, the subtraction in
 * place, the inverse convolution, overlap-add. */
int vsp_denoise(vsp_ctx* ctx, void* stream, int B, int L_max, const float* audio, int64_t audio_stride,
                const int64_t* n_samples_host, const float* bias, const float* strength_host, float* out, int64_t out_stride,
                void* workspace, int64_t workspace_bytes);

/* ---- denoiser for streams (round 26, ABI 7, additive) ---------------- */
/* The denoiser above over rows that are each a piece of a stream at its own position: a stream cut anywhere gives the bits
 * of vsp_denoise on the finished recording.  The operator has no recurrence.  With R = N / hop:
 *   frame t reads the samples [t hop - pad, t hop - pad + N), reflected at sample 0 always and at the stream's end `total`
 *   only once that end is known and reached;
 *   output j sits at padded position p = j + pad and sums the frames floor(p / hop) - (R - 1) .. floor(p / hop), clipped to
 *   [0, T(total)): it depends on the samples j - (N - 1) .. j + N - 1 and on nothing else;
 *   with n samples of an open stream, the frames t with t hop - pad + N <= n -- Tc(n) of them -- are frames of the finished
 *   recording whatever its length, and the outputs [0, E(n)), E(n) = max(0, Tc(n) hop - pad), are final: a delay n - E(n)
 *   between N - hop and N - 1 samples (1536 .. 2047 for the default model: 35 .. 46 ms at 44.1 kHz);
 *   to go on from output E(n) a stream keeps its samples from E(n) - (N - hop) on.
 * The call is stateless: it frames, transforms, subtracts and overlap-adds the window of frames its outputs need -- up to
 * R - 1 frames a row that an earlier call computed too -- and carries nothing between calls.  The two DFT products run on
 * the form vsp_denoise uses, whose column does not depend on where in the operand it sits; each output's sum is one chain
 * from 0 in ascending t, as there. */
typedef struct vsp_denoise_row {
  const float* in;      /* device: the stream's samples [first, first + count) */
  int64_t first, count;
  float* out;           /* device: receives the outputs [out_first, out_first + out_count); may alias `in` at the same positions */
  int64_t out_first, out_count;
  int64_t total;        /* the stream's length, or -1 while its end is unknown */
  float strength;       /* >= 0; NaN: the row is neither read nor written */
} vsp_denoise_row;
/* *behind = N - hop, *ahead = N - 1: the samples before an output and after it that can reach it.  Host only; VSP_ERR_ARG for
 * a context without the denoiser's geometry. */
int vsp_denoise_history(const vsp_ctx* ctx, int64_t* behind, int64_t* ahead);
/* E(n_seen) above, or n_seen for a closed stream: the outputs that are final.  Host arithmetic only -- the ONE rule that
 * callers in any language share; VSP_ERR_ARG (negative) for n_seen < 0 or a context without the geometry. */
int64_t vsp_denoise_complete(const vsp_ctx* ctx, int64_t n_seen, int closed);
/* Workspace of vsp_denoise_rows for B rows of up to L_max OUTPUTS each: three int64 per row, then the frame operand, RI and
 * the synthesis frames for windows of ceil((L_max - 1) / hop) + R columns (the dry pass of the call's own sequence).
 * Monotone in both arguments; VSP_ERR_ARG as a negative size (1 <= B <= 64, 1 <= L_max <= 2^30). */
int64_t vsp_denoise_rows_workspace_bytes(const vsp_ctx* ctx, int B, int64_t L_max);
/* rows_host: HOST array [B], 1 <= B <= 64; bias: [B][spec] float32 on the device, row b's own.  Five launches -- the window
 * framing of vsp_convert_stream_rows, the forward convolution, the subtraction, the inverse convolution, overlap-add -- whose
 * row descriptors travel as kernel arguments: no upload, no allocation, no synchronisation.  The workspace must hold
 * vsp_denoise_rows_workspace_bytes(ctx, B, the largest out_count).  Exactly out[0 .. out_count) of every live row is
 * written; a row with out_count = 0 is not read.  VSP_ERR_ARG before any launch, naming the row, when
 *   total is known and not above pad;
 *   the row's samples start behind the first sample its frames read: at most `behind` before out_first (history is missing);
 *   its frames read past first + count while the samples do not reach a known end (look-ahead is missing);
 *   samples or outputs lie behind `total`, a position or count is negative or above 2^30, a pointer of a row that has
 *   samples (outputs) is NULL, the strength is negative or infinite, bias is NULL with any finite strength;
 * and for the geometries vsp_denoise refuses.  A whole utterance of n samples is first = out_first = 0, count = out_count =
 * total = n, and has the bits of vsp_denoise. */
int vsp_denoise_rows(vsp_ctx* ctx, void* stream, int B, const vsp_denoise_row* rows_host, const float* bias, void* workspace,
                     int64_t workspace_bytes);

/* ---- the denoiser's transform (round 27, ABI 7, additive) ------------ */
/* Which transform vsp_denoise, vsp_denoise_rows, vsp_denoise_bias and vsp_istft -- and their workspace-size functions, by
 * the same dry pass -- run between framing and overlap-add:
 *   VSP_STFT_DFT (the default)  the two products with the windowed DFT bases and the subtraction between them: the
 *                               launches and the bits of rounds 25 and 26.
 *   VSP_STFT_FFT                a real FFT of N points per frame in LDS (N / 2 complex points in five radix-4 passes and a
 *                               split step; twiddles and windows from fp64 tables in the arena): vsp_denoise and
 *                               vsp_denoise_rows run framing, ONE fused launch (window, forward, subtraction, inverse, window;
 *                               the spectrum never reaches memory) and overlap-add, vsp_istft the inverse launch and
 *                               overlap-add, vsp_denoise_bias the forward launch between its two kernels.  The sums are
 *                               those of the specification; their bits are an FFT's, not the product's.  Every frame is
 *                               transformed on its own, so the contracts of the product path hold unchanged: a row's bits do
 *                               not depend on its batch, a stream cut anywhere gives the bits of vsp_denoise under the
 *                               same transform.  The workspace is smaller (one frame tensor), never larger.
 * The switch belongs to the context and is read by each call; a bias should be made under the transform that subtracts it.
 * The spectrogram front end of voice conversion (vsp_spectrogram*, vsp_convert_*) ignores it.
 * vsp_set_stft_transform: VSP_ERR_ARG, with a message and before any launch, for an unknown kind, and for VSP_STFT_FFT on a
 * context without the denoiser's geometry or with N != 2048.  vsp_stft_transform: the kind in force. */
#define VSP_STFT_DFT 0
#define VSP_STFT_FFT 1
int vsp_set_stft_transform(vsp_ctx* ctx, int kind);
int vsp_stft_transform(const vsp_ctx* ctx);

/* ---- measurement -------------------------------------------------------------------------- */
/* When enabled, every launch of a profiled class is bracketed by a HIP event pair on the launch
 * stream.  vsp_profile_read_class synchronises those events and returns, since the last reset, for
 * one class: the number of launches, their summed duration in milliseconds, their summed
 * algorithmic FLOPs and their summed algorithmic bytes:
 *   VSP_PROF_GENERATOR  the generator's convolutions (conv_pre, ups, ResBlock convs / fused pairs):
 *                       FLOPs 2 * Cout * Cin * taps * columns * B; bytes = SURVEY.md 8d's
 *                       layer-boundary model, input once + output once per convolution, fp32 (a fused
 *                       pair is charged the two convolutions it replaces = 4 passes); bytes_ext adds
 *                       the residual / accumulate operand reads (5-6 passes per pair); bytes_moved
 *                       (ABI 7) is what the launch must move through HBM AS FUSED -- input, output,
 *                       residual and previous sum once each: 2-3 passes per fused pair or chain.
 *                       The layer-boundary model is the contract's algorithmic figure; it is NOT a
 *                       bound of a fused launch (single launches exceed the HBM peak under it), bytes_moved is.
 *                       A ragged batch (trimmed tails) is charged the frames each launch COMPUTES
 *                       (ABI 7; the plan is read back inside profiled passes: one host wait per generator call);
 *   VSP_PROF_ATTENTION  relative-position attention launches (reference attentions.py:148-179):
 *                       FLOPs 4 * H * T^2 (QK^T and PV) + 4 * H * T * (2 window + 1) (banded
 *                       relative terms) per utterance; bytes = q|k|v in + out;
 *   VSP_PROF_FRAME      every other conv1d launch (encoders, predictors, flow, projection).
 * Profiling costs two hipEventRecord per launch: time the headline with it OFF.
 * vsp_profile_read is the class VSP_PROF_GENERATOR (kept from ABI version 2). */
#define VSP_PROF_GENERATOR 0
#define VSP_PROF_ATTENTION 1
#define VSP_PROF_FRAME 2
#define VSP_PROF_CLASSES 3
int vsp_profile_enable(vsp_ctx* ctx, int on);
int vsp_profile_read(vsp_ctx* ctx, int64_t* launches, double* total_ms, double* total_flops, double* total_bytes,
                     int reset);
int vsp_profile_read_class(vsp_ctx* ctx, int cls, int64_t* launches, double* total_ms, double* total_flops,
                           double* total_bytes, double* total_bytes_ext, double* total_bytes_moved, int reset);
/* ABI 5: the same measurement per KERNEL FAMILY of one class (so that a bench line can name its dominant kernel and a
 * reader can recompute its figures from a rocprofv3 kernel-stats table).  family = kind | log2(channels / 32) << 3 for
 * the generator class (channels = the launch's OUTPUT channels), 0 elsewhere:
 *   VSP_FAM_CONV   one launch per convolution (g16_conv / g16_convp)      VSP_FAM_UPS    a transposed up-convolution
 *   VSP_FAM_PAIR   one launch per ResBlock conv pair (g16_pp at 128 channels, g16_pair at 64, g16_rw at 32)
 *   VSP_FAM_CHAIN  one launch per ResBlock (g16_rc / g16_chain)           VSP_FAM_PRE    conv_pre (+ cond)
 *   VSP_FAM_RB2    one launch per ResBlock2 block (g16_rb2; round 7)
 * Launches of at most 16 output channels (the last stage of a five-stage generator, g16_c16) carry level 7 in place of
 * log2(channels / 32).
 * Fills up to `max_families` slots (families that saw no launch since the last reset are skipped) and returns the
 * number filled (>= 0) or a negative error code.  Call it BEFORE the vsp_profile_read_class(..., reset = 1) of the
 * same class; it never resets. */
#define VSP_FAM_OTHER 0
#define VSP_FAM_CONV 1
#define VSP_FAM_UPS 2
#define VSP_FAM_PAIR 3
#define VSP_FAM_CHAIN 4
#define VSP_FAM_PRE 5
#define VSP_FAM_RB2 6
int vsp_profile_read_families(vsp_ctx* ctx, int cls, int max_families, int* family, int64_t* launches, double* total_ms,
                              double* total_flops, double* total_bytes, double* total_bytes_moved /* ABI 7, may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* VISPEECH_HIP_H */
