// C-ABI of libvispeech_hip (include/vispeech_hip.h): the context, its weights and setters, the stand-alone operators and
// the profile readers.  The launch sequences are in api_frame.hip, api_generator.hip and api_convert.hip (api_common.h).
#include "api_common.h"

using namespace vsp;

namespace vsp {

int check_ready(vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  if (!ctx->ready) return ctx->fail(VSP_ERR_STATE, "weights not finalised");
  return VSP_OK;
}

int check_vc(vsp_ctx* ctx) {
  const int rc = check_ready(ctx);
  if (rc) return rc;
  if (ctx->cfg.spec_channels <= 0) return ctx->fail(VSP_ERR_STATE, "context was created without spec_channels");
  if (!ctx->model.has_vc) return ctx->fail(VSP_ERR_STATE, "enc_q.* tensors were not loaded before vsp_finalize_weights");
  return VSP_OK;
}

}  // namespace vsp

extern "C" {

int vsp_abi_version(void) { return VSP_ABI_VERSION; }

int vsp_create(const vsp_config* cfg, int device, vsp_ctx** out) { return vsp_create_ex(cfg, 1, device, out); }

int vsp_create_ex(const vsp_config* cfg, int32_t resblock, int device, vsp_ctx** out) {
  if (!cfg || !out || (resblock != 1 && resblock != 2)) return VSP_ERR_ARG;
  vsp_ctx* ctx = new (std::nothrow) vsp_ctx();
  if (!ctx) return VSP_ERR_ARG;
  ctx->cfg = *cfg;
  ctx->resblock = resblock;
  ctx->device = device;
  // Second implementations kept under test (tests/test_hip_parity.py): VSP_FRAME=f32 / VSP_ATT=f32 / VSP_GENERATOR=f32
  // (f32 matrix core), VSP_FUSE_PAIRS=0 (one launch per convolution), VSP_CHAIN=<mask> (whole-ResBlock launches:
  // bit 0 = k3, 1 = k7, 2 = k11), and the opt-in reduced precision VSP_GENERATOR=f16.  Everything else that was a
  // knob while the kernels were being tuned is compiled out of the product build (-DVSP_EXPERIMENTS brings it back).
  if (const char* e = getenv("VSP_FRAME")) ctx->frame_f16s = strcmp(e, "f32") != 0;
  if (const char* e = getenv("VSP_ATT")) ctx->att_f16s = strcmp(e, "f32") != 0;
  // the generator mode is part of the plan (conv_pre / cond packing): parse it BEFORE plan_model
  bool want_f16 = false;
  if (const char* e = getenv("VSP_GENERATOR")) {
    if (!strcmp(e, "f32")) ctx->gen_mode = 0;
    want_f16 = !strcmp(e, "f16");
  }
  if (const char* e = getenv("VSP_FUSE_PAIRS")) ctx->fuse_pairs = atoi(e) != 0;
  if (const char* e = getenv("VSP_RB2_FUSE")) ctx->rb2_fuse = atoi(e) != 0;      // 0: ResBlock2 one launch per convolution (second implementation)
  if (const char* e = getenv("VSP_TIMG")) ctx->t_img = atoi(e) != 0;   // 0: ResBlock intermediates as fp32 tensors (second implementation)
  if (const char* e = getenv("VSP_PP")) ctx->pp_pairs = atoi(e) != 0;  // 0: the 128-channel stage's k3 / k7 pairs as two launches
  if (const char* e = getenv("VSP_PAIR")) ctx->pair_ring = !strcmp(e, "ring");
  if (const char* e = getenv("VSP_CHAIN_RING")) ctx->chain_ring = atoi(e) != 0;
  if (const char* e = getenv("VSP_CHAIN")) ctx->chain_mask = atoi(e);
  if (const char* e = getenv("VSP_RW64")) ctx->rw64 = atoi(e) != 0;               // 1: g16_rw64 for the 64-channel k3 pairs (opt-in)
  if (const char* e = getenv("VSP_TRIM_TAILS")) ctx->trim_tails = atoi(e) != 0;   // 0: every utterance runs to the padded length
  if (const char* e = getenv("VSP_TAIL_TABLE")) ctx->tail_table_on = atoi(e) != 0; // 0: no silence table (second implementation)
  if (const char* e = getenv("VSP_COLS")) ctx->cols = atoi(e) != 0;               // 0: no column-tile kernels (second implementation)
  if (const char* e = getenv("VSP_COLS_BLOCKS")) ctx->cols_blocks = atol(e);      // size limits of launch_conv's routing to them
  if (const char* e = getenv("VSP_COLS_MIN_BLOCKS")) ctx->cols_min_blocks = atol(e);
  if (const char* e = getenv("VSP_ACT_SCALE_LOG2")) {                             // model.h: the generator's activation scale
    const int l = atoi(e);
    ctx->act_scale = std::ldexp(1.f, l < 0 ? 0 : l > 8 ? 8 : l);
  }
  if (const char* e = getenv("VSP_EARLY_FL")) ctx->early_fl = atoi(e) != 0;
  if (const char* e = getenv("VSP_RB_STREAMS")) ctx->rb_streams = atoi(e);   // stage mask: ResBlock chains on side streams (opt-in, measured slower)
#ifdef VSP_EXPERIMENTS
  if (const char* e = getenv("VSP_ATT_KSPLIT")) ctx->att_ksplit = atoi(e);
  if (const char* e = getenv("VSP_CHUNK_MB")) ctx->chunk_mb = atof(e);
  if (const char* e = getenv("VSP_CHAIN_CH")) ctx->chain_ch = atoi(e);
  if (const char* e = getenv("VSP_CHAIN128")) ctx->chain128_mask = atoi(e);
#endif
  build_schema(ctx->cfg, ctx->schema, ctx->resblock);
  const int rc = plan_model(ctx);            // (falls back to gen_mode 0 when the channels-last kernels do not cover the config)
  if (want_f16 && ctx->gen_mode == 1) ctx->gen_mode = 2;   // opt-in reduced precision: same packing as mode 1
  *out = ctx;  // returned even on failure so that vsp_last_error can be read; caller destroys it
  return rc;
}

int vsp_destroy(vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
  for (auto e : ctx->sync_ev) (void)hipEventDestroy(e);
  if (ctx->fl_ev) (void)hipEventDestroy(ctx->fl_ev);
  if (ctx->fl_pinned) (void)hipHostFree(ctx->fl_pinned);
  if (ctx->flags_host) (void)hipHostFree(ctx->flags_host);
  for (auto st : ctx->side) if (st) (void)hipStreamDestroy(st);
  if (ctx->arena && ctx->arena_owned) (void)hipFree(ctx->arena);
  if (ctx->out_stage.tab) (void)hipFree(ctx->out_stage.tab);
  tail_table_drop(ctx);
  for (auto& r : ctx->in_rates) if (r.tab) (void)hipFree(r.tab);
  for (auto& r : ctx->out_rates) if (r.tab) (void)hipFree(r.tab);
  delete ctx;
  return VSP_OK;
}

const char* vsp_last_error(const vsp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int vsp_status(vsp_ctx* ctx, unsigned* flags, int clear) {
  if (!ctx || !flags) return VSP_ERR_ARG;
  *flags = 0u;
  if (!ctx->flags_host) return VSP_OK;                 // (nothing has run on this context yet)
  volatile unsigned* w = ctx->flags_host;
  *flags = clear ? __atomic_exchange_n(ctx->flags_host, 0u, __ATOMIC_ACQ_REL) : *w;
  return VSP_OK;
}

int vsp_begin_weights(vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  ctx->raw.clear();
  ctx->ready = false;
  ctx->adopted_pending = false;
  tail_table_drop(ctx);
  return VSP_OK;
}

int vsp_set_weight(vsp_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim) {
  if (!ctx || !key || !host_data || !shape || ndim < 0 || ndim > 8) return ctx ? ctx->fail(VSP_ERR_ARG, "null argument") : VSP_ERR_ARG;
  const std::string k(key);
  // posterior encoder: voice conversion only; ignored by a context built without spec_channels
  if (k.rfind("enc_q.", 0) == 0 && ctx->cfg.spec_channels <= 0) return VSP_OK;
  auto it = ctx->schema.find(k);
  bool folded_form = false;
  if (it == ctx->schema.end()) {
    // accept a pre-folded "<x>.weight" where the schema has "<x>.weight_v" (remove_weight_norm'ed checkpoint)
    auto iv = ctx->schema.find(k + "_v");
    if (iv == ctx->schema.end()) return ctx->fail(VSP_ERR_KEY, "unknown state_dict key '%s'", key);
    it = iv;
    folded_form = true;
  }
  const SchemaEntry& e = it->second;
  bool same = (int)e.shape.size() == ndim;
  for (int i = 0; same && i < ndim; ++i) same = e.shape[i] == shape[i];
  if (!same) return ctx->fail(VSP_ERR_SHAPE, "shape mismatch for '%s'", key);
  if (!e.used) return VSP_OK;
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  t.data.assign(host_data, host_data + t.numel());
  // one form per layer: a folded "<x>.weight" replaces an earlier weight_g / weight_v pair and vice versa (a second
  // load on the same context must not keep the other form's tensors)
  if (folded_form) {
    ctx->raw.erase(k + "_v");
    ctx->raw.erase(k + "_g");
  } else if (k.size() > 9 && (k.compare(k.size() - 9, 9, ".weight_v") == 0 || k.compare(k.size() - 9, 9, ".weight_g") == 0)) {
    ctx->raw.erase(k.substr(0, k.size() - 2));
  }
  ctx->raw[k] = std::move(t);
  ctx->ready = false;
  return VSP_OK;
}

// f16 / bf16 bit patterns -> float (host)
static float half_bits_to_float(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
  uint32_t bits;
  if (exp == 0) {
    if (man == 0) bits = sign;
    else {  // subnormal
      int e = -1;
      uint32_t m = man;
      do { ++e; m <<= 1; } while (!(m & 0x400u));
      bits = sign | ((uint32_t)(127 - 15 - e) << 23) | ((m & 0x3ffu) << 13);
    }
  } else if (exp == 31) bits = sign | 0x7f800000u | (man << 13);
  else bits = sign | ((exp + 112u) << 23) | (man << 13);
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}

int vsp_set_weight_typed(vsp_ctx* ctx, const char* key, const void* data, const int64_t* shape, int ndim, int dtype,
                         int on_device) {
  if (!ctx || !key || !data || !shape || ndim < 0 || ndim > 8) return ctx ? ctx->fail(VSP_ERR_ARG, "null argument") : VSP_ERR_ARG;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 0) return ctx->fail(VSP_ERR_ARG, "negative dimension");
    n *= (size_t)shape[i];
  }
  size_t esz = 0;
  switch (dtype) {
    case VSP_DTYPE_F32: esz = 4; break;
    case VSP_DTYPE_F16: case VSP_DTYPE_BF16: esz = 2; break;
    case VSP_DTYPE_F64: esz = 8; break;
    default: return ctx->fail(VSP_ERR_ARG, "vsp_set_weight_typed: unknown dtype %d", dtype);
  }
  std::vector<unsigned char> staged;
  const unsigned char* src = static_cast<const unsigned char*>(data);
  if (on_device) {
    staged.resize(n * esz);
    hipError_t e = hipMemcpy(staged.data(), data, n * esz, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "vsp_set_weight_typed(%s): %s", key, hipGetErrorString(e));
    src = staged.data();
  }
  if (dtype == VSP_DTYPE_F32) return vsp_set_weight(ctx, key, reinterpret_cast<const float*>(src), shape, ndim);
  std::vector<float> f(n);
  for (size_t i = 0; i < n; ++i) {
    if (dtype == VSP_DTYPE_F64) { double d; std::memcpy(&d, src + 8 * i, 8); f[i] = (float)d; }
    else {
      uint16_t h; std::memcpy(&h, src + 2 * i, 2);
      if (dtype == VSP_DTYPE_BF16) { const uint32_t b = (uint32_t)h << 16; std::memcpy(&f[i], &b, 4); }
      else f[i] = half_bits_to_float(h);
    }
  }
  return vsp_set_weight(ctx, key, f.data(), shape, ndim);
}

int vsp_missing_weights(const vsp_ctx* ctx) {
  if (!ctx) return VSP_ERR_ARG;
  int n = 0;
  for (const auto& kv : ctx->schema) {
    if (!kv.second.used || kv.second.optional) continue;
    if (ctx->raw.count(kv.first)) continue;
    const std::string& k = kv.first;
    // weight_g / weight_v are satisfied by a pre-folded weight
    if (k.size() > 2 && (k.compare(k.size() - 2, 2, "_v") == 0 || k.compare(k.size() - 2, 2, "_g") == 0) &&
        ctx->raw.count(k.substr(0, k.size() - 2)))
      continue;
    ++n;
  }
  return n;
}

int64_t vsp_weight_arena_bytes(const vsp_ctx* ctx) {
  return ctx ? (int64_t)(ctx->model.total_floats * sizeof(float)) : VSP_ERR_ARG;
}

// The status word (vsp_status): pinned host memory mapped into the device's address space, so that reading it costs no
// stream synchronisation; the kernels touch it only when they have something to report.
static int ensure_flags(vsp_ctx* ctx) {
  if (ctx->flags_host) return VSP_OK;
  void* h = nullptr;
  void* d = nullptr;
  hipError_t e = hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable);
  if (e == hipSuccess) { *static_cast<unsigned*>(h) = 0u; e = hipHostGetDevicePointer(&d, h, 0); }
  if (e != hipSuccess) {
    if (h) (void)hipHostFree(h);
    return ctx->fail(VSP_ERR_HIP, "status word (hipHostMalloc): %s", hipGetErrorString(e));
  }
  ctx->flags_host = static_cast<unsigned*>(h);
  ctx->flags_dev = static_cast<unsigned*>(d);
  return VSP_OK;
}

static int set_arena(vsp_ctx* ctx, void* dev_arena) {
  if (int rc = ensure_flags(ctx)) return rc;
  if (ctx->arena && ctx->arena_owned && ctx->arena != dev_arena) (void)hipFree(ctx->arena);
  if (dev_arena) {
    ctx->arena = (float*)dev_arena;
    ctx->arena_owned = false;
  } else if (!ctx->arena || !ctx->arena_owned) {
    void* p = nullptr;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&p, ctx->model.total_floats * sizeof(float));
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "hipMalloc(weight arena): %s", hipGetErrorString(e));
    ctx->arena = (float*)p;
    ctx->arena_owned = true;
  }
  return VSP_OK;
}

static uint32_t config_hash(const vsp_ctx* ctx) {
  // FNV-1a over the config bytes and the switches that change the packing
  uint32_t h = 2166136261u;
  auto mix = [&](const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 16777619u; }
  };
  mix(&ctx->cfg, sizeof ctx->cfg);
  const int sw[3] = {ctx->frame_f16s ? 1 : 0, ctx->model.has_cl ? 1 : 0, ctx->gen_mode != 0 ? 1 : 0};
  mix(sw, sizeof sw);
  mix(&ctx->act_scale, sizeof ctx->act_scale);   // (the packed generator biases carry it)
  if (ctx->resblock == 2) mix(&ctx->resblock, sizeof ctx->resblock);   // (ResBlock1 arenas hash as they always did)
  return h;
}

int vsp_finalize_weights(vsp_ctx* ctx, void* dev_arena) {
  if (!ctx) return VSP_ERR_ARG;
  if (ctx->model.total_floats == 0) return ctx->fail(VSP_ERR_STATE, "context was not planned (vsp_create failed)");
  const int miss = vsp_missing_weights(ctx);
  if (miss) return ctx->fail(VSP_ERR_STATE, "%d infer-path tensors missing", miss);
  std::vector<float> host;
  int rc = fill_model(ctx, host);
  if (rc) return rc;
  {
    const uint64_t tf = ctx->model.total_floats;
    const uint32_t hdr[6] = {ARENA_MAGIC, (uint32_t)VSP_ABI_VERSION, (uint32_t)(tf & 0xffffffffu), (uint32_t)(tf >> 32),
                             ctx->model.has_vc ? ARENA_FLAG_VC : 0u, config_hash(ctx)};
    std::memcpy(host.data(), hdr, sizeof hdr);
  }
  tail_table_drop(ctx);                      // (the table belongs to the weights it was built from)
  rc = set_arena(ctx, dev_arena);
  if (rc) return rc;
  hipError_t e = hipMemcpy(ctx->arena, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "hipMemcpy(weight arena): %s", hipGetErrorString(e));
  ctx->adopted_pending = false;
  ctx->ready = true;
  tail_table_build(ctx, nullptr);
  return VSP_OK;
}

int vsp_adopt_packed_weights(vsp_ctx* ctx, void* dev_arena) {
  if (!ctx || !dev_arena) return ctx ? ctx->fail(VSP_ERR_ARG, "null arena") : VSP_ERR_ARG;
  if (ctx->model.total_floats == 0) return ctx->fail(VSP_ERR_STATE, "context was not planned");
  tail_table_drop(ctx);
  const int rc = set_arena(ctx, dev_arena);
  if (rc) return rc;
  // the bytes may not have arrived yet (the broadcast follows): nothing is known about them until
  // vsp_commit_adopted_weights has read the header -- fail closed until then
  ctx->model.has_vc = false;
  ctx->ready = false;
  ctx->adopted_pending = true;
  return VSP_OK;
}

int vsp_commit_adopted_weights(vsp_ctx* ctx, void* stream) {
  if (!ctx) return VSP_ERR_ARG;
  if (!ctx->adopted_pending || !ctx->arena) return ctx->fail(VSP_ERR_STATE, "no adopted arena to commit");
  uint32_t hdr[6] = {0, 0, 0, 0, 0, 0};
  hipError_t e = hipMemcpyAsync(hdr, ctx->arena, sizeof hdr, hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "arena header read: %s", hipGetErrorString(e));
  const uint64_t tf = (uint64_t)hdr[2] | ((uint64_t)hdr[3] << 32);
  if (hdr[0] != ARENA_MAGIC) return ctx->fail(VSP_ERR_STATE, "adopted arena has no header (bytes not broadcast yet, or not a packed arena)");
  if (hdr[1] != (uint32_t)VSP_ABI_VERSION) return ctx->fail(VSP_ERR_STATE, "adopted arena was packed by ABI %u, this library is ABI %d", hdr[1], VSP_ABI_VERSION);
  if (tf != ctx->model.total_floats || hdr[5] != config_hash(ctx))
    return ctx->fail(VSP_ERR_STATE, "adopted arena was packed for a different configuration");
  ctx->model.has_vc = (hdr[4] & ARENA_FLAG_VC) != 0;
  ctx->adopted_pending = false;
  ctx->ready = true;
  tail_table_build(ctx, (hipStream_t)stream);
  return VSP_OK;
}

int vsp_has_voice_conversion(const vsp_ctx* ctx) { return ctx && ctx->ready && ctx->model.has_vc ? 1 : 0; }

int vsp_weight_arena(const vsp_ctx* ctx, void** dev_arena, int64_t* bytes) {
  if (!ctx || !dev_arena || !bytes) return VSP_ERR_ARG;
  *dev_arena = ctx->arena;
  *bytes = (int64_t)(ctx->model.total_floats * sizeof(float));
  return VSP_OK;
}

int vsp_randn(void* stream, uint64_t seed, int64_t n, float* out) { return vsp_randn_at(stream, seed, 0, n, out); }

int vsp_randn_at(void* stream, uint64_t seed, int64_t first, int64_t n, float* out) {
  if (n < 0 || first < 0 || (n > 0 && !out)) return VSP_ERR_ARG;
  return launch_randn(seed, (long)first, (long)n, out, (hipStream_t)stream) == hipSuccess ? VSP_OK : VSP_ERR_HIP;
}

int vsp_set_noise_offset(vsp_ctx* ctx, int64_t first_element) {
  if (!ctx || first_element < 0) return ctx ? ctx->fail(VSP_ERR_ARG, "vsp_set_noise_offset: negative offset") : VSP_ERR_ARG;
  ctx->noise_first = first_element;
  return VSP_OK;
}

int vsp_set_isolated(vsp_ctx* ctx, int on) {
  if (!ctx) return VSP_ERR_ARG;
  ctx->isolated = on != 0;
  return VSP_OK;
}

int vsp_get_isolated(const vsp_ctx* ctx) { return ctx ? (ctx->isolated ? 1 : 0) : VSP_ERR_ARG; }

int vsp_set_noise_seeds(vsp_ctx* ctx, const uint64_t* seeds_host, int B) {
  if (!ctx) return VSP_ERR_ARG;
  if (B < 0 || (B > 0 && !seeds_host)) return ctx->fail(VSP_ERR_ARG, "vsp_set_noise_seeds: B < 0 or null seeds");
  ctx->noise_seeds.assign(seeds_host, seeds_host + B);     // (B = 0 forgets them)
  return VSP_OK;
}

int vsp_set_row_controls(vsp_ctx* ctx, const vsp_row_control* rows_host, int B) {
  if (!ctx) return VSP_ERR_ARG;
  if (B < 0 || (B > 0 && !rows_host)) return ctx->fail(VSP_ERR_ARG, "vsp_set_row_controls: B < 0 or null rows");
  const uint32_t known = VSP_GIVEN_DURATION | VSP_GIVEN_PITCH | VSP_GIVEN_ENERGY;
  for (int b = 0; b < B; ++b) {
    const vsp_row_control& rc = rows_host[b];
    if (rc.given & ~known) return ctx->fail(VSP_ERR_ARG, "vsp_set_row_controls: row %d has unknown given bits 0x%x", b, rc.given);
    if (!std::isfinite(rc.duration_scale) || !std::isfinite(rc.pitch_scale) || !std::isfinite(rc.energy_scale) ||
        !std::isfinite(rc.noise_scale))
      return ctx->fail(VSP_ERR_ARG, "vsp_set_row_controls: row %d has a scale that is not finite", b);
  }
  ctx->row_controls.assign(rows_host, rows_host + B);     // (B = 0 forgets the table; a refused table changes nothing)
  return VSP_OK;
}

int vsp_rq_spline(void* stream, int64_t n, int nb, const float* x, const float* uw, const float* uh, const float* ud,
                  int inverse, float tail_bound, float* y, float* logabsdet) {
  if (n < 0 || !x || !uw || !uh || !ud || !y || !logabsdet) return VSP_ERR_ARG;
  hipError_t e = launch_rq_spline(n, nb, x, uw, uh, ud, inverse, tail_bound, y, logabsdet, (hipStream_t)stream);
  return e == hipSuccess ? VSP_OK : (e == hipErrorInvalidValue ? VSP_ERR_UNSUPPORTED : VSP_ERR_HIP);
}

// -------------------------------------------------------------------------------------------- mel spectrogram
namespace {
// librosa.filters.mel with its defaults (htk = False, norm = 'slaney'), in double precision
bool mel_basis(int sr, int n_fft, int n_mels, double fmin, double fmax, std::vector<float>& w) {
  if (sr <= 0 || n_fft < 2 || (n_fft & 1) || n_mels < 1) return false;
  if (fmax <= 0.0) fmax = sr / 2.0;
  if (fmin < 0.0 || fmax <= fmin) return false;
  const int nf = n_fft / 2 + 1;
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  auto hz_to_mel = [&](double f) { return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp; };
  auto mel_to_hz = [&](double m) { return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m; };
  std::vector<double> mel_f(n_mels + 2);
  const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
  for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1));
  w.assign((size_t)n_mels * nf, 0.f);
  for (int m = 0; m < n_mels; ++m) {
    const double enorm = 2.0 / (mel_f[m + 2] - mel_f[m]);
    for (int k = 0; k < nf; ++k) {
      const double f = (sr / 2.0) * k / (nf - 1);
      const double lower = (f - mel_f[m]) / (mel_f[m + 1] - mel_f[m]), upper = (mel_f[m + 2] - f) / (mel_f[m + 2] - mel_f[m + 1]);
      const double v = std::max(0.0, std::min(lower, upper));
      w[(size_t)m * nf + k] = (float)(v * enorm);
    }
  }
  return true;
}
}  // namespace

int vsp_mel_filterbank(int sampling_rate, int n_fft, int n_mels, float fmin, float fmax, float* basis_host) {
  if (!basis_host) return VSP_ERR_ARG;
  std::vector<float> w;
  if (!mel_basis(sampling_rate, n_fft, n_mels, fmin, fmax, w)) return VSP_ERR_ARG;
  std::memcpy(basis_host, w.data(), w.size() * sizeof(float));
  return VSP_OK;
}

int vsp_spec_to_mel(void* stream, int B, int T, int n_fft, int n_mels, int sampling_rate, float fmin, float fmax,
                    const float* spec, float* mel) {
  if (!spec || !mel || B < 0 || T < 0) return VSP_ERR_ARG;
  std::vector<float> w;
  if (!mel_basis(sampling_rate, n_fft, n_mels, fmin, fmax, w)) return VSP_ERR_ARG;
  if (B == 0 || T == 0) return VSP_OK;
  const int nf = n_fft / 2 + 1;
  std::vector<int> lo(n_mels), hi(n_mels);
  for (int m = 0; m < n_mels; ++m) {
    int a = nf, b = 0;
    for (int k = 0; k < nf; ++k)
      if (w[(size_t)m * nf + k] != 0.f) { a = std::min(a, k); b = k + 1; }
    lo[m] = a < b ? a : 0; hi[m] = a < b ? b : 0;
  }
  hipStream_t s = (hipStream_t)stream;
  void *dw = nullptr, *dr = nullptr;
  hipError_t e = hipMalloc(&dw, w.size() * 4);
  if (e == hipSuccess) e = hipMalloc(&dr, (size_t)2 * n_mels * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dr, lo.data(), (size_t)n_mels * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(static_cast<int*>(dr) + n_mels, hi.data(), (size_t)n_mels * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = launch_spec_to_mel(spec, static_cast<const float*>(dw), static_cast<const int*>(dr), static_cast<const int*>(dr) + n_mels,
                           mel, B, nf, n_mels, T, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);      // (the host vectors and the scratch die with this frame)
  if (dw) (void)hipFree(dw);
  if (dr) (void)hipFree(dr);
  return e == hipSuccess ? VSP_OK : VSP_ERR_HIP;
}

// -------------------------------------------------------------------------------------------- profiling
int vsp_profile_enable(vsp_ctx* ctx, int on) {
  if (!ctx) return VSP_ERR_ARG;
  if (on && !ctx->prof_on) {          // a fresh measurement: forget whatever an earlier one left unread
    ctx->ev_used = 0;
    for (int c = 0; c < VSP_PROF_CLASSES; ++c) {
      ctx->prof_launches[c] = 0;
      ctx->prof_flops[c] = ctx->prof_bytes[c] = ctx->prof_bytes_ext[c] = ctx->prof_bytes_moved[c] = 0.0;
    }
  }
  ctx->prof_on = on != 0;
  return VSP_OK;
}

int vsp_profile_read_class(vsp_ctx* ctx, int cls, int64_t* launches, double* total_ms, double* total_flops,
                           double* total_bytes, double* total_bytes_ext, double* total_bytes_moved, int reset) {
  if (!ctx || cls < 0 || cls >= VSP_PROF_CLASSES || !launches || !total_ms || !total_flops || !total_bytes)
    return ctx ? ctx->fail(VSP_ERR_ARG, "vsp_profile_read_class: bad argument") : VSP_ERR_ARG;
  double ms = 0.0;
  for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
    if (ctx->ev_cls[i / 2] != cls) continue;
    hipError_t e = hipEventSynchronize(ctx->ev_pool[i + 1]);
    float t = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ctx->ev_pool[i], ctx->ev_pool[i + 1]);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "profile events: %s", hipGetErrorString(e));
    ms += t;
  }
  *launches = ctx->prof_launches[cls];
  *total_ms = ms;
  *total_flops = ctx->prof_flops[cls];
  *total_bytes = ctx->prof_bytes[cls];
  if (total_bytes_ext) *total_bytes_ext = ctx->prof_bytes_ext[cls];
  if (total_bytes_moved) *total_bytes_moved = ctx->prof_bytes_moved[cls];
  if (reset) {
    // the event pool is shared: drop every class's events only when the LAST class has been read; a reset of one
    // class zeroes its counters and marks its pairs as consumed
    ctx->prof_launches[cls] = 0;
    ctx->prof_flops[cls] = ctx->prof_bytes[cls] = ctx->prof_bytes_ext[cls] = ctx->prof_bytes_moved[cls] = 0.0;
    bool any = false;
    for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
      if (ctx->ev_cls[i / 2] == cls) ctx->ev_cls[i / 2] = -1;
      else if (ctx->ev_cls[i / 2] >= 0) any = true;
    }
    if (!any) ctx->ev_used = 0;
  }
  return VSP_OK;
}

int vsp_profile_read_families(vsp_ctx* ctx, int cls, int max_families, int* family, int64_t* launches, double* total_ms,
                              double* total_flops, double* total_bytes, double* total_bytes_moved) {
  if (!ctx || cls < 0 || cls >= VSP_PROF_CLASSES || max_families < 0 || !family || !launches || !total_ms || !total_flops ||
      !total_bytes)
    return ctx ? ctx->fail(VSP_ERR_ARG, "vsp_profile_read_families: bad argument") : VSP_ERR_ARG;
  int n = 0;
  for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
    if (ctx->ev_cls[i / 2] != cls) continue;
    hipError_t e = hipEventSynchronize(ctx->ev_pool[i + 1]);
    float t = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ctx->ev_pool[i], ctx->ev_pool[i + 1]);
    if (e != hipSuccess) return ctx->fail(VSP_ERR_HIP, "profile events: %s", hipGetErrorString(e));
    const int f = ctx->ev_fam[i / 2];
    int k = 0;
    while (k < n && family[k] != f) ++k;
    if (k == n) {
      if (n == max_families) continue;
      family[n] = f; launches[n] = 0; total_ms[n] = total_flops[n] = total_bytes[n] = 0.0;
      if (total_bytes_moved) total_bytes_moved[n] = 0.0;
      ++n;
    }
    launches[k] += 1;
    total_ms[k] += t;
    total_flops[k] += ctx->ev_flops[i / 2];
    total_bytes[k] += ctx->ev_bytes[i / 2];
    if (total_bytes_moved) total_bytes_moved[k] += ctx->ev_moved[i / 2];
  }
  return n;
}

int vsp_profile_read(vsp_ctx* ctx, int64_t* launches, double* total_ms, double* total_flops, double* total_bytes,
                     int reset) {
  return vsp_profile_read_class(ctx, VSP_PROF_GENERATOR, launches, total_ms, total_flops, total_bytes, nullptr, nullptr, reset);
}

}  // extern "C"
