// Stand-alone host program for a sanitizer build (tools/sanitize_isolated_args.sh): the argument validation of the
// isolated-mode entry points of include/vispeech_hip.h on paths that need no GPU -- null contexts, a context whose weights
// are not finalised, seed arrays that grow, shrink and are forgotten.  Exit status 0 = every check held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vispeech_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static vsp_config default_config() {
  vsp_config c;
  std::memset(&c, 0, sizeof c);
  c.n_vocab = 519; c.inter_channels = 192; c.hidden_channels = 192; c.filter_channels = 768; c.n_heads = 2; c.n_layers = 4;
  c.kernel_size = 3;
  c.n_resblock_kernels = 3; c.n_resblock_dilations = 3;
  const int ks[3] = {3, 7, 11}, ds[3] = {1, 3, 5};
  for (int i = 0; i < 3; ++i) {
    c.resblock_kernel_sizes[i] = ks[i];
    for (int j = 0; j < 3; ++j) c.resblock_dilation_sizes[i][j] = ds[j];
  }
  c.n_upsamples = 5;
  const int ur[5] = {8, 8, 2, 2, 2}, uk[5] = {16, 16, 4, 4, 4};
  for (int i = 0; i < 5; ++i) { c.upsample_rates[i] = ur[i]; c.upsample_kernel_sizes[i] = uk[i]; }
  c.upsample_initial_channel = 512; c.n_speakers = 67; c.gin_channels = 256; c.window_size = 4; c.pitch_layers = 6;
  c.dur_filter = 256; c.energy_filter = 256; c.flow_kernel = 5; c.flow_layers = 4; c.n_flows = 4; c.spec_channels = 0;
  c.posterior_layers = 16;
  return c;
}

int main() {
  // null contexts
  EXPECT(vsp_set_isolated(nullptr, 1) == VSP_ERR_ARG);
  EXPECT(vsp_get_isolated(nullptr) == VSP_ERR_ARG);
  uint64_t one = 1;
  EXPECT(vsp_set_noise_seeds(nullptr, &one, 1) == VSP_ERR_ARG);
  float dummy[4] = {0, 0, 0, 0};
  int64_t len = 1;
  EXPECT(vsp_generator_ragged(nullptr, nullptr, 1, 1, dummy, dummy, &len, dummy, dummy, 16) == VSP_ERR_ARG);

  vsp_config cfg = default_config();
  vsp_ctx* ctx = nullptr;
  const int rc = vsp_create(&cfg, 0, &ctx);
  std::printf("vsp_create: %d (%s)\n", rc, ctx ? vsp_last_error(ctx) : "");
  EXPECT(ctx != nullptr);
  if (ctx) {
    EXPECT(vsp_get_isolated(ctx) == 0);                      // off by default
    EXPECT(vsp_set_isolated(ctx, 7) == VSP_OK && vsp_get_isolated(ctx) == 1);
    EXPECT(vsp_set_isolated(ctx, 0) == VSP_OK && vsp_get_isolated(ctx) == 0);
    // seeds: copied (the caller's array may die), replaced by a longer and a shorter set, forgotten
    {
      std::vector<uint64_t> s(3, 0xffffffffffffffffull);
      EXPECT(vsp_set_noise_seeds(ctx, s.data(), 3) == VSP_OK);
    }
    std::vector<uint64_t> big(4096);
    for (size_t i = 0; i < big.size(); ++i) big[i] = i * 0x9E3779B97F4A7C15ull;
    EXPECT(vsp_set_noise_seeds(ctx, big.data(), (int)big.size()) == VSP_OK);
    EXPECT(vsp_set_noise_seeds(ctx, big.data() + 4095, 1) == VSP_OK);
    EXPECT(vsp_set_noise_seeds(ctx, nullptr, 0) == VSP_OK);
    EXPECT(vsp_set_noise_seeds(ctx, nullptr, 2) == VSP_ERR_ARG);
    EXPECT(vsp_set_noise_seeds(ctx, big.data(), -1) == VSP_ERR_ARG);
    EXPECT(std::strstr(vsp_last_error(ctx), "vsp_set_noise_seeds") != nullptr);
    // the ragged generator before the weights are finalised: refused before any pointer is touched
    EXPECT(vsp_generator_ragged(ctx, nullptr, 2, 8, dummy, dummy, &len, dummy, dummy, 1 << 20) == VSP_ERR_STATE);
    EXPECT(std::strstr(vsp_last_error(ctx), "not finalised") != nullptr);
    EXPECT(vsp_destroy(ctx) == VSP_OK);
  }
  std::printf(failures ? "%d check(s) FAILED\n" : "isolated-mode argument checks: ok\n", failures);
  return failures ? 1 : 0;
}
