// What the two framing kernels of the spectrogram front ends share (spectrogram_ragged.hip, convert_window.hip): the LDS
// budget of a block and the bank skew of the staged span.
#pragma once

namespace vsp {

// LDS of one framing block.  The CU has 160 KiB (MI355X_MICROARCH.md); 64 KiB per block keeps at least two blocks
// resident, so one block's staging loads run under the other's stores, and needs no opt-in above the default limit.
constexpr int FR_LDS_BYTES = 64 * 1024;
constexpr int FR_THREADS = 256;
constexpr int FR_MAX_TILE = 32;

// One float of padding per 256 samples: the lanes of a wave read tile columns that are `hop` samples apart, and with hop
// a multiple of 32 floats they would all meet in one bank.  A 4-byte LDS read is served in groups of 32 lanes over 32
// banks (MI355X_MICROARCH.md, LDS); with the skew the 16 columns x 2 samples of a group of the default configuration
// (hop 512: column tl starts at bank 2 tl) take 32 different banks.  Staging stores walk consecutive slots.
__host__ __device__ inline int fr_slot(int i) { return i + (i >> 8); }

}  // namespace vsp
