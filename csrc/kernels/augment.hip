// DrQ random-shift augmentation fused into the frame-stack gather (--augment shift).
//
// Replicate-pad the H x W frame by P pixels and take a random H x W crop, i.e.
//   out[b, y, x, c] = frame_c[clamp(y + dy, 0, H - 1)][clamp(x + dx, 0, W - 1)],   dy, dx in [-P, P],
// one (dy, dx) per minibatch position b and per stack (which = 0: s, 1: s'), shared by the four
// frames of the stack. The shift is a pure function of (seed, step counter, b, which):
//   r = philox(seed ^ kAugKey, ctr, b, which);  dy = (r.x * (2P + 1) >> 32) - P;  dx likewise from r.y
// with ctr read from a device int64 (the learner's global_step, which the optimizer launch advances:
// every step of a multi-step graph draws fresh shifts, and no block writes RNG state).
//
// The kernel reads the [B, 4] slot tables any sampler wrote and writes both NHWC uint8 stacks the
// stack loaders of the trunk / conv1 weight-gradient kernels read; pad = 0 is the plain gather
// (gather_frames_kernel of replay.hip, bit for bit).
#include "common.h"
#include "../include/dqn_kernels.h"

namespace dqn {

constexpr uint64_t kAugKey = 0x6175676dull;   // "augm"

// A block is uniform in (b, which): blockIdx.y = 2 b + which, so the shift and the four slot ids
// live in scalar registers. One thread = 4 consecutive output pixels (one 16-byte NHWC store).
__global__ void __launch_bounds__(256)
gather_shift_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ st_slots,
                    const int32_t* __restrict__ nx_slots, uint64_t seed, const int64_t* __restrict__ ctr_p, int pad,
                    uint8_t* __restrict__ out_s, uint8_t* __restrict__ out_ns, int32_t* __restrict__ shifts, int H,
                    int W, int F) {
  const int b = blockIdx.y >> 1, which = blockIdx.y & 1;
  const uint64_t ctr = (uint64_t)ctr_p[0];
  const u32x4 r = philox(seed ^ kAugKey, ctr, (uint32_t)b, (uint32_t)which);
  const uint32_t span = 2u * (uint32_t)pad + 1u;
  const int dy = (int)(((uint64_t)r.x * span) >> 32) - pad;
  const int dx = (int)(((uint64_t)r.y * span) >> 32) - pad;
  if (blockIdx.x == 0 && threadIdx.x == 0 && shifts != nullptr) {
    shifts[blockIdx.y * 2 + 0] = dy;
    shifts[blockIdx.y * 2 + 1] = dx;
  }
  const int WG = W >> 2;                       // 4-pixel groups per row (W % 4 == 0)
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= H * WG) return;
  const int y = g / WG, x0 = 4 * (g - y * WG);
  const int4 sl = reinterpret_cast<const int4*>(which ? nx_slots : st_slots)[b];
  const int slot[4] = {sl.x, sl.y, sl.z, sl.w};
  const int sy = min(max(y + dy, 0), H - 1);   // row clamping is just the row index
  const int sx = x0 + dx;
  uint32_t px[4];                              // frame c's 4 source pixels, little-endian
  if (sx >= 0 && sx + 3 < W) {
    // interior group: the 4 source bytes sit in two aligned words of the row (rows are 4-aligned:
    // W % 4 == 0). The second word is not needed when sx is aligned and is kept inside the row.
    const int w0 = sx >> 2, w1 = min(w0 + 1, WG - 1);
    const uint32_t sh = (uint32_t)sx & 3u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      DQN_ASSERT(slot[c] >= 0 && slot[c] < F);
      const int f = min(max(slot[c], 0), F - 1);
      const uint32_t* row = reinterpret_cast<const uint32_t*>(frames + ((int64_t)f * H + sy) * W);
      px[c] = __builtin_amdgcn_alignbyte(row[w1], row[w0], sh);
    }
  } else {
    // a group over the left or right edge: byte-wise, every column clamped
    int cx[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) cx[p] = min(max(sx + p, 0), W - 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      DQN_ASSERT(slot[c] >= 0 && slot[c] < F);
      const int f = min(max(slot[c], 0), F - 1);
      const uint8_t* row = frames + ((int64_t)f * H + sy) * W;
      px[c] = (uint32_t)row[cx[0]] | ((uint32_t)row[cx[1]] << 8) | ((uint32_t)row[cx[2]] << 16) |
              ((uint32_t)row[cx[3]] << 24);
    }
  }
  // transpose 4 frames x 4 pixels -> per pixel its 4 channels
  uint32_t w[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    w[p] = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) w[p] |= ((px[c] >> (8 * p)) & 0xffu) << (8 * c);
  }
  uint8_t* dst = (which ? out_ns : out_s) + (((int64_t)b * H + y) * W + x0) * 4;
  *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace dqn

using namespace dqn;

void launch_replay_gather_shift(const uint8_t* frames, const int32_t* st_slots, const int32_t* nx_slots,
                                uint64_t seed, const int64_t* ctr, int pad, uint8_t* out_s, uint8_t* out_ns,
                                int32_t* shifts, int B, int H, int W, int F, hipStream_t st) {
  const int groups = H * (W / 4);
  dim3 grid((groups + 255) / 256, 2 * B), block(256);
  hipLaunchKernelGGL(gather_shift_kernel, grid, block, 0, st, frames, st_slots, nx_slots, seed, ctr, pad, out_s,
                     out_ns, shifts, H, W, F);
}
