// Global gradient-norm clipping (TensorFlow's clip_by_global_norm) over the flat fp32 gradient:
//   norm  = grad_scale * ||g||_2          (grad_scale: the data-parallel average the optimizer applies)
//   scale = C / max(norm, C)              (exactly 1.0f when norm <= C; 0 when norm is not finite)
//   g    <- g * scale
// Two bandwidth-bound launches between the backward and the optimizer; the scale stays on the device
// (stats[0] = norm, stats[1] = scale), so both are graph-capturable.
//
// The flat gradient is already free of the fp16 build's static loss scale (every weight-gradient
// kernel multiplies by kInvLossScale when it stores, dqn_act.h), so no build rescales here.
//
// Summation shape (a function of n, the pointer's 16-byte phase and the block count only, so the
// same buffer gives the same bits on every replay and on every data-parallel rank):
//   thread: its grid-stride float4s in order, four squares each, + at most one head / tail scalar
//   wave:   DPP row sums + 4 readlanes (wave_sum_dpp);  block: 4 wave totals as (w0 + w1) + (w2 + w3)
//   grid:   one fp32 partial per block in slot blockIdx.x; the last-arriving block sums the slots:
//           thread t takes slots t, t + 256, ... in order, then the same wave / block tree.
#include "common.h"
#include "../include/dqn_kernels.h"

namespace dqn {

constexpr int kClipThreads = 256;
constexpr int kClipMaxBlocks = 512;      // two per CU
constexpr int kClipBlockElems = 4096;    // one block per 4 float4s of every thread, up to the cap

// the slice [p, p + n) as head scalars (up to the first 16-byte boundary), float4 body, tail scalars
struct ClipSplit { int head; int64_t n4; int tail; };
DQN_DEV ClipSplit clip_split(const float* p, int64_t n) {
  int head = (int)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
  if ((int64_t)head > n) head = (int)n;
  const int64_t body = n - head;
  return {head, body >> 2, (int)(body & 3)};
}

// sum over the block's 256 threads, result in every thread (sh: 4 floats, free to reuse after)
DQN_DEV float block_sum(float v, float* sh) {
  const float w = wave_sum_dpp(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  const float s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return s;
}

__global__ void __launch_bounds__(kClipThreads)
grad_sqnorm_kernel(const float* __restrict__ g, int64_t n, float max_norm, float grad_scale,
                   float* __restrict__ stats, float* __restrict__ partials, int32_t* __restrict__ counter) {
  __shared__ float sh[8];                // [0, 4): wave totals; [4]: "this block arrived last"
  const ClipSplit sp = clip_split(g, n);
  const int64_t gid = (int64_t)blockIdx.x * kClipThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kClipThreads;
  const float4* g4 = reinterpret_cast<const float4*>(g + sp.head);
  float acc = 0.f;
  for (int64_t i = gid; i < sp.n4; i += stride) {
    const float4 v = g4[i];
    acc += v.x * v.x;
    acc += v.y * v.y;
    acc += v.z * v.z;
    acc += v.w * v.w;
  }
  // head scalars on threads 0..2, tail scalars on threads 4..6 of block 0 (one each at most)
  if (gid < sp.head) {
    const float x = g[gid];
    acc += x * x;
  } else if (gid >= 4 && gid < 4 + sp.tail) {
    const float x = g[sp.head + 4 * sp.n4 + (gid - 4)];
    acc += x * x;
  }
  const float bsum = block_sum(acc, sh);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = bsum;
    // publish the partial, then arrive: agent-scope release before the relaxed ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int t = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = t == (int)gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    sh[4] = last ? 1.f : 0.f;
  }
  __syncthreads();
  if (sh[4] == 0.f) return;
  // the last block: every partial is visible (the acquire above, then the barrier)
  float s = 0.f;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += kClipThreads) s += partials[i];
  const float total = block_sum(s, sh);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(total) * grad_scale;
    const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
    stats[0] = norm;
    stats[1] = finite ? max_norm / fmaxf(norm, max_norm) : 0.f;
    // (the counter resets itself: a graph replay needs no memset node)
    __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(kClipThreads)
grad_scale_kernel(float* __restrict__ g, int64_t n, const float* __restrict__ stats) {
  const float scale = stats[1];
  if (scale == 1.0f) return;             // norm <= max_norm: the buffer is not touched
  const bool zero = scale == 0.f;        // non-finite norm: no loss gradient (NaN * 0 would stay NaN)
  const ClipSplit sp = clip_split(g, n);
  const int64_t gid = (int64_t)blockIdx.x * kClipThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kClipThreads;
  float4* g4 = reinterpret_cast<float4*>(g + sp.head);
  for (int64_t i = gid; i < sp.n4; i += stride) {
    float4 v = g4[i];
    v = zero ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
    g4[i] = v;
  }
  if (gid < sp.head) {
    g[gid] = zero ? 0.f : g[gid] * scale;
  } else if (gid >= 4 && gid < 4 + sp.tail) {
    float* p = g + sp.head + 4 * sp.n4 + (gid - 4);
    *p = zero ? 0.f : *p * scale;
  }
}

}  // namespace dqn

using namespace dqn;

int grad_clip_blocks(int64_t n) {
  const int64_t b = (n + kClipBlockElems - 1) / kClipBlockElems;
  return b < 1 ? 1 : (b > kClipMaxBlocks ? kClipMaxBlocks : (int)b);
}

void launch_grad_clip(float* grad, int64_t n, float max_norm, float grad_scale, float* stats, float* partials,
                      int32_t* counter, hipStream_t st) {
  const dim3 grid(grad_clip_blocks(n)), block(kClipThreads);
  hipLaunchKernelGGL(grad_sqnorm_kernel, grid, block, 0, st, grad, n, max_norm, grad_scale, stats, partials, counter);
  hipLaunchKernelGGL(grad_scale_kernel, grid, block, 0, st, grad, n, stats);
}
