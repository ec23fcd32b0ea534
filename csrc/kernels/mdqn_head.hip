// Munchausen-DQN head of the HIP executor (Vieillard, Pietquin, Geist 2020): a sibling of the C51
// and QR-DQN heads (rainbow.hip, qr_head.hip) on the same precomputed fp32 output rows, with ONE
// output per action. Torch oracle: dist_dqn_amd/models/losses.py (munchausen_loss).
//
//   mdqn_train_kernel  training head, one wave64 per sample: lanes [0, 32) hold the actions of
//                      target(s') and online(s), lanes [32, 64) those of target(s), so each
//                      reduction over actions serves two instances at once (DPP row ops + four
//                      read-lanes, common.h half_*_dpp); dueling combine, both log-sum-exps, the
//                      TD error (= the priority), the MSE / Huber loss partial and dL/dQ as the
//                      act_t rows the dH igemm and the output layer's grouped weight-gradient
//                      members consume; one more block per fused-acting env.
//   mdqn_infer_kernel  acting / q_values: dueling combine -> q_out / fused actor step on plain Q.
//
// Target of one sample (q' = target net on s', q0 = target net on s, Q = online net on s; every
// row after the dueling combine Q = A + V - mean A), in max-subtracted form so that tau = 0.03
// with Q values of a few hundred neither overflows nor loses the small terms:
//   soft = max_k q'_k + tau log sum_k exp((q'_k - max_k q'_k) / tau)
//   lp   = q0_a - max_k q0_k - tau log sum_k exp((q0_k - max_k q0_k) / tau)        (= tau log pi(a|s) <= 0)
//   y    = r + alpha clip(lp, l0, 0) + gamma (1 - done) soft,   d = Q_a - y,   prio = |d|
//   per  = d^2 (MSE) or Huber_delta(d);  dper / dQ_a = 2 d or clamp(d, -delta, delta)
// expf / logf are the accurate library functions, not the fast intrinsics.
// HeadArgs: m_alpha, m_tau, m_clip = alpha, tau, l0; huber / delta as in the scalar heads;
// lgi = rows of online(s), target(s'), target(s).
#include "common.h"
#include "actor_dev.h"
#include "../include/dqn_nets_k.h"

namespace dqn {

// Row layout of the precomputed output rows (the C51 head's with one output per action): KD
// floats = [Q / advantages (A <= 32) | pad to 32 | dueling value at VO = 32 | pad to 64]
constexpr int kMdVO = 32;
DQN_DEV_HOST_INLINE int mdqn_kd(const HeadArgs& a) { return a.dueling ? 64 : 32; }

// LDS (floats) of the inference kernel: Q [B][A], then per row its value minus advantage mean
DQN_DEV_HOST_INLINE size_t mdqn_infer_q_bytes(const HeadArgs& a) {
  return ((size_t)a.B * (a.A + 1) * sizeof(float) + 15) / 16 * 16;
}

// Acting / q_values: one block. Dueling: sixteen lanes per row sum its (at most 32) advantages
// on DPP row ops; then one thread per Q value.
__global__ void __launch_bounds__(1024) mdqn_infer_kernel(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int B = a.B, A = a.A, KD = mdqn_kd(a);
  const int tid = threadIdx.x, nth = blockDim.x, l16 = tid & 15;
  float* q = sm;
  float* m = q + B * A;
  const float* src = a.lgi[0];
  if (a.dueling) {
    for (int row = tid >> 4; row < B; row += nth >> 4) {          // uniform per 16-lane group
      const float* r = src + (int64_t)row * KD;
      float s = (l16 < A ? r[l16] : 0.f) + (l16 + 16 < A ? r[l16 + 16] : 0.f);
      s = row16_sum(s);
      if (l16 == 0) m[row] = r[kMdVO] - s / (float)A;
    }
    __syncthreads();
  }
  for (int t = tid; t < B * A; t += nth) {
    const int b = t / A, i = t - b * A;
    q[t] = src[(int64_t)b * KD + i] + (a.dueling ? m[b] : 0.f);
  }
  __syncthreads();
  if (a.q_out != nullptr)
    for (int t = tid; t < B * A; t += nth) a.q_out[t] = q[t];
  // (the PER tree insert's scratch lies behind Q, which the actor step is still reading)
  if (a.has_actor) actor_step_block(a.actor, q, reinterpret_cast<char*>(sm) + mdqn_infer_q_bytes(a));
}

// ---------------------------------------------------------------- Munchausen training head
// The siblings' launch shape (rainbow.hip c51_train_kernel, qr_head.hip qr_train_kernel): learner
// blocks of eight waves, ONE WAVE PER SAMPLE in a block-stride loop, plus one block per
// fused-acting env; per-block loss partials to loss_parts[block] (summed by the fc dgrad launch),
// priorities to prio[b], dL/dQ as act_t (loss-scaled) rows of dout16 [B][KD]: columns [0, A)
// (dueling: times (i == a) - 1/A) and the plain value at VO; pad columns are never written (zero
// from allocation).
//   * all of the sample's loads (three rows, their dueling values, the transition's scalars)
//     issued up front; lanes past A read column 0 (in bounds) and enter the reductions as 0 / -inf;
//   * every per-sample reduction is over a half-wave and its result wave-uniform: no LDS, no
//     atomics, no divergence but the uniform dueling / Huber switches (the block's loss partial
//     is combined through LDS once, after the loop, as in the siblings).
constexpr int kMdWaves = 8, kMdThreads = 64 * kMdWaves, kMdMaxParts = 64;

// Fused acting, one block per env e: env e's row -> wave 0 -> Q row in LDS, while every thread
// writes the env's new frames; then the decision / replay append (actor_dev.h).
DQN_DEV void mdqn_act_env_block(const HeadArgs& a, int e, SumtreeLds& st) {
  __shared__ float qs[32];
  __shared__ int flag;
  const ActorArgs& x = a.actor;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = a.A;
  const ActorPre pre = actor_prefetch(x);
  int32_t st_e[4] = {0, 0, 0, 0};                    // env e's frame stack (thread 0)
  if (tid == 0)
    for (int c = 0; c < 4; ++c) st_e[c] = x.stacks[(int64_t)e * x.K + min(c, x.K - 1)];
  float xr = 0.f, v = 0.f;
  if (wave == 0) {                                   // the Q row's loads first ...
    const float* row = a.act_lgi + (int64_t)e * mdqn_kd(a);
    xr = row[lane < A ? lane : 0];
    v = row[a.dueling ? kMdVO : 0];
  }
  actor_env_frames(x, e, pre);                       // ... the frames under their latency
  if (wave == 0) {
    if (a.dueling) xr += v - wave_sum_dpp(lane < A ? xr : 0.f) / (float)A;
    if (lane < A) qs[lane] = xr;
  }
  __syncthreads();
  actor_env_finish(x, qs, e, pre, st_e, &flag, st);
}

DQN_DEV_HOST_INLINE int mdqn_learn_blocks(int B) {
  const int n = (B + kMdWaves - 1) / kMdWaves;
  return n < kMdMaxParts ? n : kMdMaxParts;
}

__global__ void __launch_bounds__(kMdThreads) mdqn_train_kernel(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int nlearn = (int)gridDim.x - (a.act_E > 0 ? a.act_E : 0);
  if ((int)blockIdx.x >= nlearn) {
    mdqn_act_env_block(a, (int)blockIdx.x - nlearn, *reinterpret_cast<SumtreeLds*>(sm));
    return;
  }
  const int B = a.B, A = a.A, KD = mdqn_kd(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool hi = lane >= 32;                   // upper half-wave: target(s); lower: target(s') and online(s)
  const int i = lane & 31;
  const bool on = i < A;
  const int ii = on ? i : 0;                    // clamped: loads of idle lanes stay in bounds
  const float* ltg = a.lgi[hi ? 2 : 1];
  const float* lon = a.lgi[0];
  const int vcol = a.dueling ? kMdVO : 0;       // (no dueling: an ignored in-row load)
  const float tau = a.m_tau, delta = a.delta;
  const float inva = a.dueling ? 1.f / (float)A : 0.f;
  act_t* dout = reinterpret_cast<act_t*>(a.dq16);
  float contrib = 0.f;
  for (int b = blockIdx.x * kMdWaves + wave; b < B; b += nlearn * kMdWaves) {
    const int64_t r0 = (int64_t)b * KD;
    float xt = ltg[r0 + ii], xo = lon[r0 + ii];
    const float vt = ltg[r0 + vcol], vo = lon[r0 + vcol];
    const int act = a.act[b];
    const float rw = a.rew[b], gm = a.gam[b] * (1.f - a.done[b]);
    const float w = a.wts != nullptr ? a.wts[b] : 1.f;
    if (a.dueling) {                            // x_i += v - mean_j x_j
      const Half2 st = half_sum_dpp(on ? xt : 0.f), so = half_sum_dpp(on ? xo : 0.f);
      xt += vt - (hi ? st.hi : st.lo) * inva;
      xo += vo - so.lo * inva;
    }
    // 1. both log-sum-exps of the target net: max, then the sum of exp((q - max) / tau) <= A
    const Half2 mx = half_max_dpp(on ? xt : -INFINITY);
    const Half2 se = half_sum_dpp(on ? expf((xt - (hi ? mx.hi : mx.lo)) / tau) : 0.f);
    // 2. the taken action's online Q (lower half) and target Q on s (upper half): one non-zero
    //    term each, so the sums are exact
    const Half2 qa = half_sum_dpp(on && i == act ? (hi ? xt : xo) : 0.f);
    // 3. target, TD error, loss and its derivative (wave-uniform)
    const float soft = mx.lo + tau * logf(se.lo);
    const float lp = (qa.hi - mx.hi) - tau * logf(se.hi);
    const float y = rw + a.m_alpha * fminf(fmaxf(lp, a.m_clip), 0.f) + gm * soft;
    const float d = qa.lo - y;
    const float ad = fabsf(d);
    float per, g;
    if (a.huber) {                              // c (|d| - c / 2): d^2 / 2 below delta, delta (|d| - delta / 2) above
      const float c = fminf(ad, delta);
      per = c * (ad - 0.5f * c);
      g = copysignf(c, d);
    } else {
      per = d * d;
      g = 2.f * d;
    }
    const float dl = w / (float)B * g * kLossScale;
    if (lane == 0) a.prio[b] = ad;
    contrib += w * per;
    act_t* drow = dout + r0;
    if (!hi && on) drow[i] = (act_t)(dl * ((i == act ? 1.f : 0.f) - inva));
    if (a.dueling && lane == 0) drow[kMdVO] = (act_t)dl;
  }
  __shared__ float red[kMdWaves];
  if (lane == 0) red[wave] = contrib;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < kMdWaves; ++k) t += red[k];
    a.loss_parts[blockIdx.x] = t;
  }
}

}  // namespace dqn

using namespace dqn;

size_t mdqn_head_lds_bytes(const HeadArgs& a) {
  // training: the acting blocks' PER insert scratch (the rest is static); infer: Q and the row
  // offsets, then the fused actor's PER insert scratch
  const size_t per = a.actor.tsum != nullptr ? sizeof(SumtreeLds) : 0;
  if (!a.infer) return a.act_E > 0 ? per : 0;
  return mdqn_infer_q_bytes(a) + (a.has_actor ? per : 0);
}

void launch_mdqn_head(const HeadArgs& a, hipStream_t st) {
  const size_t lds = mdqn_head_lds_bytes(a);
  if (a.infer) {
    hipLaunchKernelGGL(mdqn_infer_kernel, dim3(1), dim3(1024), lds, st, a);
    return;
  }
  const dim3 grid(mdqn_learn_blocks(a.B) + (a.act_E > 0 ? a.act_E : 0));   // learner blocks + one per env
  hipLaunchKernelGGL(mdqn_train_kernel, grid, dim3(kMdThreads), lds, st, a);
}
