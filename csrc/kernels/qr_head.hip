// QR-DQN head of the HIP executor (quantile regression, Dabney et al. 2018): the sibling of the
// C51 head in rainbow.hip, on the same precomputed output-layer rows and with the same outputs.
// Torch oracle: dist_dqn_amd/models/losses.py (qr_loss).
//
//   qr_train_kernel  training head, one wave64 per sample (lanes = quantiles, N <= 64): dueling
//                    combine per quantile, Double-DQN action choice on the quantile means, the
//                    N x N pairwise quantile Huber loss (= the priority) and dL/dtheta as the
//                    act_t dZ rows the dH igemm and the output layer's grouped weight-gradient
//                    members consume; one more block per fused-acting env.
//   qr_infer_kernel  acting / q_values: Q = mean over quantiles -> q_out / fused actor step.
//
// Loss of one sample (theta = online quantiles of the taken action, T = r + gamma (1 - done) *
// target quantiles of a*, tau_i = (2 i + 1) / 2 N, u_ij = T_j - theta_i, c_ij = min(|u_ij|, kappa)):
//   rho_ij = |tau_i - 1{u_ij < 0}| c_ij (|u_ij| - c_ij / 2) / kappa      (Huber, both branches)
//   per    = sum_i 1/N sum_j rho_ij
//   dper / dtheta_i = -1/N sum_j |tau_i - 1{u_ij < 0}| copysign(c_ij, u_ij) / kappa
// HeadArgs: atoms = N, delta = kappa (vmin / vmax unused).
#include "common.h"
#include "actor_dev.h"
#include "../include/dqn_nets_k.h"

namespace dqn {

// Row layout of the precomputed output rows: the C51 head's (rainbow.hip c51_vo / c51_kd): KD
// floats = [plain / advantage quantiles (A * N) | pad | dueling value quantiles (N) at VO | pad]
DQN_DEV_HOST_INLINE int qr_vo(const HeadArgs& a) { return (a.A * a.atoms + 31) / 32 * 32; }
DQN_DEV_HOST_INLINE int qr_kd(const HeadArgs& a) {
  return qr_vo(a) + (a.dueling ? (a.atoms + 31) / 32 * 32 : 0);
}

// LDS (floats) of the inference kernel: row means [B][A + 1] (the dueling value row last), Q [B][A]
DQN_DEV_HOST_INLINE size_t qr_infer_floats(const HeadArgs& a) { return (size_t)a.B * (2 * a.A + 1); }
DQN_DEV_HOST_INLINE size_t qr_infer_q_bytes(const HeadArgs& a) {
  return (qr_infer_floats(a) * sizeof(float) + 15) / 16 * 16;
}

// Acting / q_values: one block. Sixteen lanes per row (quantile n = l16 + 16 u, u < 4) sum it on
// DPP row ops; the dueling combine is linear, so it runs on the row means:
// Q_i = mean_n x_i + mean_n v - mean_a mean_n x_a.
__global__ void __launch_bounds__(1024) qr_infer_kernel(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int B = a.B, A = a.A, NA = a.atoms, R = A + (a.dueling ? 1 : 0);
  const int VO = qr_vo(a), KD = qr_kd(a);
  const int tid = threadIdx.x, nth = blockDim.x, l16 = tid & 15;
  float* m = sm;
  float* q = m + B * (A + 1);
  const float* src = a.lgi[0];
  const float invn = 1.f / (float)NA;
  for (int row = tid >> 4; row < B * R; row += nth >> 4) {      // uniform per 16-lane group
    const int b = row / R, i = row - b * R;
    const float* r = src + (int64_t)b * KD + (i < A ? i * NA : VO);
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = l16 + 16 * u;
      s += n < NA ? r[n] : 0.f;
    }
    s = row16_sum(s);
    if (l16 == 0) m[b * (A + 1) + i] = s * invn;
  }
  __syncthreads();
  for (int t = tid; t < B * A; t += nth) {
    const int b = t / A, i = t - b * A;
    const float* mb = m + b * (A + 1);
    float v = 0.f;
    if (a.dueling) {
      float mean = 0.f;
      for (int k = 0; k < A; ++k) mean += mb[k];
      v = mb[A] - mean / (float)A;
    }
    q[t] = mb[i] + v;
  }
  __syncthreads();
  if (a.q_out != nullptr)
    for (int t = tid; t < B * A; t += nth) a.q_out[t] = q[t];
  // (the PER tree insert's scratch lies behind Q, which the actor step is still reading)
  if (a.has_actor) actor_step_block(a.actor, q, reinterpret_cast<char*>(sm) + qr_infer_q_bytes(a));
}

// ---------------------------------------------------------------- QR training head
// The C51 training head's launch shape (rainbow.hip c51_train_kernel): learner blocks of eight
// waves, ONE WAVE PER SAMPLE in a block-stride loop, lanes = quantiles, plus one block per
// fused-acting env; per-block loss partials to loss_parts[block] (summed by the fc dgrad launch),
// priorities to prio[b], dL/dtheta as act_t (loss-scaled) rows of dout16 [B][KD]: plain /
// advantage columns [0, A N) (dueling: times (i == a) - 1/A), value columns [VO, VO + N); pad
// columns are never written (zero from allocation).
//   * all of the sample's loads (selection / target / online instances, every action row +
//     dueling value row) issued up front; lanes >= N read lane 0's column (in bounds);
//   * dueling combine per quantile; Q_i = mean of the selection instance's row -> a* (first
//     maximum wins; no early exit: the AM reduction chains interleave);
//   * lane j forms T_j; the pairwise loop broadcasts T_j by a read-lane (j is wave-uniform: no
//     LDS, no atomics) while lane i accumulates its row of rho and of the gradient.
constexpr int kQrWaves = 8, kQrThreads = 64 * kQrWaves, kQrMaxParts = 64;

// Fused acting, one block per env e: env e's rows -> wave 0 -> Q row in LDS, while every thread
// writes the env's new frames; then the decision / replay append (actor_dev.h).
template <int AM>
DQN_DEV void qr_act_env_block(const HeadArgs& a, int e, SumtreeLds& st) {
  __shared__ float qs[32];
  __shared__ int flag;
  const ActorArgs& x = a.actor;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = a.A, NA = a.atoms;
  const ActorPre pre = actor_prefetch(x);
  int32_t st_e[4] = {0, 0, 0, 0};                    // env e's frame stack (thread 0)
  if (tid == 0)
    for (int c = 0; c < 4; ++c) st_e[c] = x.stacks[(int64_t)e * x.K + min(c, x.K - 1)];
  const bool on = lane < NA;
  const int ln = on ? lane : 0;
  float xr[AM], v = 0.f;
  if (wave == 0) {                                   // the Q row's loads first ...
    const float* row = a.act_lgi + (int64_t)e * qr_kd(a);
#pragma unroll
    for (int i = 0; i < AM; ++i) xr[i] = row[min(i, A - 1) * NA + ln];
    v = a.dueling ? row[qr_vo(a) + ln] : 0.f;
  }
  actor_env_frames(x, e, pre);                       // ... the frames under their latency
  if (wave == 0) {
    if (a.dueling) {
      float mean = 0.f;
#pragma unroll
      for (int i = 0; i < AM; ++i) mean += i < A ? xr[i] : 0.f;
      v -= mean / (float)A;
    }
    const float invn = 1.f / (float)NA;
#pragma unroll
    for (int i = 0; i < AM; ++i) {
      const float qi = wave_sum_dpp(on ? xr[i] + v : 0.f) * invn;
      if (lane == 0 && i < A) qs[i] = qi;
    }
  }
  __syncthreads();
  actor_env_finish(x, qs, e, pre, st_e, &flag, st);
}

DQN_DEV_HOST_INLINE int qr_learn_blocks(int B) {
  const int n = (B + kQrWaves - 1) / kQrWaves;
  return n < kQrMaxParts ? n : kQrMaxParts;
}

template <int AM>
__global__ void __launch_bounds__(kQrThreads) qr_train_kernel(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int nlearn = (int)gridDim.x - (a.act_E > 0 ? a.act_E : 0);
  if ((int)blockIdx.x >= nlearn) {
    qr_act_env_block<AM>(a, (int)blockIdx.x - nlearn, *reinterpret_cast<SumtreeLds*>(sm));
    return;
  }
  const int B = a.B, A = a.A, NA = a.atoms;
  const int VO = qr_vo(a), KD = qr_kd(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool on = lane < NA;
  const int ln = on ? lane : 0;                 // clamped: loads of idle lanes stay in bounds
  const bool dbl = a.lgi[2] != nullptr;
  const float* lsel = a.lgi[dbl ? 2 : 1];       // action choice on s'
  const float* ltgt = a.lgi[1];                 // target quantiles (same buffer without Double DQN)
  const float* lon = a.lgi[0];

  const float kap = a.delta;
  const float invn = 1.f / (float)NA;
  const float tau = (float)(2 * ln + 1) * (0.5f * invn);
  const float inva = a.dueling ? 1.f / (float)A : 0.f;
  act_t* dout = reinterpret_cast<act_t*>(a.dq16);
  float contrib = 0.f;
  for (int b = blockIdx.x * kQrWaves + wave; b < B; b += nlearn * kQrWaves) {
    float xs[AM], xt[AM], xo[AM];
    const int64_t r0 = (int64_t)b * KD + ln;
#pragma unroll
    for (int i = 0; i < AM; ++i) {
      const int ii = i < A ? i : 0;
      xs[i] = lsel[r0 + ii * NA];
      xt[i] = ltgt[r0 + ii * NA];
      xo[i] = lon[r0 + ii * NA];
    }
    const int64_t v0 = (int64_t)b * KD + (a.dueling ? VO : 0) + ln;   // (no dueling: an ignored in-row load)
    float vs = lsel[v0], vt = ltgt[v0], vo = lon[v0];
    const int act = a.act[b];
    const float rw = a.rew[b], gm = a.gam[b] * (1.f - a.done[b]);
    const float w = a.wts != nullptr ? a.wts[b] : 1.f;
    if (a.dueling) {                            // x_i += v - mean_j x_j, per quantile
      float ms = 0.f, mt = 0.f, mo = 0.f;
#pragma unroll
      for (int i = 0; i < AM; ++i)
        if (i < A) { ms += xs[i]; mt += xt[i]; mo += xo[i]; }
      vs -= ms * inva; vt -= mt * inva; vo -= mo * inva;
#pragma unroll
      for (int i = 0; i < AM; ++i) { xs[i] += vs; xt[i] += vt; xo[i] += vo; }
    }
    // 1. action choice: Q_i = mean_n theta_sel(s', i)_n, first maximum wins
    int best = 0;
    float bq = -INFINITY;
#pragma unroll
    for (int i = 0; i < AM; ++i) {
      const float qi = wave_sum_dpp(on ? xs[i] : 0.f) * invn;
      if (i < A && qi > bq) { bq = qi; best = i; }
    }
    // 2. a*'s target row, the taken action's online row (register select: no dynamic indexing)
    float xa = xt[0], xb = xo[0];
#pragma unroll
    for (int i = 1; i < AM; ++i) {
      if (i == best) xa = xt[i];
      if (i == act) xb = xo[i];
    }
    // 3. pairwise quantile Huber loss: lane i = theta_i against every T_j
    const int tzi = __float_as_int(rw + gm * xa);
    float rho = 0.f, g = 0.f;
    for (int j = 0; j < NA; ++j) {
      const float u = __int_as_float(__builtin_amdgcn_readlane(tzi, j)) - xb;
      const float au = fabsf(u);
      const float c = fminf(au, kap);
      const float wq = u < 0.f ? 1.f - tau : tau;
      rho += wq * (c * (au - 0.5f * c));
      g += wq * copysignf(c, u);
    }
    const float sc = invn / kap;
    const float per = wave_sum_dpp(on ? rho : 0.f) * sc;
    const float dl = w / (float)B * (-g * sc) * kLossScale;
    if (lane == 0) a.prio[b] = per;
    contrib += w * per;
    act_t* drow = dout + (int64_t)b * KD;
    if (on) {
#pragma unroll
      for (int i = 0; i < AM; ++i)
        if (i < A) drow[i * NA + lane] = (act_t)(dl * ((i == act ? 1.f : 0.f) - inva));
      if (a.dueling) drow[VO + lane] = (act_t)dl;
    }
  }
  __shared__ float red[kQrWaves];
  if (lane == 0) red[wave] = contrib;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < kQrWaves; ++i) t += red[i];
    a.loss_parts[blockIdx.x] = t;
  }
}

}  // namespace dqn

using namespace dqn;

size_t qr_head_lds_bytes(const HeadArgs& a) {
  // training: the acting blocks' PER insert scratch (the rest is static); infer: the row means
  // and Q, then the fused actor's PER insert scratch
  const size_t per = a.actor.tsum != nullptr ? sizeof(SumtreeLds) : 0;
  if (!a.infer) return a.act_E > 0 ? per : 0;
  return qr_infer_q_bytes(a) + (a.has_actor ? per : 0);
}

void launch_qr_head(const HeadArgs& a, hipStream_t st) {
  const size_t lds = qr_head_lds_bytes(a);
  if (a.infer) {
    hipLaunchKernelGGL(qr_infer_kernel, dim3(1), dim3(1024), lds, st, a);
    return;
  }
  const dim3 grid(qr_learn_blocks(a.B) + (a.act_E > 0 ? a.act_E : 0));   // learner blocks + one per env
#define QRK(AM) hipLaunchKernelGGL(qr_train_kernel<AM>, grid, dim3(kQrThreads), lds, st, a)
  if (a.A <= 4) QRK(4);
  else if (a.A <= 8) QRK(8);
  else if (a.A <= 18) QRK(18);
  else QRK(32);
#undef QRK
}
