// Wide QR-DQN head of the HIP executor: 64 < N <= 256 quantiles per action, N % 4 == 0 (the paper's
// QR-DQN-1 uses N = 200). The sibling of qr_head.hip (N <= 64, one lane per quantile) on the same
// HeadArgs, the same output rows (qr_vo / qr_kd layout below) and the same outputs; the loss
// formulas are those of qr_head.hip's header. Torch oracle: dist_dqn_amd/models/losses.py (qr_loss).
//
//   qr_wide_train_kernel  training head, ONE WORKGROUP PER SAMPLE of W = ceil(N / 64) waves in a
//                         block-stride loop (at most 64 learner blocks = loss partials), plus one
//                         block per fused-acting env.
//   qr_wide_infer_kernel  acting / q_values: Q = mean over quantiles -> q_out / fused actor step.
//
// Two lane layouts per sample:
//   * streaming over actions: lane l of a wave owns the quantiles 4l .. 4l + 3 of a row (one
//     16-byte load; N % 4 == 0 and VO % 32 == 0 keep every row start 16-byte aligned; lanes at or
//     beyond N / 4 read lane 0's columns, in bounds, and contribute nothing). Wave w takes the
//     actions i = w (mod W), four at a time so their loads are in flight together, and keeps no
//     per-action state: the selection instance's row sums go to LDS, and with dueling the
//     per-quantile action sums of the target and online instances go there as one partial per wave.
//   * pairwise loop: thread i of the workgroup owns theta_i, thread j forms T_j and stages it in
//     LDS (N floats); every thread then walks the T_j as 16-byte LDS broadcast reads (all lanes
//     the same address: no bank conflict) with four independent accumulator chains.
// Action choice: the dueling combine adds the same v - mean_a x_a to every action's row mean, so
// a* = argmax_i of the selection instance's plain row sums (first maximum wins; bit-identical rows
// give bit-identical sums).
// dL/dtheta of the taken action is dl (1 - 1/A), of every other action -dl / A (dueling) or 0:
// written straight from thread n's dl_n, no per-action state.
// No atomics; every sum's order depends on (A, N) only (per-wave partials in wave order, then the
// waves in order), so two launches give the same bits.
//
// Why a workgroup per sample over LDS and not one wave per sample with a read-lane broadcast over
// four T registers: the pairwise loop is N * N pair terms of ~10 VALU operations. One wave would
// run 4 N of them per lane in sequence (N = 200: 800 iterations); W waves on the CU's four SIMDs
// run N each, and at the minibatch sizes of the step (32) either shape leaves most CUs idle, so the
// per-sample latency is the launch's duration. Only this variant was built and timed (README,
// QR-DQN paragraph).
#include "common.h"
#include "actor_dev.h"
#include "../include/dqn_nets_k.h"

namespace dqn {

// Row layout of the precomputed output rows (qr_head.hip qr_vo / qr_kd): KD floats =
// [plain / advantage quantiles (A * N) | pad | dueling value quantiles (N) at VO | pad]
DQN_DEV_HOST_INLINE int qrw_vo(const HeadArgs& a) { return (a.A * a.atoms + 31) / 32 * 32; }
DQN_DEV_HOST_INLINE int qrw_kd(const HeadArgs& a) {
  return qrw_vo(a) + (a.dueling ? (a.atoms + 31) / 32 * 32 : 0);
}

constexpr int kQrwMaxN = 256, kQrwMaxWaves = kQrwMaxN / 64, kQrwMaxParts = 64;

DQN_DEV_HOST_INLINE int qrw_waves(int N) { return (N + 63) / 64; }
DQN_DEV_HOST_INLINE int qrw_learn_blocks(int B) { return B < kQrwMaxParts ? B : kQrwMaxParts; }

// LDS (floats) of the inference kernel: row means [B][A + 1] (the dueling value row last), Q [B][A]
DQN_DEV_HOST_INLINE size_t qrw_infer_floats(const HeadArgs& a) { return (size_t)a.B * (2 * a.A + 1); }
DQN_DEV_HOST_INLINE size_t qrw_infer_q_bytes(const HeadArgs& a) {
  return (qrw_infer_floats(a) * sizeof(float) + 15) / 16 * 16;
}

DQN_DEV float sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
DQN_DEV void add4(float4& s, const float4& v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
DQN_DEV float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// Acting / q_values: one block (qr_head.hip qr_infer_kernel with the 16-lane row sum looped over
// N / 16 columns). The dueling combine is linear, so it runs on the row means:
// Q_i = mean_n x_i + mean_n v - mean_a mean_n x_a.
__global__ void __launch_bounds__(1024) qr_wide_infer_kernel(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int B = a.B, A = a.A, NA = a.atoms, R = A + (a.dueling ? 1 : 0);
  const int VO = qrw_vo(a), KD = qrw_kd(a);
  const int tid = threadIdx.x, nth = blockDim.x, l16 = tid & 15;
  float* m = sm;
  float* q = m + B * (A + 1);
  const float* src = a.lgi[0];
  const float invn = 1.f / (float)NA;
  for (int row = tid >> 4; row < B * R; row += nth >> 4) {      // uniform per 16-lane group
    const int b = row / R, i = row - b * R;
    const float* r = src + (int64_t)b * KD + (i < A ? i * NA : VO);
    float s = 0.f;
    for (int n = l16; n < NA; n += 16) s += r[n];
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
  if (a.has_actor) actor_step_block(a.actor, q, reinterpret_cast<char*>(sm) + qrw_infer_q_bytes(a));
}

// Fused acting, one block per env e (qr_head.hip qr_act_env_block): wave 0 streams env e's action
// rows into the Q row in LDS, while every thread writes the env's new frames; then the decision /
// replay append (actor_dev.h).
DQN_DEV void qr_wide_act_env_block(const HeadArgs& a, int e, SumtreeLds& st) {
  __shared__ float qs[32];
  __shared__ int flag;
  const ActorArgs& x = a.actor;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = a.A, NA = a.atoms;
  const ActorPre pre = actor_prefetch(x);
  int32_t st_e[4] = {0, 0, 0, 0};                    // env e's frame stack (thread 0)
  if (tid == 0)
    for (int c = 0; c < 4; ++c) st_e[c] = x.stacks[(int64_t)e * x.K + min(c, x.K - 1)];
  const bool on = 4 * lane < NA;
  const int c4 = on ? 4 * lane : 0;
  const float* row = a.act_lgi + (int64_t)e * qrw_kd(a);
  float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (wave == 0 && a.dueling) v4 = ld4(row + qrw_vo(a) + c4);       // the value row's load first ...
  actor_env_frames(x, e, pre);                       // ... the frames under its latency
  if (wave == 0) {
    const float invn = 1.f / (float)NA;
    float tot = 0.f, ql = 0.f;                       // lane i < A keeps Q_i (A <= 32)
    for (int i0 = 0; i0 < A; i0 += 4) {              // four action rows in flight
      float4 xr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) xr[u] = ld4(row + min(i0 + u, A - 1) * NA + c4);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float qi = wave_sum_dpp(on ? sum4(xr[u]) : 0.f) * invn;
        if (i0 + u < A) {
          tot += qi;
          if (lane == i0 + u) ql = qi;
        }
      }
    }
    if (a.dueling)                                   // Q_i = mean x_i + mean v - mean_a mean x_a
      ql += wave_sum_dpp(on ? sum4(v4) : 0.f) * invn - tot / (float)A;
    if (lane < A) qs[lane] = ql;
  }
  __syncthreads();
  actor_env_finish(x, qs, e, pre, st_e, &flag, st);
}

// ---------------------------------------------------------------- wide QR training head
// Outputs as qr_train_kernel: priorities to prio[b], per-block loss partials to
// loss_parts[block] (summed by the fc dgrad launch), dL/dtheta as act_t (loss-scaled) rows of
// dout16 [B][KD]: plain / advantage columns [0, A N) (dueling: times (i == a) - 1/A), value
// columns [VO, VO + N); pad columns are never written (zero from allocation).
__global__ void __launch_bounds__(64 * kQrwMaxWaves) qr_wide_train_kernel(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int nlearn = (int)gridDim.x - (a.act_E > 0 ? a.act_E : 0);
  if ((int)blockIdx.x >= nlearn) {
    qr_wide_act_env_block(a, (int)blockIdx.x - nlearn, *reinterpret_cast<SumtreeLds*>(sm));
    return;
  }
  __shared__ __attribute__((aligned(16))) float pt[kQrwMaxWaves][kQrwMaxN];   // per-wave action sums, target
  __shared__ __attribute__((aligned(16))) float po[kQrwMaxWaves][kQrwMaxN];   // ... online
  __shared__ __attribute__((aligned(16))) float Tz[kQrwMaxN];                 // T_j
  __shared__ float qsel[32];                                                  // selection row sums
  __shared__ float red[kQrwMaxWaves];
  const int B = a.B, A = a.A, NA = a.atoms;
  const int VO = qrw_vo(a), KD = qrw_kd(a);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = (int)blockDim.x >> 6;
  const bool on4 = 4 * lane < NA;               // streaming layout: this lane's four quantiles exist
  const int c4 = on4 ? 4 * lane : 0;            // clamped: loads of idle lanes stay in bounds
  const bool on = tid < NA;                     // pairwise layout: this thread's theta exists
  const int tn = on ? tid : 0;
  const bool dbl = a.lgi[2] != nullptr;
  const float* lsel = a.lgi[dbl ? 2 : 1];       // action choice on s'
  const float* ltgt = a.lgi[1];                 // target quantiles (same buffer without Double DQN)
  const float* lon = a.lgi[0];
  const bool duel = a.dueling != 0;

  const float kap = a.delta;
  const float invn = 1.f / (float)NA;
  const float tau = (float)(2 * tn + 1) * (0.5f * invn);
  const float inva = duel ? 1.f / (float)A : 0.f;
  const float sc = invn / kap;
  act_t* dout = reinterpret_cast<act_t*>(a.dq16);
  float contrib = 0.f;                          // (thread 0's is the block's)
  for (int b = blockIdx.x; b < B; b += nlearn) {               // uniform per block: the barriers are too
    const int64_t r0 = (int64_t)b * KD;
    const int act = a.act[b];
    const float rw = a.rew[b], gm = a.gam[b] * (1.f - a.done[b]);
    const float w = a.wts != nullptr ? a.wts[b] : 1.f;
    // the rows that do not wait for a*: the taken action's online row, the value rows
    const float xo_n = lon[r0 + act * NA + tn];
    float vt_n = 0.f, vo_n = 0.f;
    if (duel) { vt_n = ltgt[r0 + VO + tn]; vo_n = lon[r0 + VO + tn]; }
    // 1. streaming pass: wave w takes actions w, w + W, ..., four in flight
    float4 st = make_float4(0.f, 0.f, 0.f, 0.f), so = st;
    for (int i0 = wave; i0 < A; i0 += 4 * W) {
      float4 xs[4], xt[4], xo[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t o = r0 + min(i0 + u * W, A - 1) * NA + c4;
        xs[u] = ld4(lsel + o);
        if (duel) { xt[u] = ld4(ltgt + o); xo[u] = ld4(lon + o); }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * W;
        const float s = wave_sum_dpp(on4 ? sum4(xs[u]) : 0.f);
        if (i < A) {
          if (lane == 0) qsel[i] = s;
          if (duel) { add4(st, xt[u]); add4(so, xo[u]); }
        }
      }
    }
    if (duel && on4) {
      *reinterpret_cast<float4*>(&pt[wave][c4]) = st;
      *reinterpret_cast<float4*>(&po[wave][c4]) = so;
    }
    __syncthreads();
    // 2. a* (first maximum wins), then T_j and theta_i, one quantile per thread
    int best = 0;
    float bq = -INFINITY;
    for (int i = 0; i < A; ++i) {
      const float qi = qsel[i];
      if (qi > bq) { bq = qi; best = i; }
    }
    float xt_n = ltgt[r0 + best * NA + tn], th = xo_n;
    if (duel) {                                 // x += v - mean_a x_a, per quantile
      float mt = 0.f, mo = 0.f;
      const int nw = A < W ? A : W;             // (waves beyond A took no action: nothing stored)
      for (int k = 0; k < nw; ++k) { mt += pt[k][tn]; mo += po[k][tn]; }
      xt_n += vt_n - mt * inva;
      th += vo_n - mo * inva;
    }
    if (on) Tz[tid] = rw + gm * xt_n;
    __syncthreads();
    // 3. pairwise quantile Huber loss: thread i = theta_i against every T_j
    float rho[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < NA; j += 4) {
      const float4 t4 = *reinterpret_cast<const float4*>(&Tz[j]);
      const float tj[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float u = tj[k] - th;
        const float au = fabsf(u);
        const float c = fminf(au, kap);
        const float wq = u < 0.f ? 1.f - tau : tau;
        rho[k] += wq * (c * (au - 0.5f * c));
        g[k] += wq * copysignf(c, u);
      }
    }
    const float rs = wave_sum_dpp(on ? (rho[0] + rho[1]) + (rho[2] + rho[3]) : 0.f);
    if (lane == 0) red[wave] = rs;
    const float gs = (g[0] + g[1]) + (g[2] + g[3]);
    const float dl = w / (float)B * (-gs * sc) * kLossScale;
    act_t* drow = dout + r0;
    if (on) {
      const act_t oth = (act_t)(dl * -inva), tak = (act_t)(dl * (1.f - inva));
      for (int i = 0; i < A; ++i) drow[i * NA + tid] = i == act ? tak : oth;
      if (duel) drow[VO + tid] = (act_t)dl;
    }
    __syncthreads();
    if (tid == 0) {
      float per = 0.f;
      for (int k = 0; k < W; ++k) per += red[k];
      per *= sc;
      a.prio[b] = per;
      contrib += w * per;
    }
  }
  if (tid == 0) a.loss_parts[blockIdx.x] = contrib;
}

}  // namespace dqn

using namespace dqn;

size_t qr_wide_head_lds_bytes(const HeadArgs& a) {
  // training: the acting blocks' PER insert scratch (the rest is static); infer: the row means
  // and Q, then the fused actor's PER insert scratch
  const size_t per = a.actor.tsum != nullptr ? sizeof(SumtreeLds) : 0;
  if (!a.infer) return a.act_E > 0 ? per : 0;
  return qrw_infer_q_bytes(a) + (a.has_actor ? per : 0);
}

void launch_qr_wide_head(const HeadArgs& a, hipStream_t st) {
  const size_t lds = qr_wide_head_lds_bytes(a);
  if (a.infer) {
    hipLaunchKernelGGL(qr_wide_infer_kernel, dim3(1), dim3(1024), lds, st, a);
    return;
  }
  const dim3 grid(qrw_learn_blocks(a.B) + (a.act_E > 0 ? a.act_E : 0));   // learner blocks + one per env
  hipLaunchKernelGGL(qr_wide_train_kernel, grid, dim3(64 * qrw_waves(a.atoms)), lds, st, a);
}
