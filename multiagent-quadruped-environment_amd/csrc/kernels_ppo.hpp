// kernels_ppo.hpp -- the clipped-surrogate PPO loss of rsl_rl, its gradient with respect to the engine's actor-critic parameters, and the Adam step
// on them (mqe_ppo_grad, mqe_ppo_adam; include/mqe_hip.h).  This file holds the primitives of the gradient kernel -- the LDS rule, backward-data
// (ppo_dx), the weight gradient (ppo_dw), the tile load, the two loss heads and the statistics -- and the kernels behind it: k_ppo_reduce, k_ppo_norm,
// k_ppo_adam.  The walk over the layers and the entry points k_ppo_grad / k_ln_grad are in kernels_actor_critic.hpp, behind the norm (kernels_ln.hpp).
//
// THE LOSS.  A sample is a flat index s = t * R' + r into a trajectory in mqe_rollout's layout, 0 <= s < T * R': its observation is the D
// floats at packed + t * row_stride + r * D; actions[s][3], logp_old[s], v_old = value[s] (the first T rows of the [T + 1][R'] array), adv[s],
// ret[s].  THE SELECTION (ppo_unit below, the one statement of it).  A minibatch is `count` UNITS out of the trajectory's n: unit i is
// index[first + i] when an int32 index list is given (a slice of a device permutation; a value outside [0, n) is the caller's error -- the kernel
// clamps it, so that it cannot read outside the trajectory), otherwise first + i.  The units are samples (n = T R') here, groups under THE JOINT
// RATIO below (n = T N), chunks under MQE_PPO_BPTT (kernels_bptt.hpp: n = (T / L) R', with both flags chunk groups, n = (T / L) N); M is the
// minibatch's number of samples.  Per sample, all f32:
//     mean = actor(obs), v = critic(obs)        the fmaf chains of k_actor (kernels_actor.hpp: actor_layer, unchanged)
//     z_j  = (a_j - mean_j) * exp(-log_std_j)
//     logp = sum_j (-0.5 z_j^2 - log_std_j) - 1.5 ln(2 pi)        (j ascending, from 0, as k_actor);   ratio = exp(logp - logp_old)
//     L_pi = -min(ratio * adv, clamp(ratio, 1 - c, 1 + c) * adv)
//     L_v  = (v - ret)^2;   with MQE_PPO_CLIP_VALUE:  max((v - ret)^2, (v_c - ret)^2),  v_c = v_old + clamp(v - v_old, -c_v, c_v)
//     H    = sum_j log_std_j + 1.5 (1 + ln(2 pi))                   (state-independent)
//     L    = mean(L_pi) + value_coef * mean(L_v) - entropy_coef * H
// THE GRADIENT is what autograd gives away from the kinks; the kinks are decided by selects, never by products with a mask:
//     dL/dlogp       = 0 when (adv > 0 and ratio > 1 + c) or (adv < 0 and ratio < 1 - c), otherwise -adv * ratio * (1 / M)
//     dlogp/dmean_j  = z_j * exp(-log_std_j);    dlogp/dlog_std_j = z_j^2 - 1;    log_std_j additionally receives -entropy_coef
//     dL/dv          = value_coef * (1 / M) * { 2 (v - ret) when the unclipped square is the larger one (ties: unclipped) or the flag is off;
//                                               2 (v_c - ret) when |v - v_old| < c_v;  0 otherwise }
//     hidden layers:   delta_in = (W^T delta_out) * (1 - y^2) (tanh, from the stored output y) or (y > 0 ? . : 0) (relu)
// 1 / M is one f32 value, formed on the host as (float)(1.0 / M).
//
// THE JOINT RATIO (MQE_PPO_JOINT; OpenRL's use_joint_action_loss, jrpo.yaml).  R' = N A' rows a step, s = t R' + n A' + a.  A GROUP is the A' samples of
// one env-step: g = t N + n, samples g A' + a; A' divides 32.  THE GROUP IS THE MINIBATCH'S UNIT: index / first / count are group numbers in [0, T N)
// (a ratio over half an env-step's agents does not exist), k_joint_expand writes the flat list g A' + a, group-major, clamped, and the gradient kernel
// reads that list as its index with count A' entries -- a group is A' aligned lanes of one tile, wholly valid or wholly padding.  Per sample
// d_a = logp_a - logp_old_a as above; per group, pairwise in the xor butterfly's order:
//     Delta = d_0 | d_0 + d_1 | (d_0 + d_1) + (d_2 + d_3) | ...;   rho = exp(Delta);   A = (adv_0 + ...) * (float)(1.0 / A'), the same order
//     L_pi(g) = -min(rho A, clamp(rho, 1 - c, 1 + c) A);   the policy term of L is the mean over the G = count groups, 1 / G = (float)(1.0 / G)
//     dL/dlogp_a = 0 when (A > 0 and rho > 1 + c) or (A < 0 and rho < 1 - c), otherwise -A rho (1 / G), for every agent a of the group
// Every lane of a group holds the same bits of Delta, rho and A, so no two agents decide a kink differently.  The value term stays the mean over the
// M = G A' samples; the entropy term is unchanged.  Statistics: every lane adds its GROUP's L_pi, -Delta and |rho - 1| > c; k_ppo_reduce divides by M,
// which is the mean over groups.  At A' = 1 every quantity has the bits of the plain path.
// THE DUAL CLIP (MQE_PPO_DUAL_CLIP, coefficient c_d > 1 + c; OpenRL's dual_clip_ppo / dual_clip_coeff, dppo.yaml).  Where the advantage is negative,
//     L_pi = -max(min(rho A, clamp(rho) A), c_d A),   and dL/dlogp is additionally 0 when A < 0 and rho > c_d
// (for c_d > 1 + c value for value OpenRL's ratio = min(ratio, c_d) form); without the joint ratio rho = ratio and A = adv of the single sample.
//
// LAYOUT.  A workgroup is 1024 threads = 16 wavefronts (k_actor's) and walks row tiles of RT samples (kernels_actor_critic.hpp: the tile loop and the
// order of the phases).  LDS holds, as [k][row] with an odd row stride, the observation and EVERY layer output of ONE network -- the backward pass
// needs them.  No separate delta buffers: the delta of layer l - 1 overwrites the stored output of layer l - 1 IN PLACE, element by element by
// the thread that reads that element for the activation derivative, after the weight gradient of layer l (the last reader of that output as
// an input) is done.  So the footprint is
// (D + sum of hidden widths + 4) rows; RT = 64 (stride 65) when that fits 160 KiB -- every network up to 128 x 128 x 128, the 64 x 64 case
// included -- else RT = 32 (stride 33: lanes 32 .. 63 repeat rows 0 .. 31 in the lane = row phases), which holds the widest accepted stack
// (128 + 3 x 256 + 4 rows = 116 KiB).  A 16-row tile is never needed.
// FORWARD: actor_layer, lane = row, weights wave-uniform.  BACKWARD-DATA (ppo_dx): lane = row as well; a wavefront owns four input neurons k
// and runs  acc = 0; for o ascending: acc = fmaf(W[o][k], delta[o], acc)  -- one LDS read feeds four FMAs, weights wave-uniform again.
// WEIGHT GRADIENT (ppo_dw): dW[o][k] = sum over rows of delta[o][row] x[k][row] is a reduction ACROSS the lanes of the other phases, so the
// threads are mapped again: a thread owns a 4 x 4 block (o = 4 ob .. 4 ob + 3; k = kb, kb + nbk, kb + 2 nbk, kb + 3 nbk with nbk = ceil(K / 4), so that
// consecutive lanes read consecutive LDS banks and store consecutive floats) and runs, per element, ONE fmaf chain over the rows in ascending
// order:  acc = fmaf(delta[o][row], x[k][row], acc)  (db: acc += delta[o][row]).  The chain continues over all tiles of the workgroup: the
// accumulators start at 0 on the workgroup's first tile and are otherwise read from, and written back to, the workgroup's partial
// gradient in per-handle scratch by the thread that owns them (L2-resident; no atomics, the same thread every time).  8 LDS reads feed 16
// FMAs.  WHY VALU AND NOT THE f32 MFMA: on this chip v_mfma_f32_32x32x2_f32 runs at 64 FLOP / clk / SIMD, exactly the f32 vector rate, so the
// matrix cores buy no arithmetic; they would save LDS reads (2 per 32 x 32 x 2 step against 8 per 16 FMAs) at the price of operands padded
// to 32 x 32 for widths such as 3, 7, 14 and 17 and of rows (the MFMA's k) fed from two LDS arrays through a lane layout that the lane = row
// phases do not produce.  Per 64-row tile of a 64 x 64 layer: 2048 wave-level ds_read (4096 clk of the CU's LDS port) against 4096
// wave-level FMAs (2048 clk over 4 SIMDs): the weight gradient is LDS-bound at about twice its arithmetic time, which is what DESIGN 3.5's
// roofline carries.
// REDUCTION (k_ppo_reduce, a second launch): grad[i] = (float) sum over workgroups b ascending of (double) partial[b][i]; the statistics
// and the three log_std gradients are f64 per lane of wavefront 0 over the workgroup's tiles, added across lanes by the xor butterfly
// 32, 16, ..., 1 (k_gae's), stored per workgroup and added in workgroup order.  No floating-point atomics anywhere: the same bits every run.
// Rows past the end of the minibatch load the last sample (clamped) and carry delta = 0: they contribute +0 to every chain.
//
// ADAM (k_ppo_norm, k_ppo_adam).  norm = sqrt(sum g_i^2) in f64: thread t of ONE 1024-thread workgroup adds i = t, t + 1024, ... ascending
// (fma), then a fixed LDS tree (stride 512, 256, ..., 1).  scale = min(1, max_grad_norm / ((float) norm + 1e-6f)) (f32; 1 when clipping is off).
// Per element, f32:  g = grad * scale;  m = fmaf(b1, m, (1 - b1) * g);  v = fmaf(b2, v, ((1 - b2) * g) * g);
//     p = p - (step_size * m) / (sqrtf(v) / bc2s + eps)     step_size = lr / (1 - b1^step), bc2s = sqrt(1 - b2^step), 1 - b1, 1 - b2: formed on the
// host in f64 and passed as f32.
#pragma once
#include "mqe_common.hpp"
#include "kernels_actor.hpp"

#define PPO_MAX_WG 256                 // persistent workgroups of k_ppo_grad at most: the chip's 256 CUs, one 1024-thread workgroup each
#define PPO_LDS_LIMIT (160 * 1024)
#define PPO_PST 8                      // doubles per workgroup in the statistics scratch: L_pi, L_v, logp_old - logp, clipped, dlog_std[3], pad
#define PPO_REDUCE_THREADS 256
#define PPO_ADAM_THREADS 256
#define PPO_NORM_THREADS 1024

// the two loss switches of mqe_ppo_grad's flags: stated in the comment of include/mqe_hip.h in words, defined here (the header's define set is pinned by the
// tests), mirrored in mqe/engine/abi.py
#define MQE_PPO_JOINT 64               // index_dev / first / count are groups (THE JOINT RATIO above)
#define MQE_PPO_DUAL_CLIP 128          // loss points at an mqe_ppo_loss_ex (THE DUAL CLIP above)
#define JOINT_EXPAND_THREADS 256

// THE SELECTION: unit i of a minibatch out of n.  No __restrict__ and this statement order: what the gradient kernels were compiled from before
// the rule had a name (a second no-alias scope moves their schedules: the comment above ppo_grad_body, kernels_actor_critic.hpp)
__device__ __forceinline__ long long ppo_unit(const int32_t* index, long long first, long long i, long long n) {
  long long u = first + i;
  if (index != nullptr) {
    u = index[first + i];
    u = u < 0 ? 0 : (u > n - 1 ? n - 1 : u);
  }
  return u;
}

// the minibatch's count A' flat numbers g A' + a, group-major (samples; under MQE_PPO_BPTT chunks): what the gradient kernels, k_bptt_expand and
// k_vn_moments / k_vn_apply read as their index list.  n_groups: T N, or (T / L) N
__global__ void __launch_bounds__(JOINT_EXPAND_THREADS) k_joint_expand(const int32_t* __restrict__ index, long long first, long long count, long long n_groups, int Aw,
                                                                       int32_t* __restrict__ out) {
  for (long long e = (long long)blockIdx.x * JOINT_EXPAND_THREADS + threadIdx.x; e < count * Aw; e += (long long)gridDim.x * JOINT_EXPAND_THREADS) {
    const long long i = e / Aw;
    const long long g = ppo_unit(index, first, i, n_groups);
    out[e] = (int32_t)(g * Aw + (e - i * Aw));
  }
}

// rows of the LDS image: observation, every hidden output of the larger network, 4 output rows (mean 0 .. 2, value)
static inline int ppo_lds_rows(const ActorNet& a, const ActorNet& c, int D) {
  int ha = 0, hc = 0;
  for (int l = 1; l < a.n_layers; l++) ha += a.dims[l];
  for (int l = 1; l < c.n_layers; l++) hc += c.dims[l];
  return D + (ha > hc ? ha : hc) + 4;
}
static inline size_t ppo_lds_bytes(int rows, int rt) { return ((size_t)rows * (rt + 1) + 2 + 2 * 64) * sizeof(float); }      // + the tile's sample indices (64-bit)

// backward-data of one layer, in place: y (the stored output of the layer below, [K][LD]) becomes its delta.  RAW (kernels_ln.hpp): W^T delta alone
// into y, no activation derivative -- what a layer norm between the two layers receives
template <int LD, bool RAW = false>
__device__ __forceinline__ void ppo_dx(const float* __restrict__ W, int K, int Nout, const float* dY, float* y, int row, int wave, int relu) {
  for (int k0 = wave * ACT_NB; k0 < K; k0 += ACT_WAVES * ACT_NB) {
    int kk[ACT_NB];
    float acc[ACT_NB];
#pragma unroll
    for (int j = 0; j < ACT_NB; j++) {
      kk[j] = min(k0 + j, K - 1);      // a short last block recomputes the last neuron and does not store it
      acc[j] = 0.0f;
    }
    int o = 0;
    for (; o + 4 <= Nout; o += 4) {
      float d[4], w[4][ACT_NB];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        d[q] = dY[(o + q) * LD + row];
#pragma unroll
        for (int j = 0; j < ACT_NB; j++) w[q][j] = W[(size_t)(o + q) * K + kk[j]];
      }
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int j = 0; j < ACT_NB; j++) acc[j] = fmaf(w[q][j], d[q], acc[j]);
    }
    for (; o < Nout; o++) {
      const float d = dY[o * LD + row];
#pragma unroll
      for (int j = 0; j < ACT_NB; j++) acc[j] = fmaf(W[(size_t)o * K + kk[j]], d, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < ACT_NB; j++) {
      if (k0 + j < K) {
        if (RAW) { y[(k0 + j) * LD + row] = acc[j]; continue; }
        const float yv = y[(k0 + j) * LD + row];
        y[(k0 + j) * LD + row] = relu ? (yv > 0.0f ? acc[j] : 0.0f) : acc[j] * fmaf(-yv, yv, 1.0f);
      }
    }
  }
}

// weight and bias gradient of one layer: the workgroup's partial (gW [Nout][K], gB [Nout]) continues its per-element fmaf chain over the RT rows
template <int LD, int RT>
__device__ __forceinline__ void ppo_dw(const float* dY, const float* x, int K, int Nout, float* __restrict__ gW, float* __restrict__ gB, bool first,
                                       int tid) {
  const int nbk = (K + 3) >> 2, nbo = (Nout + 3) >> 2;
  for (int blk = tid; blk < nbk * nbo; blk += ACT_THREADS) {
    const int ob = blk / nbk, kb = blk - ob * nbk;
    int oo[4], kk[4];
    bool ov[4], kv[4];
    float acc[4][4], accb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      ov[j] = ob * 4 + j < Nout; oo[j] = ov[j] ? ob * 4 + j : Nout - 1;
      kv[j] = kb + j * nbk < K;  kk[j] = kv[j] ? kb + j * nbk : K - 1;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      accb[j] = (!first && ov[j] && kb == 0) ? gB[oo[j]] : 0.0f;
#pragma unroll
      for (int q = 0; q < 4; q++) acc[j][q] = (!first && ov[j] && kv[q]) ? gW[(size_t)oo[j] * K + kk[q]] : 0.0f;
    }
#pragma unroll 4
    for (int r = 0; r < RT; r++) {
      float dy[4], xv[4];
#pragma unroll
      for (int j = 0; j < 4; j++) { dy[j] = dY[oo[j] * LD + r]; xv[j] = x[kk[j] * LD + r]; }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        accb[j] += dy[j];
#pragma unroll
        for (int q = 0; q < 4; q++) acc[j][q] = fmaf(dy[j], xv[q], acc[j][q]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (ov[j] && kb == 0) gB[oo[j]] = accb[j];
#pragma unroll
      for (int q = 0; q < 4; q++)
        if (ov[j] && kv[q]) gW[(size_t)oo[j] * K + kk[q]] = acc[j][q];
    }
  }
}

// inv_g, inv_a, group: THE JOINT RATIO above (without the flag inv_g = inv_m, group = 1); dual, dual_clip: THE DUAL CLIP
struct PpoLoss { float clip, value_coef, entropy_coef, value_clip, inv_m; int clip_value; float inv_g, inv_a, dual_clip; int group, dual; };
struct PpoTraj {                       // the trajectory and the minibatch of it (THE LOSS above)
  const float* packed; long long stride; int rows; long long n_total;
  const float *actions, *logp_old, *value, *adv, *ret;
  const int32_t* index; long long first, count;
};
struct PpoSums { double Lpi = 0.0, Lv = 0.0, Kl = 0.0, Clip = 0.0, gls[3] = {0.0, 0.0, 0.0}; };      // f64 per lane of wavefront 0 over the workgroup's tiles

// the samples of tile `tile` (past the end of the minibatch the last one again) and their observations -> LDS [k][row]
template <int LD, int RT>
__device__ __forceinline__ void ppo_load_tile(float* lds, long long* srow, const float* __restrict__ packed, long long stride, int rows, long long n_total,
                                              const int32_t* __restrict__ index, long long first, long long count, long long tile, int D, int tid) {
  if (tid < RT) {
    long long i = tile * RT + tid;
    if (i > count - 1) i = count - 1;
    srow[tid] = ppo_unit(index, first, i, n_total);
  }
  __syncthreads();
  for (int e = tid; e < RT * D; e += ACT_THREADS) {
    const int r = e / D, k = e - r * D;
    const long long s = srow[r];
    const long long t = s / rows, rr = s - t * rows;
    lds[k * LD + r] = packed[(size_t)t * (size_t)stride + (size_t)rr * D + k];
  }
  __syncthreads();
}

// wavefront 0, behind the actor's forward: out[0 .. 2] (the mean) becomes the delta of the last layer; the policy statistics
template <int LD, int RT>
__device__ __forceinline__ void ppo_actor_head(const float* __restrict__ params, int log_std_off, float* out, const long long* srow, int row, int lane, bool valid,
                                               const float* __restrict__ actions, const float* __restrict__ logp_old, const float* __restrict__ adv,
                                               const PpoLoss& ls, PpoSums& S) {
  const long long s = srow[row];
  const float lpo = logp_old[s];
  float z[3], inv[3], lp = 0.0f;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float lsj = params[log_std_off + j];
    inv[j] = expf(-lsj);
    z[j] = (actions[(size_t)s * 3 + j] - out[j * LD + row]) * inv[j];
    lp += -0.5f * z[j] * z[j] - lsj;
  }
  lp -= 3.0f * 0.9189385332046727f;       // 3 x 0.5 ln(2 pi)
  // the joint ratio: the group's log-ratio and advantage over the xor butterfly 1, 2, ...: a + b is b + a, so every lane of a group holds the same bits
  // (all 64 lanes are here; a group is `group` aligned lanes of one tile, wholly valid or wholly padding; at 32-row tiles the upper half mirrors the lower)
  float d = lp - lpo, ad = adv[s];
  if (ls.group > 1) {
    for (int m = 1; m < ls.group; m <<= 1) {
      d += __shfl_xor(d, m);
      ad += __shfl_xor(ad, m);
    }
    ad *= ls.inv_a;
  }
  const float ratio = expf(d);
  const float lo = 1.0f - ls.clip, hi = 1.0f + ls.clip;
  float Lpi = -fminf(ratio * ad, fminf(fmaxf(ratio, lo), hi) * ad);
  bool gate = (ad > 0.0f && ratio > hi) || (ad < 0.0f && ratio < lo);
  if (ls.dual) {                       // the second bound, where the advantage is negative
    const float bound = -(ls.dual_clip * ad);
    Lpi = ad < 0.0f ? fminf(Lpi, bound) : Lpi;
    gate = gate || (ad < 0.0f && ratio > ls.dual_clip);
  }
  const float dlp = gate ? 0.0f : -ad * ratio * ls.inv_g;
  if (lane < RT) {
#pragma unroll
    for (int j = 0; j < 3; j++) out[j * LD + row] = valid ? dlp * z[j] * inv[j] : 0.0f;
  }
  if (valid) {
    S.Lpi += (double)Lpi;
    S.Kl += (double)(-d);              // lpo - lp of the sample; of the group under the joint ratio
    S.Clip += fabsf(ratio - 1.0f) > ls.clip ? 1.0 : 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) S.gls[j] += (double)(dlp * (z[j] * z[j] - 1.0f));
  }
}

// wavefront 0, behind the critic's forward: out[3] (the value) becomes the delta of the last layer; the value statistic
template <int LD, int RT>
__device__ __forceinline__ void ppo_critic_head(float* out, const long long* srow, int row, int lane, bool valid, const float* __restrict__ value,
                                                const float* __restrict__ ret, const PpoLoss& ls, PpoSums& S) {
  const long long s = srow[row];
  const float v = out[3 * LD + row], rt = ret[s];
  const float d1 = v - rt, u = d1 * d1;
  float Lv = u, dv = 2.0f * d1;
  if (ls.clip_value) {
    const float vo = value[s];
    const float dvo = v - vo;
    const float vc = vo + fminf(fmaxf(dvo, -ls.value_clip), ls.value_clip);
    const float d2 = vc - rt, cl = d2 * d2;
    Lv = fmaxf(u, cl);
    dv = u >= cl ? 2.0f * d1 : (fabsf(dvo) < ls.value_clip ? 2.0f * d2 : 0.0f);
  }
  if (lane < RT) out[3 * LD + row] = valid ? ls.value_coef * ls.inv_m * dv : 0.0f;
  if (valid) S.Lv += (double)Lv;
}

// wavefront 0, at the end: the seven sums across the lanes (xor butterfly 32, 16, ..., 1) -> the workgroup's statistics slot
__device__ __forceinline__ void ppo_store_sums(const PpoSums& S, int lane, double* __restrict__ pst) {
  double v[7] = {S.Lpi, S.Lv, S.Kl, S.Clip, S.gls[0], S.gls[1], S.gls[2]};
#pragma unroll
  for (int q = 0; q < 7; q++) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v[q] += __shfl_xor(v[q], m);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 7; q++) pst[q] = v[q];
  }
}

// grad and the statistics from the G workgroups' partials, in workgroup order
__global__ void __launch_bounds__(PPO_REDUCE_THREADS) k_ppo_reduce(const float* __restrict__ part, const double* __restrict__ pst, int G, int n_params,
                                                                   int log_std_off, long long M, float value_coef, float entropy_coef,
                                                                   const float* __restrict__ params, float* __restrict__ grad, float* __restrict__ stats) {
  const int i = blockIdx.x * PPO_REDUCE_THREADS + threadIdx.x;
  if (i < log_std_off) {
    double a = 0.0;
    for (int b = 0; b < G; b++) a += (double)part[(size_t)b * n_params + i];
    grad[i] = (float)a;
  } else if (i < n_params) {
    double a = 0.0;
    for (int b = 0; b < G; b++) a += pst[(size_t)b * PPO_PST + 4 + (i - log_std_off)];
    grad[i] = (float)(a - (double)entropy_coef);
  }
  if (i == 0 && stats != nullptr) {
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < G; b++)
      for (int q = 0; q < 4; q++) S[q] += pst[(size_t)b * PPO_PST + q];
    const double n = (double)M;
    double H = 1.5 * (1.0 + 1.8378770664093453);        // ln(2 pi)
    for (int j = 0; j < 3; j++) H += (double)params[log_std_off + j];
    const double Lpi = S[0] / n, Lv = S[1] / n;
    stats[0] = (float)Lpi;
    stats[1] = (float)Lv;
    stats[2] = (float)H;
    stats[3] = (float)(Lpi + (double)value_coef * Lv - (double)entropy_coef * H);
    stats[4] = (float)(S[2] / n);
    stats[5] = (float)(S[3] / n);
  }
}

// the L2 norm of the gradient in f64, a fixed order: one workgroup
__global__ void __launch_bounds__(PPO_NORM_THREADS) k_ppo_norm(const float* __restrict__ grad, int n, double* __restrict__ norm_out, float* __restrict__ norm_dev) {
  __shared__ double red[PPO_NORM_THREADS];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += PPO_NORM_THREADS) a = fma((double)grad[i], (double)grad[i], a);
  red[threadIdx.x] = a;
  __syncthreads();
  for (int w = PPO_NORM_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double nn = sqrt(red[0]);
    norm_out[0] = nn;
    if (norm_dev != nullptr) norm_dev[0] = (float)nn;
  }
}

struct PpoAdam { float b1, b2, omb1, omb2, step_size, bc2s, eps, max_norm; };

__global__ void __launch_bounds__(PPO_ADAM_THREADS) k_ppo_adam(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ grad,
                                                               int n, const double* __restrict__ norm, PpoAdam a) {
  const int i = blockIdx.x * PPO_ADAM_THREADS + threadIdx.x;
  if (i >= n) return;
  float scale = 1.0f;
  if (a.max_norm > 0.0f) scale = fminf(1.0f, a.max_norm / ((float)norm[0] + 1e-6f));
  const float g = grad[i] * scale;
  const float mi = fmaf(a.b1, m[i], a.omb1 * g);
  const float vi = fmaf(a.b2, v[i], (a.omb2 * g) * g);
  m[i] = mi;
  v[i] = vi;
  p[i] = p[i] - (a.step_size * mi) / (sqrtf(vi) / a.bc2s + a.eps);
}
