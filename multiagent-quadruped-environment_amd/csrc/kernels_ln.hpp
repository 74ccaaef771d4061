// kernels_ln.hpp -- k_actor_ln / k_ln_grad: layer normalisation in the engine's actor-critic, forward and backward (MQE_ACTOR_LAYER_NORM,
// MQE_ACTOR_FEATURE_NORM; include/mqe_hip.h).  Siblings of k_actor (kernels_actor.hpp) and k_ppo_grad (kernels_ppo.hpp), built from their device
// functions (actor_layer, actor_load_obs, actor_finish; ppo_load_tile, ppo_actor_head, ppo_critic_head, ppo_dw, ppo_dx, ppo_store_sums): a handle
// created without the two bits never launches a kernel of this file, and one created with either launches these two INSTEAD of the plain pair.
// k_ppo_reduce, k_ppo_norm and k_ppo_adam are shared: gamma and beta are ordinary entries of the flat parameter buffer.
//
// THE OPERATOR is torch.nn.LayerNorm(n, eps = 1e-5, elementwise_affine = True) on the n features of one row: u = gamma * xhat + beta,
// xhat = (a - mu) * rstd, mu = mean(a), rstd = 1 / sqrt(mean((a - mu)^2) + eps)   (biased variance).  Two switches, for both networks of a handle:
//   hidden norm   behind the activation of EVERY hidden layer (never behind the output layer): a = tanh / relu (W x + b), u is the next layer's input
//   feature norm  on the D observation floats in front of layer 0; each network has its own gamma and beta
// PARAMETERS, per network:  [norm_in.weight (D), norm_in.bias (D)]  then per layer l:  weight, bias, [norm.weight (n), norm.bias (n)] (hidden l only).
// So gamma of the norm behind layer l starts at w_off[l] + K n + n, and the feature norm's at w_off[0] - 2 D: no offsets beyond ActorNet's.
//
// ARITHMETIC (all f32; tests/layer_norm_ref.py restates it).  The n features of a row are split over the 16 wavefronts in consecutive chunks of
// c = ceil(n / 16):  wavefront w owns k = w c .. min(n, w c + c) - 1 (possibly none).  With 1 / n = (float)(1.0 / n) formed on the host:
//     s_w = 0;  for k ascending in the chunk:  s_w = s_w + a[k]                 mu   = (((0 + s_0) + s_1) + ... + s_15) * (1 / n)
//     q_w = 0;  for k ascending:  d = a[k] - mu;  q_w = fmaf(d, d, q_w)          var  = (((0 + q_0) + q_1) + ... + q_15) * (1 / n)
//     rstd = 1 / sqrtf(var + 1e-5f)                                              u[k] = fmaf(gamma[k], (a[k] - mu) * rstd, beta[k])
// two-pass and centred: E[a^2] - mu^2 would cancel.  The order is a function of n and ACT_WAVES alone.
// WHY SPLIT OVER THE WAVEFRONTS.  A serial sweep by one wavefront leaves 15 idle and is two passes of up to 256 dependent LDS reads; split, a pass is
// at most 16 reads per wavefront, plus 16 reads of the per-wave partials ([w][row] in LDS, added in wave order by every wavefront, so all hold the
// same mu and rstd without a broadcast).  Three barriers per norm.  Lane = row as everywhere: gamma[k] and beta[k] are wave-uniform scalar loads.
//
// BACKWARD, per row and normalised layer, du the gradient with respect to u (W^T delta of the layer above, ppo_dx without an activation derivative):
//     dgamma[k] = sum over the rows of du * xhat;   dbeta[k] = sum over the rows of du        (per tile by the xor butterfly RT / 2, ..., 1 across the
//         lanes of the wavefront that owns k -- lane = row --, then added to the workgroup's partial gradient, which continues over its tiles;
//         k_ppo_reduce adds the workgroups, exactly like a bias)
//     dxhat = du * gamma;   m1 = mean(dxhat),  m2 = mean(dxhat * xhat)          (per-wave partials fmaf(du, gamma, .) and fmaf(dxhat, xhat, .), wave order, * (1 / n))
//     da = rstd * fmaf(-xhat, m2, dxhat - m1);    delta = da * (1 - a^2)  (tanh)  or  (a > 0 ? da : 0)  (relu)
// No atomics: the same bits on every run.  The feature norm has no da (nothing lies below the observation): only dgamma and dbeta.
//
// LDS OF k_ln_grad (the delta scheme of DESIGN 3.5, extended).  What is STORED per normalised layer is the activation a (where the plain kernel
// stores the layer's output) and two rows (mu, rstd); xhat and u are RECOMPUTED from them with the forward's own expression, so they are the
// forward's bits.  u lives in one shared buffer U as wide as the widest normalised vector: the forward writes u there for the next layer to
// read; the backward fills it again before each weight gradient (the last reader of u as an input), then ppo_dx writes du over it, then the norm's
// backward turns the stored a into delta in place.  Rows of the image:
//     D + (hidden widths of the larger network) + Uw + 8 (mu, rstd of at most 4 norms) + 32 (per-wave partials) + 4 (mean 0 .. 2, value)
//     Uw = max(D if feature norm, the widest hidden layer of either network if hidden norm)
// RT = 64 (stride 65) when that fits 160 KiB, else 32 (stride 33): it takes 32-row tiles earlier than the plain rule (two 128 x 128 x 128 networks at
// D = 16: 572 rows -> 145 KiB at 64; at D = 128 with both switches: 684 rows -> 32-row tiles).  The widest accepted shape, D = 128 and 3 x 256 with
// both switches, is 1196 rows = 154.7 KiB at 32 rows.  k_actor_ln: the two ping-pong buffers, normalised in place, + the 32 partial rows.
#pragma once
#include "mqe_common.hpp"
#include "kernels_actor.hpp"
#include "kernels_ppo.hpp"

// the constants of the layer-normalisation section of include/mqe_hip.h: stated there in words, defined here (the header's ACTOR define set is
// pinned by the tests), mirrored in mqe/engine/abi.py; tests/test_layer_norm.py compares the three.  Bits of the kind byte of activation.
#define MQE_ACTOR_LAYER_NORM 2            // a LayerNorm behind the activation of every hidden layer
#define MQE_ACTOR_FEATURE_NORM 4          // a LayerNorm on the observation in front of layer 0

#define LN_EPS 1e-5f
#define LN_PART (2 * ACT_WAVES)                      // LDS rows of per-wave partials: two sums at a time
#define LN_STAT (2 * MQE_ACTOR_MAX_LAYERS)           // LDS rows of (mu, rstd): norm j at rows 2 j, 2 j + 1; j = 0 the feature norm, j = l the norm in front of layer l

struct LnNet { ActorNet net; float inv_n[MQE_ACTOR_MAX_LAYERS]; };      // inv_n[l] = (float)(1.0 / dims[l]): the width of layer l's INPUT
struct LnNets { LnNet actor, critic; int hidden, feat; };
struct ActorLnArgs { ActorArgs a; float inv_actor[MQE_ACTOR_MAX_LAYERS], inv_critic[MQE_ACTOR_MAX_LAYERS]; int hidden, feat; };

static inline size_t actor_ln_lds_bytes(int ldh) { return (size_t)(2 * ldh + 4 + LN_PART) * ACT_LD * sizeof(float); }
static inline int ln_lds_rows(const ActorNet& a, const ActorNet& c, int D, bool hidden, bool feat) {
  int uw = feat ? D : 0;
  if (hidden) {
    for (int l = 1; l < a.n_layers; l++) uw = a.dims[l] > uw ? a.dims[l] : uw;
    for (int l = 1; l < c.n_layers; l++) uw = c.dims[l] > uw ? c.dims[l] : uw;
  }
  return ppo_lds_rows(a, c, D) + uw + LN_STAT + LN_PART;
}
// gamma of the norm in front of layer l (beta follows it, dims[l] floats on)
__host__ __device__ inline int ln_gamma_off(const ActorNet& net, int l) {
  return l == 0 ? net.w_off[0] - 2 * net.dims[0] : net.w_off[l - 1] + net.dims[l - 1] * net.dims[l] + net.dims[l];
}

// the norm of the n features of the workgroup's rows: a ([n][LD]) -> u (may be a itself); stat (or null) receives mu and rstd.  Ends in a barrier.
template <int LD>
__device__ __forceinline__ void ln_rows(const float* a, float* u, int n, const float* __restrict__ g, const float* __restrict__ b, float inv_n, float* part,
                                        float* stat, int row, int wave) {
  const int c = (n + ACT_WAVES - 1) / ACT_WAVES;
  const int k0 = min(wave * c, n), k1 = min(k0 + c, n);
  float s = 0.0f;
  for (int k = k0; k < k1; k++) s = s + a[k * LD + row];
  part[wave * LD + row] = s;
  __syncthreads();
  float t = 0.0f;
#pragma unroll
  for (int w = 0; w < ACT_WAVES; w++) t = t + part[w * LD + row];
  const float mu = t * inv_n;
  float q = 0.0f;
  for (int k = k0; k < k1; k++) {
    const float d = a[k * LD + row] - mu;
    q = fmaf(d, d, q);
  }
  part[(ACT_WAVES + wave) * LD + row] = q;
  __syncthreads();
  t = 0.0f;
#pragma unroll
  for (int w = 0; w < ACT_WAVES; w++) t = t + part[(ACT_WAVES + w) * LD + row];
  const float rstd = 1.0f / sqrtf(t * inv_n + LN_EPS);
  for (int k = k0; k < k1; k++) u[k * LD + row] = fmaf(g[k], (a[k * LD + row] - mu) * rstd, b[k]);
  if (stat != nullptr && wave == 0) {
    stat[row] = mu;
    stat[LD + row] = rstd;
  }
  __syncthreads();
}

// u again from the stored a, mu and rstd: the last statement of ln_rows, so the forward's bits.  No barrier.
template <int LD>
__device__ __forceinline__ void ln_again(const float* a, float* u, int n, const float* __restrict__ g, const float* __restrict__ b, const float* stat, int row,
                                         int wave) {
  const int c = (n + ACT_WAVES - 1) / ACT_WAVES;
  const int k0 = min(wave * c, n), k1 = min(k0 + c, n);
  const float mu = stat[row], rstd = stat[LD + row];
  for (int k = k0; k < k1; k++) u[k * LD + row] = fmaf(g[k], (a[k * LD + row] - mu) * rstd, b[k]);
}

// backward of one norm: du ([n][LD]) and the stored a, mu, rstd -> the workgroup's partial dgamma / dbeta (gG, gB) and, with DX, delta over a in place.
// dgamma / dbeta of feature k: the tile's sum over the rows (= lanes) of du * xhat / du by the xor butterfly RT / 2, ..., 1 (k_gae's), in the wavefront
// that owns k; lane j keeps the sums of the chunk's feature j and adds them to the running partial with one load and one store
template <int LD, int RT, bool DX>
__device__ __forceinline__ void ln_back(float* a, const float* du, int n, const float* __restrict__ g, float inv_n, const float* stat, float* part,
                                        float* __restrict__ gG, float* __restrict__ gB, bool first, int relu, int row, int lane, int wave) {
  const int c = (n + ACT_WAVES - 1) / ACT_WAVES;
  const int k0 = min(wave * c, n), k1 = min(k0 + c, n);
  const float mu = stat[row], rstd = stat[LD + row];
  float s1 = 0.0f, s2 = 0.0f, mg = 0.0f, mb = 0.0f;
  for (int k = k0; k < k1; k++) {
    const float d = du[k * LD + row];
    const float xh = (a[k * LD + row] - mu) * rstd;
    if (DX) {
      const float gk = g[k];
      s1 = fmaf(d, gk, s1);
      s2 = fmaf(d * gk, xh, s2);
    }
    float pg = d * xh, pb = d;
#pragma unroll
    for (int m = RT / 2; m >= 1; m >>= 1) {
      pg += __shfl_xor(pg, m);
      pb += __shfl_xor(pb, m);
    }
    if (lane == k - k0) { mg = pg; mb = pb; }
  }
  if (DX) {
    part[wave * LD + row] = s1;
    part[(ACT_WAVES + wave) * LD + row] = s2;
  }
  if (lane < k1 - k0) {                 // c <= 16 lanes
    gG[k0 + lane] = (first ? 0.0f : gG[k0 + lane]) + mg;
    gB[k0 + lane] = (first ? 0.0f : gB[k0 + lane]) + mb;
  }
  __syncthreads();
  if (!DX) return;
  float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
  for (int w = 0; w < ACT_WAVES; w++) {
    m1 = m1 + part[w * LD + row];
    m2 = m2 + part[(ACT_WAVES + w) * LD + row];
  }
  m1 *= inv_n;
  m2 *= inv_n;
  for (int k = k0; k < k1; k++) {
    const float av = a[k * LD + row];
    const float xh = (av - mu) * rstd;
    const float da = rstd * fmaf(-xh, m2, du[k * LD + row] * g[k] - m1);
    a[k * LD + row] = relu ? (av > 0.0f ? da : 0.0f) : da * fmaf(-av, av, 1.0f);
  }
  __syncthreads();
}

// ---- k_actor_ln: k_actor with the norms; the two ping-pong buffers are normalised in place -----------------------------------------------------
__device__ __forceinline__ void ln_actor_net(const ActorNet& net, const float* inv_n, int hidden, int feat, const float* __restrict__ params, float* bufA,
                                             float* bufB, float* out, float* part, int lane, int wave, int hidden_act) {
  if (feat) {
    const float* g = params + ln_gamma_off(net, 0);
    ln_rows<ACT_LD>(bufB, bufB, net.dims[0], g, g + net.dims[0], inv_n[0], part, nullptr, lane, wave);
  }
  const float* x = bufB;
  float* y = bufA;
  for (int l = 0; l < net.n_layers; l++) {
    const bool last = l + 1 == net.n_layers;
    const int K = net.dims[l], Nout = net.dims[l + 1];
    const float* W = params + net.w_off[l];
    const float* b = W + (size_t)K * Nout;
    float* dst = last ? out : y;
    if (((K | net.w_off[l]) & 3) == 0) actor_layer<true>(W, b, K, Nout, x, dst, lane, wave, last ? 0 : hidden_act);
    else actor_layer<false>(W, b, K, Nout, x, dst, lane, wave, last ? 0 : hidden_act);
    __syncthreads();
    if (!last && hidden) ln_rows<ACT_LD>(y, y, Nout, b + Nout, b + 2 * Nout, inv_n[l + 1], part, nullptr, lane, wave);
    float* t = const_cast<float*>(x); x = y; y = t;
  }
}

__global__ void __launch_bounds__(ACT_THREADS) k_actor_ln(ActorLnArgs k) {
  extern __shared__ __attribute__((aligned(16))) float act_ln_lds[];
  const ActorArgs& a = k.a;
  float* bufA = act_ln_lds;
  float* bufB = act_ln_lds + (size_t)a.ldh * ACT_LD;
  float* out = act_ln_lds + (size_t)2 * a.ldh * ACT_LD;       // [4][ACT_LD]: mean 0..2, value
  float* part = out + 4 * ACT_LD;                             // [LN_PART][ACT_LD]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * ACT_ROWS;
  const int hidden_act = a.relu ? 2 : 1;
  const bool sample = a.actions != nullptr;
  if (sample) {
    actor_load_obs(a.obs, row0, a.rows, a.D, bufB, tid);
    __syncthreads();
    ln_actor_net(a.actor, k.inv_actor, k.hidden, k.feat, a.params, bufA, bufB, out, part, lane, wave, hidden_act);
  }
  const bool critic = a.critic.n_layers > 0 && a.value != nullptr;
  if (critic) {
    actor_load_obs(a.obs, row0, a.rows, a.D, bufB, tid);
    __syncthreads();
    ln_actor_net(a.critic, k.inv_critic, k.hidden, k.feat, a.params, bufA, bufB, out + 3 * ACT_LD, part, lane, wave, hidden_act);
  }
  if (wave != 0) return;
  actor_finish(a, out, sample, critic, row0, lane);
}

// ---- k_ln_grad: k_ppo_grad with the norms ---------------------------------------------------------------------------------------------------------
// forward of one network, every activation kept: observation at lds[0], the activation of hidden layer l behind it as in ppo_forward, u in U
template <int LD>
__device__ __forceinline__ void ln_forward(const LnNet& ln, int hidden, int feat, const float* __restrict__ params, float* lds, int D, float* U, float* stat,
                                           float* part, float* out, int row, int wave, int hidden_act) {
  const ActorNet& net = ln.net;
  const float* x = lds;
  if (feat) {
    const float* g = params + ln_gamma_off(net, 0);
    ln_rows<LD>(lds, U, D, g, g + D, ln.inv_n[0], part, stat, row, wave);
    x = U;
  }
  float* y = lds + (size_t)D * LD;
  for (int l = 0; l < net.n_layers; l++) {
    const bool last = l + 1 == net.n_layers;
    const int K = net.dims[l], Nout = net.dims[l + 1];
    const float* W = params + net.w_off[l];
    const float* b = W + (size_t)K * Nout;
    float* dst = last ? out : y;
    if (((K | net.w_off[l]) & 3) == 0) actor_layer<true, LD>(W, b, K, Nout, x, dst, row, wave, last ? 0 : hidden_act);
    else actor_layer<false, LD>(W, b, K, Nout, x, dst, row, wave, last ? 0 : hidden_act);
    __syncthreads();
    if (last) break;
    x = y;
    if (hidden) {
      ln_rows<LD>(y, U, Nout, b + Nout, b + 2 * Nout, ln.inv_n[l + 1], part, stat + (size_t)2 * (l + 1) * LD, row, wave);
      x = U;
    }
    y += (size_t)Nout * LD;
  }
}

// backward of one network: `out` holds the delta of the last layer; per layer, top down: u of its input into U again, the weight gradient, du over U,
// the norm's backward (delta over the stored activation in place).  A layer whose input is not normalised goes the plain way (ppo_dx in place).
template <int LD, int RT>
__device__ __forceinline__ void ln_backward(const LnNet& ln, int hidden, int feat, const float* __restrict__ params, float* __restrict__ pg, float* lds, int D,
                                            float* U, float* stat, float* part, float* out, int row, int wave, int tid, int relu, bool first) {
  const ActorNet& net = ln.net;
  int below = 0;
  for (int l = 1; l + 1 < net.n_layers; l++) below += net.dims[l];
  float* dY = out;
  for (int l = net.n_layers - 1; l >= 0; l--) {
    const int K = net.dims[l], Nout = net.dims[l + 1];
    float* a = l == 0 ? lds : lds + (size_t)(D + below) * LD;      // the stored input of layer l: the observation, or the activation below
    const bool normed = l == 0 ? feat != 0 : hidden != 0;
    const int go = normed ? ln_gamma_off(net, l) : 0;
    const float* st = stat + (size_t)2 * l * LD;
    const float* x = a;
    if (normed) {
      ln_again<LD>(a, U, K, params + go, params + go + K, st, row, wave);
      __syncthreads();
      x = U;
    }
    ppo_dw<LD, RT>(dY, x, K, Nout, pg + net.w_off[l], pg + net.w_off[l] + (size_t)K * Nout, first, tid);
    __syncthreads();
    if (l == 0 && !normed) break;
    if (!normed) {
      ppo_dx<LD>(params + net.w_off[l], K, Nout, dY, a, row, wave, relu);
      __syncthreads();
    } else {
      ppo_dx<LD, true>(params + net.w_off[l], K, Nout, dY, U, row, wave, relu);
      __syncthreads();
      if (l == 0) {
        ln_back<LD, RT, false>(a, U, K, params + go, ln.inv_n[0], st, part, pg + go, pg + go + K, first, relu, row, tid & 63, wave);
        break;
      }
      ln_back<LD, RT, true>(a, U, K, params + go, ln.inv_n[l], st, part, pg + go, pg + go + K, first, relu, row, tid & 63, wave);
    }
    dY = a;
    if (l >= 2) below -= net.dims[l - 1];
  }
}

struct PpoTraj {
  const float* packed; long long stride; int rows; long long n_total;
  const float *actions, *logp_old, *value, *adv, *ret;
  const int32_t* index; long long first, count;
};

template <int RT>
__global__ void __launch_bounds__(ACT_THREADS) k_ln_grad(const float* __restrict__ params, const LnNets* __restrict__ nets, int log_std_off, int n_params, int D,
                                                         int rows_lds, int uw, int relu, PpoTraj tr, PpoLoss ls, float* __restrict__ part_all,
                                                         double* __restrict__ pst) {
  constexpr int LD = RT + 1;
  extern __shared__ __attribute__((aligned(16))) float ln_lds[];
  float* out = ln_lds + (size_t)(rows_lds - 4) * LD;
  float* part = out - (size_t)LN_PART * LD;
  float* stat = part - (size_t)LN_STAT * LD;
  float* U = stat - (size_t)uw * LD;
  long long* srow = reinterpret_cast<long long*>(ln_lds + (size_t)rows_lds * LD + (((size_t)rows_lds * LD) & 1));      // 8-byte aligned
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row = lane & (RT - 1);
  const int hidden_act = relu ? 2 : 1;
  const int hidden = nets->hidden, feat = nets->feat;
  float* pg = part_all + (size_t)blockIdx.x * n_params;
  const long long tiles = (tr.count + RT - 1) / RT;
  PpoSums S;
  bool first_tile = true;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    ppo_load_tile<LD, RT>(ln_lds, srow, tr.packed, tr.stride, tr.rows, tr.n_total, tr.index, tr.first, tr.count, tile, D, tid);
    const bool valid = tile * RT + lane < tr.count && lane < RT;
    ln_forward<LD>(nets->actor, hidden, feat, params, ln_lds, D, U, stat, part, out, row, wave, hidden_act);
    if (wave == 0) ppo_actor_head<LD, RT>(params, log_std_off, out, srow, row, lane, valid, tr.actions, tr.logp_old, tr.adv, ls, S);
    __syncthreads();
    ln_backward<LD, RT>(nets->actor, hidden, feat, params, pg, ln_lds, D, U, stat, part, out, row, wave, tid, relu, first_tile);
    ln_forward<LD>(nets->critic, hidden, feat, params, ln_lds, D, U, stat, part, out + 3 * LD, row, wave, hidden_act);
    if (wave == 0) ppo_critic_head<LD, RT>(out, srow, row, lane, valid, tr.value, tr.ret, ls, S);
    __syncthreads();
    ln_backward<LD, RT>(nets->critic, hidden, feat, params, pg, ln_lds, D, U, stat, part, out + 3 * LD, row, wave, tid, relu, first_tile);
    first_tile = false;
  }
  if (wave != 0) return;
  ppo_store_sums(S, lane, pst + (size_t)blockIdx.x * PPO_PST);
}
