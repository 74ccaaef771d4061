// kernels_ln.hpp -- layer normalisation in the engine's actor-critic (MQE_ACTOR_LAYER_NORM, MQE_ACTOR_FEATURE_NORM; include/mqe_hip.h): the norm
// itself, forward (ln_rows), again from its stored statistics (ln_again) and backward (ln_back), its constants and its two LDS rules.  The walks of
// kernels_actor_critic.hpp switch it in at compile time (LN): k_actor_ln and k_ln_grad are the instantiations with it, k_actor and k_ppo_grad those
// without.  A handle created without the two bits never launches the first pair, and one created with either launches it INSTEAD of the plain pair.
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
// DX: 0 the gamma / beta gradients alone (the feature norm), 1 delta = da times the activation derivative of a, 2 da alone (the norm behind the GRU cell:
// its input is the cell's h', no activation; kernels_bptt.hpp).  dgamma / dbeta of feature k: the tile's sum over the rows (= lanes) of du * xhat / du by the xor butterfly RT / 2, ..., 1 (k_gae's), in the wavefront
// that owns k; lane j keeps the sums of the chunk's feature j and adds them to the running partial with one load and one store
template <int LD, int RT, int DX>
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
    a[k * LD + row] = DX == 2 ? da : relu ? (av > 0.0f ? da : 0.0f) : da * fmaf(-av, av, 1.0f);
  }
  __syncthreads();
}
