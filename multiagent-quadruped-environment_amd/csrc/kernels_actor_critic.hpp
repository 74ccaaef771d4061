// kernels_actor_critic.hpp -- the network walks of the engine's actor-critic and the entry points built on them: k_actor / k_actor_ln and, with a
// GRU cell in front of the output layer (kernels_gru.hpp; the compile-time parameter GRU), k_actor_gru / k_actor_gru_ln (the rollout's actor,
// mqe_rollout) and k_ppo_grad<RT> / k_ln_grad<RT> (the PPO gradient, mqe_ppo_grad).  Each walk is stated once, with the layer norm a
// compile-time parameter LN: the LN = false instantiation contains no norm code and reads neither the switches nor the 1 / n arrays.  The primitives
// are in kernels_actor.hpp (one layer, the observation load, the draw) and kernels_ppo.hpp (the tile load, the loss heads, ppo_dw, ppo_dx); the norm
// is in kernels_ln.hpp.  The entry points do nothing but call the body: their names are what a kernel trace shows of the path that ran.
//
// THE ROLLOUT'S WALK (actor_net).  Two activation buffers ping-pong (observation in B -> A -> B -> A); the critic re-reads the observation (4 kB per
// workgroup, L2-hot) instead of holding a third buffer.  LN: the feature norm normalises B in place in front of layer 0, the hidden norm every hidden
// output in place behind its barrier, through the LN_PART partial rows behind the four output rows.
//
// THE GRADIENT'S WALK (ppo_forward, ppo_backward, ppo_grad_body).  A workgroup walks row tiles of RT samples: tile i of the minibatch is samples
// i RT .. i RT + RT - 1; workgroup b of G = min(tiles, PPO_MAX_WG) takes tiles b, b + G, b + 2 G, ... in that order (a fixed grid: a function
// of count, the tile height and PPO_MAX_WG alone).  The two networks run one after the other (actor forward, actor head, actor backward,
// critic forward on the observation that is still there, critic head, critic backward); every layer output is kept for the backward pass, which
// turns it into its delta in place (kernels_ppo.hpp, LAYOUT).  LN: what is kept of a normalised layer is its activation a and (mu, rstd); the
// normalised u goes to the shared buffer U, which the backward fills again before each weight gradient (kernels_ln.hpp, LDS OF k_ln_grad).
#pragma once
#include "mqe_common.hpp"
#include "kernels_actor.hpp"
#include "kernels_ppo.hpp"
#include "kernels_ln.hpp"
#include "kernels_gru.hpp"

// ---- k_actor / k_actor_ln / k_actor_gru / k_actor_gru_ln ---------------------------------------------------------------------------------------------
// a whole network: observation in bufB; result (last layer, linear) -> out[j * ACT_LD + row].  LN: the two buffers are normalised in place.
// GRU (kernels_gru.hpp): the cell sits in front of the last layer.  h: the network's masked state in LDS; h' goes to the free buffer, is copied over h
// when the launch advances the state (keep), and is normalised into the other buffer under the hidden norm: the last layer reads it from there
template <bool LN, bool GRU = false>
__device__ __forceinline__ void actor_net(const ActorNet& net, const float* inv_n, int hidden, int feat, const float* __restrict__ params, float* bufA,
                                          float* bufB, float* out, float* part, int lane, int wave, int hidden_act, float* h = nullptr, bool keep = false,
                                          int tid = 0) {
  if constexpr (LN) {
    if (feat) {
      const float* g = params + ln_gamma_off(net, 0);
      ln_rows<ACT_LD>(bufB, bufB, net.dims[0], g, g + net.dims[0], inv_n[0], part, nullptr, lane, wave);
    }
  }
  const float* x = bufB;
  float* y = bufA;
  for (int l = 0; l < net.n_layers; l++) {
    const bool last = l + 1 == net.n_layers;
    if constexpr (GRU) {
      if (last) {
        const int H = net.dims[l];
        const int go = gru_layer(net, l, hidden, params, x, h, y, lane, wave);
        __syncthreads();
        if (keep)
          for (int e = tid; e < H * ACT_LD; e += ACT_THREADS) h[e] = y[e];      // read again only behind the last layer's barrier
        float* t = const_cast<float*>(x); x = y; y = t;
        if constexpr (LN) {
          if (hidden) {
            const float* g = params + go;
            ln_rows<ACT_LD>(x, y, H, g, g + H, inv_n[l], part, nullptr, lane, wave);
            x = y;
          }
        }
      }
    }
    actor_layer_of<ACT_LD>(net, l, params, x, last ? out : y, lane, wave, hidden_act);
    __syncthreads();
    if constexpr (LN) {
      if (!last && hidden) {
        const int Nout = net.dims[l + 1];
        const float* g = params + ln_gamma_off(net, l + 1);
        ln_rows<ACT_LD>(y, y, Nout, g, g + Nout, inv_n[l + 1], part, nullptr, lane, wave);
      }
    }
    float* t = const_cast<float*>(x); x = y; y = t;
  }
}

// GRU: the state of both networks sits behind the partial rows, [Ha + Hc][ACT_LD], loaded masked in front of the networks and stored behind
// actor_finish, the last reader of a parameter.  The critic of a recurrent handle runs whether or not its value is asked for: its state advances
// gparams / gsh: the parameter buffer and the shapes as __restrict__ kernel arguments of the recurrent entry points (kernels_gru.hpp, SCALAR WEIGHT LOADS)
template <bool LN, bool GRU = false>
__device__ __forceinline__ void actor_body(const ActorArgs& a, const GruArgs& gr, const float* __restrict__ gparams = nullptr, const ActorShapes* __restrict__ gsh = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float act_lds[];
  float* bufA = act_lds;
  float* bufB = act_lds + (size_t)a.ldh * ACT_LD;
  float* out = act_lds + (size_t)2 * a.ldh * ACT_LD;       // [4][ACT_LD]: mean 0..2, value
  float* part = LN ? out + 4 * ACT_LD : nullptr;           // [LN_PART][ACT_LD]
  float* hs = GRU ? out + (4 + (LN ? LN_PART : 0)) * ACT_LD : nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * ACT_ROWS;
  const int hidden_act = a.relu ? 2 : 1;
  const ActorShapes& shp = GRU ? *gsh : a.sh;
  const int hidden = LN ? shp.hidden : 0, feat = LN ? shp.feat : 0;
  const bool sample = a.actions != nullptr;                // false: the value-only launch behind the last step
  if constexpr (GRU) gru_load_state(gr.state, gr.done, row0, a.rows, a.Aw, gr.Ha + gr.Hc, hs, tid);      // the observation load's barrier covers it
  if (sample) {
    actor_load_obs(a.obs, row0, a.rows, a.D, bufB, tid);
    __syncthreads();
    if constexpr (GRU) actor_net<LN, true>(gsh->actor, gsh->inv_actor, hidden, feat, gparams, bufA, bufB, out, part, lane, wave, hidden_act, hs, true, tid);
    else actor_net<LN>(a.sh.actor, a.sh.inv_actor, hidden, feat, a.params, bufA, bufB, out, part, lane, wave, hidden_act);
  }
  bool critic = a.sh.critic.n_layers > 0 && a.value != nullptr;
  if constexpr (GRU) critic = gr.Hc > 0 && (sample || a.value != nullptr);
  if (critic) {
    actor_load_obs(a.obs, row0, a.rows, a.D, bufB, tid);
    __syncthreads();
    if constexpr (GRU)
      actor_net<LN, true>(gsh->critic, gsh->inv_critic, hidden, feat, gparams, bufA, bufB, out + 3 * ACT_LD, part, lane, wave, hidden_act,
                          hs + (size_t)gr.Ha * ACT_LD, sample, tid);
    else actor_net<LN>(a.sh.critic, a.sh.inv_critic, hidden, feat, a.params, bufA, bufB, out + 3 * ACT_LD, part, lane, wave, hidden_act);
  }
  if constexpr (GRU) {
    if (wave == 0) actor_finish(a, out, sample, critic && a.value != nullptr, row0, lane);
    __syncthreads();       // a launch without a network to walk has had no barrier behind the state's load
    gru_store_state(hs, gr.state, row0, a.rows, gr.Ha + gr.Hc, tid);
    if (sample && gr.record != nullptr) gru_store_state(hs, gr.record, row0, a.rows, gr.Ha + gr.Hc, tid);
  } else {
    if (wave != 0) return;
    actor_finish(a, out, sample, critic, row0, lane);
  }
}
template <bool LN>
__device__ __forceinline__ void actor_body(const ActorArgs& a) { actor_body<LN, false>(a, GruArgs{}); }
__global__ void __launch_bounds__(ACT_THREADS) k_actor(ActorArgs a) { actor_body<false>(a); }
__global__ void __launch_bounds__(ACT_THREADS) k_actor_ln(ActorArgs a) { actor_body<true>(a); }
extern "C" __global__ void __launch_bounds__(ACT_THREADS) k_actor_gru(ActorArgs a, GruArgs g, const float* __restrict__ params, const ActorShapes* __restrict__ sh) {
  actor_body<false, true>(a, g, params, sh);
}
extern "C" __global__ void __launch_bounds__(ACT_THREADS) k_actor_gru_ln(ActorArgs a, GruArgs g, const float* __restrict__ params, const ActorShapes* __restrict__ sh) {
  actor_body<true, true>(a, g, params, sh);
}

// ---- k_ppo_grad / k_ln_grad -------------------------------------------------------------------------------------------------------------------------
// forward of one network with every layer output kept: observation at lds[0], hidden output l behind it at (sum of the widths below it) rows, the
// last layer at `out`.  LN: what is kept of a normalised layer is its activation; u goes to U, mu and rstd of the norm in front of layer l to stat[2 l]
template <int LD, bool LN>
__device__ __forceinline__ void ppo_forward(const ActorNet& net, const float* inv_n, int hidden, int feat, const float* __restrict__ params, float* lds, int D,
                                            float* U, float* stat, float* part, float* out, int row, int wave, int hidden_act) {
  const float* x = lds;
  if constexpr (LN) {
    if (feat) {
      const float* g = params + ln_gamma_off(net, 0);
      ln_rows<LD>(lds, U, D, g, g + D, inv_n[0], part, stat, row, wave);
      x = U;
    }
  }
  float* y = lds + (size_t)D * LD;
  for (int l = 0; l < net.n_layers; l++) {
    const bool last = l + 1 == net.n_layers;
    const int Nout = net.dims[l + 1];
    actor_layer_of<LD>(net, l, params, x, last ? out : y, row, wave, hidden_act);
    __syncthreads();
    x = y;
    if constexpr (LN) {
      if (!last && hidden) {
        const float* g = params + ln_gamma_off(net, l + 1);
        ln_rows<LD>(y, U, Nout, g, g + Nout, inv_n[l + 1], part, stat + (size_t)2 * (l + 1) * LD, row, wave);
        x = U;
      }
    }
    y += (size_t)Nout * LD;
  }
}

// backward of one network: `out` holds the delta of the last layer; walks the layers down, weight gradient first, then the delta below in place.
// LN, where the layer's input is normalised: u of the input into U again, the weight gradient, du over U (ppo_dx without an activation derivative),
// the norm's backward (delta over the stored activation in place).  A layer whose input is not normalised goes the plain way
template <int LD, int RT, bool LN>
__device__ __forceinline__ void ppo_backward(const ActorNet& net, const float* inv_n, int hidden, int feat, const float* __restrict__ params,
                                             float* __restrict__ pg, float* lds, int D, float* U, float* stat, float* part, float* out, int row, int wave,
                                             int tid, int relu, bool first) {
  int below = 0;                       // rows under the input of layer l: D + hidden widths 1 .. l - 1, minus the input's own
  for (int l = 1; l + 1 < net.n_layers; l++) below += net.dims[l];
  // x of the last layer starts at row D + (sum of hidden widths but the last); for a single-layer network it is the observation
  float* dY = out;
  for (int l = net.n_layers - 1; l >= 0; l--) {
    const int K = net.dims[l], Nout = net.dims[l + 1];
    float* a = l == 0 ? lds : lds + (size_t)(D + below) * LD;      // the stored input of layer l: the observation, or the activation below
    const bool normed = LN && (l == 0 ? feat != 0 : hidden != 0);
    const int go = normed ? ln_gamma_off(net, l) : 0;
    const float* st = LN ? stat + (size_t)2 * l * LD : nullptr;
    const float* x = a;
    if constexpr (LN) {
      if (normed) {
        ln_again<LD>(a, U, K, params + go, params + go + K, st, row, wave);
        __syncthreads();
        x = U;
      }
    }
    ppo_dw<LD, RT>(dY, x, K, Nout, pg + net.w_off[l], pg + net.w_off[l] + (size_t)K * Nout, first, tid);
    __syncthreads();
    if (l == 0 && !normed) break;
    if (!normed) {
      ppo_dx<LD>(params + net.w_off[l], K, Nout, dY, a, row, wave, relu);
      __syncthreads();
    } else if constexpr (LN) {
      ppo_dx<LD, true>(params + net.w_off[l], K, Nout, dY, U, row, wave, relu);
      __syncthreads();
      if (l == 0) {                    // the feature norm: nothing lies below the observation
        ln_back<LD, RT, false>(a, U, K, params + go, inv_n[0], st, part, pg + go, pg + go + K, first, relu, row, tid & 63, wave);
        break;
      }
      ln_back<LD, RT, true>(a, U, K, params + go, inv_n[l], st, part, pg + go, pg + go + K, first, relu, row, tid & 63, wave);
    }
    dY = a;
    if (l >= 2) below -= net.dims[l - 1];
  }
}

// uw: the rows of U (LN only).  LDS from the top down: the sample indices, 4 output rows, and with LN the partials, the statistics and U under them.
// No __restrict__ here: the entry points' arguments carry it, and a second set of no-alias scopes from the inlined body costs k_ppo_grad 12 - 14
// more spilled SGPRs (116 - 118 against 102 - 104 without)
template <int RT, bool LN>
__device__ __forceinline__ void ppo_grad_body(const float* params, const ActorShapes* sh, int log_std_off, int n_params, int D, int rows_lds, int uw, int relu,
                                              const PpoTraj& tr, const PpoLoss& ls, float* part_all, double* pst) {
  constexpr int LD = RT + 1;
  extern __shared__ __attribute__((aligned(16))) float ppo_lds[];
  float* out = ppo_lds + (size_t)(rows_lds - 4) * LD;
  float* part = LN ? out - (size_t)LN_PART * LD : nullptr;
  float* stat = LN ? part - (size_t)LN_STAT * LD : nullptr;
  float* U = LN ? stat - (size_t)uw * LD : nullptr;
  long long* srow = reinterpret_cast<long long*>(ppo_lds + (size_t)rows_lds * LD + (((size_t)rows_lds * LD) & 1));      // 8-byte aligned
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row = lane & (RT - 1);
  const int hidden_act = relu ? 2 : 1;
  const int hidden = LN ? sh->hidden : 0, feat = LN ? sh->feat : 0;
  float* pg = part_all + (size_t)blockIdx.x * n_params;
  const long long tiles = (tr.count + RT - 1) / RT;
  PpoSums S;
  bool first_tile = true;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    ppo_load_tile<LD, RT>(ppo_lds, srow, tr.packed, tr.stride, tr.rows, tr.n_total, tr.index, tr.first, tr.count, tile, D, tid);
    const bool valid = tile * RT + lane < tr.count && lane < RT;
    // ---- actor ----
    ppo_forward<LD, LN>(sh->actor, sh->inv_actor, hidden, feat, params, ppo_lds, D, U, stat, part, out, row, wave, hidden_act);
    if (wave == 0) ppo_actor_head<LD, RT>(params, log_std_off, out, srow, row, lane, valid, tr.actions, tr.logp_old, tr.adv, ls, S);
    __syncthreads();
    ppo_backward<LD, RT, LN>(sh->actor, sh->inv_actor, hidden, feat, params, pg, ppo_lds, D, U, stat, part, out, row, wave, tid, relu, first_tile);
    // ---- critic: the observation is still in place ----
    ppo_forward<LD, LN>(sh->critic, sh->inv_critic, hidden, feat, params, ppo_lds, D, U, stat, part, out + 3 * LD, row, wave, hidden_act);
    if (wave == 0) ppo_critic_head<LD, RT>(out, srow, row, lane, valid, tr.value, tr.ret, ls, S);
    __syncthreads();
    ppo_backward<LD, RT, LN>(sh->critic, sh->inv_critic, hidden, feat, params, pg, ppo_lds, D, U, stat, part, out + 3 * LD, row, wave, tid, relu, first_tile);
    first_tile = false;
  }
  if (wave != 0) return;
  ppo_store_sums(S, lane, pst + (size_t)blockIdx.x * PPO_PST);
}
// The order of the arguments is chosen by what the register allocator makes of it (it decides how the kernel arguments are fetched): with the two
// structs side by side behind the sizes, k_ppo_grad<64> reloads spilled SGPRs in 399 places instead of 243, and an epoch measured 3 % slower
template <int RT>
__global__ void __launch_bounds__(ACT_THREADS) k_ppo_grad(const float* __restrict__ params, const ActorShapes* __restrict__ sh, PpoTraj tr, int log_std_off, int n_params, int D,
                                                          int rows_lds, int uw, int relu, float* __restrict__ part_all, double* __restrict__ pst, PpoLoss ls) {
  ppo_grad_body<RT, false>(params, sh, log_std_off, n_params, D, rows_lds, uw, relu, tr, ls, part_all, pst);
}
template <int RT>
__global__ void __launch_bounds__(ACT_THREADS) k_ln_grad(const float* __restrict__ params, const ActorShapes* __restrict__ sh, PpoTraj tr, int log_std_off, int n_params, int D,
                                                         int rows_lds, int uw, int relu, float* __restrict__ part_all, double* __restrict__ pst, PpoLoss ls) {
  ppo_grad_body<RT, true>(params, sh, log_std_off, n_params, D, rows_lds, uw, relu, tr, ls, part_all, pst);
}
