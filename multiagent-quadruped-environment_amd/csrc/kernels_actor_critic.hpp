// kernels_actor_critic.hpp -- the network walks of the engine's actor-critic and the entry points built on them: k_actor / k_actor_ln and, with a
// GRU cell in front of the output layer (kernels_gru.hpp; the compile-time parameter GRU), k_actor_gru / k_actor_gru_ln (the rollout's actor,
// mqe_rollout), k_ppo_grad<RT> / k_ln_grad<RT> (the PPO gradient, mqe_ppo_grad) and, for a recurrent handle, k_bptt_grad<RT> / k_bptt_ln_grad<RT>
// (the same gradient through time over chunks of L steps; kernels_bptt.hpp states the walk, bptt_network below is it).  Each walk is stated once, with the layer norm a
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
#include "kernels_bptt.hpp"

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
// last layer at `out`.  LN: what is kept of a normalised layer is its activation; u goes to U, mu and rstd of the norm in front of layer l to stat[2 l].
// BASE (the recurrent walk, which stops in front of the cell): the hidden layers alone, n_layers - 1 of them
template <int LD, bool LN, bool BASE = false>
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
  for (int l = 0; l < net.n_layers - (BASE ? 1 : 0); l++) {
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

// backward of one network: `out` holds the delta of the last layer (BASE, the recurrent walk: of the last HIDDEN layer, n_layers - 2 -- the delta the
// cell's backward left over that layer's stored output); walks the layers down, weight gradient first, then the delta below in place.
// LN, where the layer's input is normalised: u of the input into U again, the weight gradient, du over U (ppo_dx without an activation derivative),
// the norm's backward (delta over the stored activation in place).  A layer whose input is not normalised goes the plain way
template <int LD, int RT, bool LN, bool BASE = false>
__device__ __forceinline__ void ppo_backward(const ActorNet& net, const float* inv_n, int hidden, int feat, const float* __restrict__ params,
                                             float* __restrict__ pg, float* lds, int D, float* U, float* stat, float* part, float* out, int row, int wave,
                                             int tid, int relu, bool first) {
  int below = 0;                       // rows under the input of layer l: D + hidden widths 1 .. l - 1, minus the input's own
  for (int l = 1; l + 1 < net.n_layers - (BASE ? 1 : 0); l++) below += net.dims[l];
  // x of the last layer starts at row D + (sum of hidden widths but the last); for a single-layer network it is the observation
  float* dY = out;
  for (int l = net.n_layers - 1 - (BASE ? 1 : 0); l >= 0; l--) {
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
        ln_back<LD, RT, 0>(a, U, K, params + go, inv_n[0], st, part, pg + go, pg + go + K, first, relu, row, tid & 63, wave);
        break;
      }
      ln_back<LD, RT, 1>(a, U, K, params + go, inv_n[l], st, part, pg + go, pg + go + K, first, relu, row, tid & 63, wave);
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

// ---- k_bptt_grad / k_bptt_ln_grad (kernels_bptt.hpp: the chunks, the state, the cell's backward, the LDS rule) -----------------------------------------
// one network over the L steps of the tile's chunks: the forward sweep that keeps the input states, then the backward sweep.  actor: which of the two
// (its rows in `out` and in the state, its loss head).  LDS beside k_ln_grad's: cell = [h_in | r z n gh_n | h' | carried dh], H rows each; stat2:
// (mu, rstd) of the norm behind the cell; dn: the done bytes of steps j and j + 1 (slot j & 1); sums: the running statistics
template <int RT, bool LN>
__device__ __forceinline__ void bptt_network(const ActorNet& net, const float* inv_n, int hidden, int feat, const float* __restrict__ params, float* __restrict__ pg,
                                             float* __restrict__ scr, bool actor, int log_std_off, int D, int relu, const PpoTraj& tr, const PpoLoss& ls,
                                             const BpttArgs& b, float* lds, float* cell, float* U, float* stat, float* stat2, float* part, float* out,
                                             long long* srow, const long long* crow, int* dn, double* sums, long long tile, bool first_tile, int tid) {
  constexpr int LD = RT + 1;
  // what derives from the thread index is formed again in front of every phase (BPTT_FRESH): computed once in front of the tile loop, the phases' LDS
  // addresses and masks stay in registers across all of them, and the kernel spills 30 - 70 VGPRs
  int lane, row, wave;
#define BPTT_FRESH() do { asm volatile("" : "+v"(tid)); lane = tid & 63; row = lane & (RT - 1); wave = __builtin_amdgcn_readfirstlane(tid >> 6); } while (0)
  BPTT_FRESH();
  const int hidden_act = relu ? 2 : 1;
  const int nl = net.n_layers, H = net.dims[nl - 1], Nout = net.dims[nl], L = b.L;
  int below = 0;
  for (int l = 1; l + 1 < nl; l++) below += net.dims[l];
  float* a_last = lds + (size_t)(D + below) * LD;                // the stored output of the last hidden layer
  float* hin = cell;
  float* g = cell + (size_t)H * LD;
  float* hp = cell + (size_t)5 * H * LD;
  float* carry = cell + (size_t)6 * H * LD;
  const bool normed = LN && hidden != 0;
  const float* x = normed ? U : a_last;                          // the cell's input
  float* ho = out + (actor ? 0 : 3) * LD;
  const int coff = net.w_off[nl - 1] - gru_param_floats(H, normed);      // the cell's block; gru.norm.weight follows its 6 H H + 6 H floats
  const int cgo = coff + 6 * H * H + 6 * H, lgo = normed ? ln_gamma_off(net, nl - 1) : 0;
  const float* Wih = params + coff;
  const float* Whh = Wih + (size_t)3 * H * H;
  const float* Wo = params + net.w_off[nl - 1];
  const size_t step = (size_t)H * RT;
  // ---- forward sweep: h_in of steps 1 .. L - 1 ----
  bptt_load_step<LD, RT>(lds, srow, dn, crow, tr.packed, tr.stride, tr.rows, b, 0, D, tid);
  bptt_load_tail<LD, RT>(hin, srow, dn, tr.packed, tr.stride, tr.rows, b, actor ? 0 : b.Ha, H, tid);
  __syncthreads();
  for (int j = 0; j + 1 < L; j++) {
    BPTT_FRESH();
    ppo_forward<LD, LN, true>(net, inv_n, hidden, feat, params, lds, D, U, stat, part, ho, row, wave, hidden_act);
    gru_layer<LD>(net, nl - 1, normed, params, x, hin, hp, row, wave);
    __syncthreads();
    bptt_load_step<LD, RT>(lds, srow, dn + ((j + 1) & 1) * 64, crow, tr.packed, tr.stride, tr.rows, b, j + 1, D, tid);
    bptt_keep_state<LD, RT>(hp, hin, dn + ((j + 1) & 1) * 64, scr + (size_t)(j + 1) * step, H, tid);
    __syncthreads();
  }
  // ---- backward sweep: the observation and h_in of step L - 1 are in place ----
  for (int j = L - 1; j >= 0; j--) {
    const bool first = first_tile && j == L - 1;
    BPTT_FRESH();
    if (j != L - 1) {
      bptt_load_step<LD, RT>(lds, srow, dn + (j & 1) * 64, crow, tr.packed, tr.stride, tr.rows, b, j, D, tid);
      if (j == 0) bptt_load_tail<LD, RT>(hin, srow, dn, tr.packed, tr.stride, tr.rows, b, actor ? 0 : b.Ha, H, tid);
      else bptt_fetch_state<LD, RT>(hin, scr + (size_t)j * step, H, tid);
      __syncthreads();
    }
    ppo_forward<LD, LN, true>(net, inv_n, hidden, feat, params, lds, D, U, stat, part, ho, row, wave, hidden_act);
    gru_layer<LD>(net, nl - 1, normed, params, x, hin, hp, row, wave, g);
    __syncthreads();
    const float* xo = hp;                                        // the head's input
    if constexpr (LN) {
      if (normed) {
        ln_rows<LD>(hp, U, H, params + cgo, params + cgo + H, inv_n[nl - 1], part, stat2, row, wave);
        xo = U;
      }
    }
    actor_layer_of<LD>(net, nl - 1, params, xo, ho, row, wave, hidden_act);
    __syncthreads();
    if (wave == 0) {                                             // the running statistics wait in LDS between the steps
      const bool valid = tile * RT + lane < tr.count && lane < RT;
      PpoSums S = bptt_sums<false>(sums, lane, PpoSums());
      if (actor) ppo_actor_head<LD, RT>(params, log_std_off, out, srow, row, lane, valid, tr.actions, tr.logp_old, tr.adv, ls, S);
      else ppo_critic_head<LD, RT>(out, srow, row, lane, valid, tr.value, tr.ret, ls, S);
      bptt_sums<true>(sums, lane, S);
    }
    __syncthreads();
    BPTT_FRESH();
    // the head: its weight gradient, then dh' over h' (through the norm behind the cell)
    ppo_dw<LD, RT>(ho, xo, H, Nout, pg + net.w_off[nl - 1], pg + net.w_off[nl - 1] + (size_t)H * Nout, first, tid);
    __syncthreads();
    if (!normed) {
      ppo_dx<LD, true>(Wo, H, Nout, ho, hp, row, wave, relu);
      __syncthreads();
    } else if constexpr (LN) {
      ppo_dx<LD, true>(Wo, H, Nout, ho, U, row, wave, relu);
      __syncthreads();
      ln_back<LD, RT, 2>(hp, U, H, params + cgo, inv_n[nl - 1], stat2, part, pg + cgo, pg + cgo + H, first, relu, row, lane, wave);
    }
    // the cell
    BPTT_FRESH();
    bptt_gates_back<LD>(H, g, hp, hin, carry, j == L - 1 ? nullptr : dn + ((j + 1) & 1) * 64, row, wave);
    if constexpr (LN) {
      if (normed) ln_again<LD>(a_last, U, H, params + lgo, params + lgo + H, stat + (size_t)2 * (nl - 1) * LD, row, wave);
    }
    __syncthreads();
    BPTT_FRESH();
    ppo_dw<LD, RT>(g, x, H, 3 * H, pg + coff, pg + coff + (size_t)6 * H * H, first, tid);
    __syncthreads();
    if (!normed) {
      ppo_dx<LD>(Wih, H, 3 * H, g, a_last, row, wave, relu);
    } else if constexpr (LN) {
      ppo_dx<LD, true>(Wih, H, 3 * H, g, U, row, wave, relu);
      __syncthreads();
      ln_back<LD, RT, 1>(a_last, U, H, params + lgo, inv_n[nl - 1], stat + (size_t)2 * (nl - 1) * LD, part, pg + lgo, pg + lgo + H, first, relu, row, lane, wave);
    }
    __syncthreads();
    bptt_rows<LD, false>(g + (size_t)2 * H * LD, g + (size_t)3 * H * LD, H, row, wave);      // dgh = (da_r, da_z, da_n r), contiguous
    __syncthreads();
    BPTT_FRESH();
    ppo_dw<LD, RT>(g, hin, H, 3 * H, pg + coff + (size_t)3 * H * H, pg + coff + (size_t)6 * H * H + 3 * H, first, tid);
    if (j > 0) {                                                 // the dh of step 0 is dropped
      ppo_dx<LD, true>(Whh, H, 3 * H, g, carry, row, wave, relu);
      __syncthreads();
      bptt_rows<LD, true>(carry, hp, H, row, wave);
    }
    __syncthreads();
    BPTT_FRESH();
    ppo_backward<LD, RT, LN, true>(net, inv_n, hidden, feat, params, pg, lds, D, U, stat, part, a_last, row, wave, tid, relu, first);
  }
#undef BPTT_FRESH
}

// the arguments are k_ppo_grad's, then the chunk addressing and the workgroups' state scratch.  LDS from the top down: the statistics, the done bytes, the
// chunks' and the step's sample numbers, 4 output rows, with LN the partials, the cell norm's statistics, the statistics and U, then the cell's 7 Hm rows.
// The two networks run one after the other through ONE copy of the walk (a loop of two: half the code, the scalar registers of one network)
template <int RT, bool LN>
__device__ __forceinline__ void bptt_grad_body(const float* params, const ActorShapes* sh, int log_std_off, int n_params, int D, int rows_lds, int uw, int relu,
                                               const PpoTraj& tr, const PpoLoss& ls, const BpttArgs& b, float* part_all, double* pst, float* hscr) {
  constexpr int LD = RT + 1;
  extern __shared__ __attribute__((aligned(16))) float bptt_lds[];
  float* out = bptt_lds + (size_t)(rows_lds - 4) * LD;
  float* part = LN ? out - (size_t)LN_PART * LD : nullptr;
  float* stat2 = LN ? part - (size_t)2 * LD : nullptr;
  float* stat = LN ? stat2 - (size_t)LN_STAT * LD : nullptr;
  float* U = LN ? stat - (size_t)uw * LD : nullptr;
  float* cell = (LN ? U : out) - (size_t)BPTT_CELL_ROWS * b.Hm * LD;
  long long* srow = reinterpret_cast<long long*>(bptt_lds + (size_t)rows_lds * LD + (((size_t)rows_lds * LD) & 1));      // 8-byte aligned
  long long* crow = srow + 64;
  int* dn = reinterpret_cast<int*>(crow + 64);                  // [2][64]: the done bytes of two steps, one int a row
  double* sums = reinterpret_cast<double*>(crow + 128);         // [7][64]: PpoSums per lane of wavefront 0
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (wave == 0) bptt_sums<true>(sums, lane, PpoSums());
  const int hidden = LN ? sh->hidden : 0, feat = LN ? sh->feat : 0;
  float* pg = part_all + (size_t)blockIdx.x * n_params;
  float* scr = hscr + (size_t)blockIdx.x * b.L * b.Hm * RT;
  const long long tiles = (tr.count + RT - 1) / RT;
  bool first_tile = true;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();                   // the last reader of crow is the tile before
    bptt_chunks<RT>(crow, tr, b, tile, tid);
    __syncthreads();
    for (int w = 0; w < 2; w++) {
      const bool actor = w == 0;
      bptt_network<RT, LN>(actor ? sh->actor : sh->critic, actor ? sh->inv_actor : sh->inv_critic, hidden, feat, params, pg, scr, actor, log_std_off, D, relu, tr, ls,
                           b, bptt_lds, cell, U, stat, stat2, part, out, srow, crow, dn, sums, tile, first_tile, tid);
    }
    first_tile = false;
  }
  if (wave != 0) return;
  ppo_store_sums(bptt_sums<false>(sums, lane, PpoSums()), lane, pst + (size_t)blockIdx.x * PPO_PST);
}
template <int RT>
__global__ void __launch_bounds__(ACT_THREADS) k_bptt_grad(const float* __restrict__ params, const ActorShapes* __restrict__ sh, PpoTraj tr, int log_std_off, int n_params,
                                                           int D, int rows_lds, int uw, int relu, float* __restrict__ part_all, double* __restrict__ pst, PpoLoss ls,
                                                           BpttArgs b, float* __restrict__ hscr) {
  bptt_grad_body<RT, false>(params, sh, log_std_off, n_params, D, rows_lds, uw, relu, tr, ls, b, part_all, pst, hscr);
}
template <int RT>
__global__ void __launch_bounds__(ACT_THREADS) k_bptt_ln_grad(const float* __restrict__ params, const ActorShapes* __restrict__ sh, PpoTraj tr, int log_std_off,
                                                              int n_params, int D, int rows_lds, int uw, int relu, float* __restrict__ part_all,
                                                              double* __restrict__ pst, PpoLoss ls, BpttArgs b, float* __restrict__ hscr) {
  bptt_grad_body<RT, true>(params, sh, log_std_off, n_params, D, rows_lds, uw, relu, tr, ls, b, part_all, pst, hscr);
}
