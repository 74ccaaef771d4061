// kernels_gru.hpp -- the recurrent actor-critic of an on-device rollout (MQE_ACTOR_RECURRENT; include/mqe_hip.h): the GRU cell, its carried state,
// its constants and its LDS rule.  The walk of kernels_actor_critic.hpp switches it in at compile time (GRU): k_actor_gru and k_actor_gru_ln are the
// instantiations with it, and a handle created without the bit never launches them.  The gradient is a kernel of its own: back-propagation through
// time over chunks of the recorded trajectory, k_bptt_grad / k_bptt_ln_grad (kernels_bptt.hpp; mqe_ppo_grad with MQE_PPO_BPTT), built on this file's cell.
//
// THE NETWORK, per network of the handle (each has its own cell and its own state; H = the width of the last hidden layer):
//     hidden layers (with their norms) -> x (H) -> GRU cell H -> H -> [LayerNorm(H) under the hidden norm: ln_rows] -> the output Linear
// THE CELL is torch.nn.GRU's, gate order r, z, n; W_ih, W_hh (3H, H) row-major, b_ih, b_hh (3H):
//     gi = W_ih x + b_ih;  gh = W_hh h + b_hh          every entry actor_layer's chain:  acc = b[o];  k ascending:  acc = fmaf(W[o][k], v[k], acc)
//     r  = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z)                  sigmoid(v) = 1.0f / (1.0f + expf(-v))
//     n  = tanhf(fmaf(r, gh_n, gi_n));   h' = fmaf(z, h - n, n)             (= (1 - z) n + z h)
// all f32; tests/gru_ref.py restates these rounding points on the host.
// PARAMETERS, per network, in front of the output layer's weight:  gru.weight_ih (3H, H), gru.weight_hh (3H, H), gru.bias_ih (3H), gru.bias_hh (3H)
// and, under the hidden norm, gru.norm.weight (H), gru.norm.bias (H).  So the cell's block ends at w_off[n_layers - 1]: no offsets beyond ActorNet's.
//
// THE STATE is [R'][Hs] floats, Hs = Ha + Hc, row r = the actor's Ha floats, then the critic's Hc; it belongs to the actor (mqe_actor_create makes it
// zeroed), not to DevState.  A launch evaluates its step from  h_in = state * (1 - done)  with done the byte of the row's env in the packed row the
// observation comes from (exactly 0.0f where done), and leaves h' UNMASKED in the state and, when recorded, in the tail of the next packed row.  The
// launch behind the last step (no draw) masks the state in place and advances nothing; with value_dev it also evaluates the critic from the masked state.
//
// LAYOUT: k_actor's (kernels_actor.hpp).  The state of the workgroup's 64 rows is loaded into LDS [Hs][65] by the observation's coalesced
// transposing load, masked on the way in.  A wavefront carries GRU_NB = 1 hidden unit at a time = its 3 gate rows per operand, and runs the x
// chains, then the h chains: 3 rows x 8 k of 16-byte scalar loads are 24 SGPRs, one LDS read feeds 3 FMAs (k_actor: 4).  Two units per pass
// measured 3 us SLOWER per launch (175 / 188 spilled SGPRs against 112 / 105; profiles/gru.txt).  h' goes to the free ping-pong buffer; behind the
// barrier it is copied over the old state in LDS, where it WAITS: every global store of the kernel -- the state's too, coalesced from LDS -- comes
// after the last weight load of both networks.
// SCALAR WEIGHT LOADS.  That ordering alone does not keep them scalar here: read through ActorArgs' plain pointer, as k_actor reads them, the
// compiler's no-clobber walk gives up in a kernel of this size (it has to pass every LDS store on the way back to the entry) and all weight
// loads become per-lane vector loads (80 global_load_dwordx4, 3 s_load_dwordx4).  So the parameter buffer and the shapes are kernel arguments
// of their own, `const ... * __restrict__` as k_ppo_grad's are: nothing the kernel writes may alias them, and the loads are scalar whatever lies
// between (0 global_load_dwordx4, 41 s_load_dwordx4 + 24 s_load_dwordx8; k_actor: 18 + 8).  The shapes come from device memory for the
// registers' sake: as words of the kernel-argument struct they stay live in SGPRs and the allocator leaves a 32-byte private frame object.
// THE ENTRY POINTS ARE extern "C": a kernel trace shows k_actor_gru / k_actor_gru_ln, and the resource tests of the plain kernels, which select
// their kernels by the C++-mangled prefix, keep seeing exactly the set they pin.
#pragma once
#include "mqe_common.hpp"
#include "kernels_actor.hpp"
#include "kernels_ln.hpp"

// the constants of the recurrent section of include/mqe_hip.h: stated there in words, defined here (the header's ACTOR / ROLLOUT define sets are
// pinned by the tests), mirrored in mqe/engine/abi.py; tests/test_gru.py compares the three
#define MQE_ACTOR_RECURRENT 16            // bit of the kind byte of mqe_actor_shape.activation: a GRU cell in front of the output layer of both networks
#define MQE_ROLLOUT_HIDDEN_IN 2           // mqe_rollout flags: the start state is read from the tail of packed row 0
#define MQE_ROLLOUT_HIDDEN_RECORD 4       // mqe_rollout flags: the tails of packed rows 0 .. T are written

#define GRU_NB 1                          // hidden units a wavefront carries per pass: 3 gate rows per operand
#define GRU_LDS_LIMIT (160 * 1024)        // the LDS of a workgroup

// what the recurrent kernels take beside ActorArgs (whose layout, a kernel argument of k_actor and k_actor_ln, stays as it is)
struct GruArgs {
  float* state;             // [rows][Hs], read and written in place (a workgroup touches its own 64 rows only)
  float* record;            // [rows][Hs] the tail of the next packed row, or null
  const uint8_t* done;      // [N] the done bytes of the packed row the observation comes from
  int Ha, Hc;               // widths of the two cells (Hc = 0: no critic)
};

// THE LDS RULE: the two ping-pong buffers of the widest layer input, the 4 output rows, the norm's partial rows, and the state of both networks
static inline size_t actor_gru_lds_bytes(int ldh, int Ha, int Hc, bool ln) { return (size_t)(2 * ldh + 4 + (ln ? LN_PART : 0) + Ha + Hc) * ACT_LD * sizeof(float); }
// floats of one network's cell in the parameter buffer
__host__ __device__ inline int gru_param_floats(int H, bool ln_hidden) { return 6 * H * H + 6 * H + (ln_hidden ? 2 * H : 0); }

// the state of the workgroup's 64 rows -> LDS [k][row], masked: coalesced (thread t reads float t of the 64 x Hs block), clamped at the end
__device__ __forceinline__ void gru_load_state(const float* __restrict__ state, const uint8_t* __restrict__ done, int row0, int rows, int Aw, int Hs, float* hs, int tid) {
  const size_t last = (size_t)rows * Hs - 1;
#pragma clang loop vectorize(disable) interleave(disable)
  for (int e = tid; e < ACT_ROWS * Hs; e += ACT_THREADS) {
    const int r = e / Hs, k = e - r * Hs;
    const size_t g = (size_t)row0 * Hs + e;
    const int row = min(row0 + r, rows - 1);
    const float v = state[g < last ? g : last];
    hs[k * ACT_LD + r] = done[row / Aw] ? 0.0f : v;
  }
}
// LDS [k][row] -> the state, or the record: the same coalesced pattern, rows past the end masked
__device__ __forceinline__ void gru_store_state(const float* hs, float* __restrict__ dst, int row0, int rows, int Hs, int tid) {
#pragma clang loop vectorize(disable) interleave(disable)
  for (int e = tid; e < ACT_ROWS * Hs; e += ACT_THREADS) {
    const int r = e / Hs, k = e - r * Hs;
    if (row0 + r >= rows) break;               // e ascends with r
    dst[(size_t)row0 * Hs + e] = hs[k * ACT_LD + r];
  }
}

// the three gate chains of GRU_NB units over one operand: acc[j][g] = b[g H + u_j] + sum over k ascending of W[g H + u_j][k] v[k]
template <bool VEC4, int LD = ACT_LD>
__device__ __forceinline__ void gru_chains(const float* __restrict__ W, const float* __restrict__ b, int H, int u0, const float* v, float (&acc)[GRU_NB][3], int lane) {
  const float* w[GRU_NB][3];
#pragma unroll
  for (int j = 0; j < GRU_NB; j++) {
    const int u = min(u0 + j, H - 1);            // a short last block recomputes the last unit and does not store it
#pragma unroll
    for (int g = 0; g < 3; g++) {
      w[j][g] = W + (size_t)(g * H + u) * H;
      acc[j][g] = b[g * H + u];
    }
  }
  int k = 0;
  if (VEC4) {
    for (; k + 8 <= H; k += 8) {
      float4 wa[GRU_NB][3], wb[GRU_NB][3];
      float xv[8];
#pragma unroll
      for (int j = 0; j < GRU_NB; j++)
#pragma unroll
        for (int g = 0; g < 3; g++) {
          wa[j][g] = *reinterpret_cast<const float4*>(__builtin_assume_aligned(w[j][g] + k, 16));
          wb[j][g] = *reinterpret_cast<const float4*>(__builtin_assume_aligned(w[j][g] + k + 4, 16));
        }
#pragma unroll
      for (int q = 0; q < 8; q++) xv[q] = v[(k + q) * LD + lane];
#pragma unroll
      for (int j = 0; j < GRU_NB; j++)
#pragma unroll
        for (int g = 0; g < 3; g++) {
          float a = acc[j][g];
          a = fmaf(wa[j][g].x, xv[0], a); a = fmaf(wa[j][g].y, xv[1], a); a = fmaf(wa[j][g].z, xv[2], a); a = fmaf(wa[j][g].w, xv[3], a);
          a = fmaf(wb[j][g].x, xv[4], a); a = fmaf(wb[j][g].y, xv[5], a); a = fmaf(wb[j][g].z, xv[6], a); a = fmaf(wb[j][g].w, xv[7], a);
          acc[j][g] = a;
        }
    }
  }
  for (; k + 4 <= H; k += 4) {
    float wv[GRU_NB][3][4], xv[4];
#pragma unroll
    for (int j = 0; j < GRU_NB; j++)
#pragma unroll
      for (int g = 0; g < 3; g++)
#pragma unroll
        for (int q = 0; q < 4; q++) wv[j][g][q] = w[j][g][k + q];
#pragma unroll
    for (int q = 0; q < 4; q++) xv[q] = v[(k + q) * LD + lane];
#pragma unroll
    for (int j = 0; j < GRU_NB; j++)
#pragma unroll
      for (int g = 0; g < 3; g++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[j][g] = fmaf(wv[j][g][q], xv[q], acc[j][g]);
  }
  for (; k < H; k++) {
    const float xk = v[k * LD + lane];
#pragma unroll
    for (int j = 0; j < GRU_NB; j++)
#pragma unroll
      for (int g = 0; g < 3; g++) acc[j][g] = fmaf(w[j][g][k], xk, acc[j][g]);
  }
}

__device__ __forceinline__ float gru_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// the cell for the 64 rows of the workgroup: x, h (LDS, [H][ACT_LD]) -> y = h' (LDS, another buffer: every wavefront reads all of h).  No barrier.
// LD: the LDS row stride (the gradient's 32-row tiles use 33).  gates (the gradient's backward sweep, kernels_bptt.hpp; null: not kept): [4 H][LD], r, z, n, gh_n
template <bool VEC4, int LD = ACT_LD>
__device__ __forceinline__ void gru_cell(const float* __restrict__ p, int H, const float* x, const float* h, float* y, int lane, int wave, float* gates = nullptr) {
  const float* Wih = p;
  const float* Whh = p + (size_t)3 * H * H;
  const float* bih = p + (size_t)6 * H * H;
  const float* bhh = bih + 3 * H;
  for (int u0 = wave * GRU_NB; u0 < H; u0 += ACT_WAVES * GRU_NB) {
    float gi[GRU_NB][3], gh[GRU_NB][3];
    gru_chains<VEC4, LD>(Wih, bih, H, u0, x, gi, lane);
    gru_chains<VEC4, LD>(Whh, bhh, H, u0, h, gh, lane);
#pragma unroll
    for (int j = 0; j < GRU_NB; j++) {
      const float r = gru_sigmoid(gi[j][0] + gh[j][0]);
      const float z = gru_sigmoid(gi[j][1] + gh[j][1]);
      const float n = tanhf(fmaf(r, gh[j][2], gi[j][2]));
      const float hp = h[min(u0 + j, H - 1) * LD + lane];
      if (u0 + j < H) y[(u0 + j) * LD + lane] = fmaf(z, hp - n, n);
      if (gates != nullptr && u0 + j < H) {
        float* gu = gates + (u0 + j) * LD + lane;
        gu[0] = r; gu[(size_t)H * LD] = z; gu[(size_t)2 * H * LD] = n; gu[(size_t)3 * H * LD] = gh[j][2];
      }
    }
  }
}
// the cell in front of layer l = n_layers - 1 of a network: its block by its offset, and the ONE alignment test that picks the 16-byte loads (both
// matrices start on the same residue).  -> the offset of gru.norm.weight
template <int LD = ACT_LD>
__device__ __forceinline__ int gru_layer(const ActorNet& net, int l, int hidden, const float* __restrict__ params, const float* x, const float* h, float* y, int lane,
                                         int wave, float* gates = nullptr) {
  const int H = net.dims[l], off = net.w_off[l] - gru_param_floats(H, hidden != 0);
  if (((H | off) & 3) == 0) gru_cell<true, LD>(params + off, H, x, h, y, lane, wave, gates);
  else gru_cell<false, LD>(params + off, H, x, h, y, lane, wave, gates);
  return off + 6 * H * H + 6 * H;
}
