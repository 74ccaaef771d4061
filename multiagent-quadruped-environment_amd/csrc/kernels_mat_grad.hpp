// kernels_mat_grad.hpp -- the PPO gradient of the Multi-Agent Transformer policy inside the engine (MQE_PPO_TRANSFORMER; include/mqe_hip.h, mqe_ppo_grad):
// the loss, the backward of the three operators of kernels_mat.hpp's program, the reverse walk, the tape, the two rules (LDS, scratch) and the kernels
// k_mat_grad and k_mat_reduce.  A call without the bit never launches them; a handle without MQE_ACTOR_TRANSFORMER is refused with it.
//
// THE LOSS is mqe_ppo_grad's (kernels_ppo.hpp: L_pi, L_v, the selects at the kinks, 1 / M, 1 / G, the six statistics -- its two loss heads run here unchanged)
// with MAT's head, all f32.  THE UNIT of the minibatch is the env-step group g = t N + n, standing for the samples g A' + a (MQE_PPO_JOINT's unit and
// numbering: the attention needs all A' agents of an env-step); M = count A'; k_joint_expand writes the flat list.  Per group:
//     mean, value = the parallel pass of kernels_mat.hpp over the group (s_0 = 0, s_a = actions[a - 1]: DATA, no gradient flows into s)
//     sigma_j = 0.5 sigmoid(log_std_j);  z_j = (a_j - mean_j) / sigma_j;  logp = sum_j (-0.5 z_j^2 - ln sigma_j) - 1.5 ln(2 pi)
//     H = sum_j ln sigma_j + 1.5 (1 + ln(2 pi))
//     dlogp/dmean_j = z_j / sigma_j;  dlogp/dlog_std_j = (z_j^2 - 1)(1 - sigmoid(log_std_j));  log_std_j additionally receives -entropy_coef (1 - sigmoid(log_std_j))
// HOW THE HEADS ARE REUSED.  ppo_actor_head reads three numbers l_j and forms exp(-l_j), z_j = (a_j - mean_j) exp(-l_j), -0.5 z_j^2 - l_j and the sums of
// dL/dlogp (z_j^2 - 1).  Here l_j = logf(0.5f * gru_sigmoid(log_std_j)), formed once per workgroup into LDS: exp(-l_j) = 1 / sigma_j, and the three sums are dL/dl_j.
// k_mat_reduce (k_ppo_reduce's order, f64) applies dl_j / dlog_std_j = 1 - sigmoid(log_std_j):  grad[log_std_j] = (sum - entropy_coef) (1 - sigmoid(log_std_j)),
// and states H from ln sigma_j.  k_ppo_reduce is untouched: handles without the bit get the bits they got.
// With MQE_PPO_JOINT the ratio is the group's and the policy term is divided by G = count; without it the ratio is per sample and every mean is over M.
//
// LAYOUT: the family's.  1024 threads = 16 wavefronts, a tile of 64 rows = 64 / A' whole groups (a group is A' aligned rows, wholly valid or wholly padding),
// LANE = ROW in the forward and backward-data phases, ppo_dw's 4 x 4 thread blocks for the weight gradients, activations in LDS as [k][row] with stride 65,
// weights through wave-uniform scalar loads, persistent workgroups (at most PPO_MAX_WG: workgroup b of G takes tiles b, b + G, ...), each continuing its fmaf
// chains over its tiles in the per-handle partials; k_mat_reduce adds the workgroups in order.  No floating-point atomics: the same bits on every run.
// Rows past the end of the minibatch load the last group (clamped) and carry delta = 0: they add +0 to every chain; a padded group shares no attention with a
// valid one.  Every element of the partial gradient is stored by every workgroup on every tile, so every element of grad_dev is written by every call.
//
// FORWARD (matg_forward): mat_run's own chain -- actor_layer, ln_rows, mat_attend, mat_post's statements -- over MAT_ENC and then ONE pass of MAT_DEC over the
// recorded actions: mean and value have the bits the rollout produced.  Behind its operator each slab the backward needs goes to THE TAPE.
// BACKWARD (matg_backward): ONE interpreter walks the same two tables in reverse, the decoder first, then the encoder.  Every LDS slot of the program has a
// gradient slot at the same address (the observation's lies behind dB0); `live` says which hold a gradient.  Per operator:
//   Linear     behind a GELU first  d_pre = d * (0.5 (1 + erff(x / sqrt 2)) + x exp(-x^2 / 2) / sqrt(2 pi))  from the taped pre-activation x, by the thread that
//              applied the GELU;  behind a residual the incoming gradient d also goes to the residual's source;  ppo_dw(d, taped input) for dW and db;
//              ppo_dx<RAW> for dx.  act_fc (input s) has a weight gradient only.
//   LayerNorm  ln_back with DX = 2 (da alone; dgamma, dbeta as there) on the taped input a and (mu, rstd);  obs_norm: DX = 0, nothing lies below the observation.
//   Attention  per row i of a group, J(i) the forward's index set ({0 .. A' - 1}, masked {0 .. i}), p recomputed from the taped q and k by the forward's
//              statements (matg_probs), c the host-formed scale:
//                  dp_ij = dY_i . v_j  (n ascending);   r_i = sum_{j in J(i)} p_ij dp_ij  (j ascending, fmaf);   ds_ij = p_ij (dp_ij - r_i)
//                  dv_j = sum_{i : j in J(i)} p_ij dY_i;   dq_i = c sum_{j in J(i)} ds_ij k_j;   dk_j = c sum_{i : j in J(i)} ds_ij q_i     (i, j ascending, fmaf from 0)
//              Wavefront 0 forms p and ds of its lane's row and leaves them in LDS ([j][row], in the norm's partial rows); behind a barrier the features n are
//              split over the wavefronts (n = wave, wave + 16, ...) and every lane reads its group's columns out of LDS, as the forward does.  No cross-lane
//              operation; an index outside J is excluded by select.  dq, dk, dv replace q, k, v in place (a wavefront owns row n of all three).
// WHERE GRADIENTS MEET: the first contribution to a slot is stored, every later one is added (one f32 addition per element), in the order the reverse walk
// meets them:  the x of attn and of attn1 = the residual of proj, + dx of value, + dx of query, + dx of key;  the decoder's ln1 output (key and value input
// of attn2) = dx of attn2.value, + dx of attn2.key;  rep = the decoder's residual (attn2.proj), + dx of attn2.query, + dx of the value head's head0 (met
// first in the encoder's own walk): the encoder is then walked once with that sum.  The input of an mlp block = the residual of mlp1, + dx of mlp0.
//
// THE TAPE.  What the backward needs is 40 E + 2 D + 20 rows a tile (E = 64, D = 128: 709 KiB at 64 rows): it cannot live in LDS.  Each workgroup owns a tape in
// per-handle global scratch, rows of 64 floats, used as a stack: the forward pushes, behind its operator, a Linear's input (not s, which stays in LDS; not when
// the next operator is a Linear on the same input: key, query, value share one slab, pushed by the last), the pre-activation in front of a GELU, a norm's
// input and (mu, rstd), an attention's q, k, v; the backward pops when the operator is reached.  Closed count: 2 D + 40 E + 20 rows (the host holds the
// walk to it).  SCRATCH RULE (mat_grad_scratch_bytes, the one statement): PPO_MAX_WG tapes.  The first flagged call allocates it (and synchronises once).
// LDS RULE (mat_grad_lds_bytes, the one statement; the first flagged call refuses above MATG_LDS_LIMIT with -5): T = max(D, E) + 2 rows (the observation; a
// popped input; a norm's input and statistics), G = max(6 E, E + D) rows (the program's six slabs = their gradient slots; E + D: obs_fc's delta and the
// observation's), X = E rows (a dx that has to be added), 2 rows of (mu, rstd), 3 of s, 4 output rows, the norm's 32 partial rows, each 65 floats; in front of
// them the tile's 64 sample numbers (64-bit) and the three l_j.  E = 64, D = 128: 619 rows = 157.7 KiB; E = 64 fits for every D <= 128.
#pragma once
#include "mqe_common.hpp"
#include "kernels_actor.hpp"
#include "kernels_ppo.hpp"
#include "kernels_ln.hpp"
#include "kernels_gru.hpp"
#include "kernels_mat.hpp"

// the constant of the transformer section of include/mqe_hip.h: stated there in words, defined here (the header's define set is pinned by the tests),
// mirrored in mqe/engine/abi.py; tests/test_mat_grad.py compares the three
#define MQE_PPO_TRANSFORMER 65536         // bit 16 of mqe_ppo_grad's flags, the first above the chunk-length byte

#define MATG_LDS_LIMIT (160 * 1024)       // the LDS of a workgroup
#define MATG_FIXED_ROWS (2 + 3 + 4 + LN_PART)      // (mu, rstd), s, the output rows, the norm's partials
#define MATG_HEAD_BYTES (64 * 8 + 16)     // the tile's sample numbers, the three l_j
#define MATG_MAX(a, b) ((a) > (b) ? (a) : (b))

static inline size_t mat_grad_lds_bytes(int D, int E) { return (size_t)(MATG_MAX(D, E) + 2 + MATG_MAX(MAT_SLABS * E, E + D) + E + MATG_FIXED_ROWS) * ACT_LD * sizeof(float) + MATG_HEAD_BYTES; }
static inline size_t mat_grad_scratch_bytes(int D, int E) { return (size_t)PPO_MAX_WG * (2 * D + 40 * E + 20) * ACT_ROWS * sizeof(float); }

// a Linear pushes (pops) its input unless it is s or the next operator is a Linear on the same input
__host__ __device__ inline bool matg_keeps_x(const MatOp* prog, int n, int i) {
  return prog[i].src != MAT_S && !(i + 1 < n && prog[i + 1].kind == MAT_LIN && prog[i + 1].src == prog[i].src);
}
// rows one operator pushes: the host's walk of THE TAPE (mqe_ppo_grad holds the closed count to it)
static inline int matg_tape_rows(const MatOp* prog, int n, int D, int E) {
  int rows = 0;
  for (int i = 0; i < n; i++) {
    const MatOp& op = prog[i];
    if (op.kind == MAT_LN) rows += mat_width(op.kin, D, E) + 2;
    else if (op.kind == MAT_ATT) rows += 3 * E;
    else rows += (matg_keeps_x(prog, n, i) ? mat_width(op.kin, D, E) : 0) + (op.post == MAT_GELU ? mat_width(op.nout, D, E) : 0);
  }
  return rows;
}

struct MatgLds { float *T, *G, *X, *stat, *S, *out, *part; };

// the LDS slot of the program (grad: its gradient slot -- the same address, but the observation's, which lies behind dB0)
__device__ __forceinline__ float* matg_slot(const MatgLds& m, int slot, int E, bool grad) {
  if (slot == MAT_O) return grad ? m.G + (size_t)E * ACT_LD : m.T;
  if (slot <= MAT_REP) return m.G + (size_t)(slot - MAT_B0) * E * ACT_LD;
  return slot == MAT_S ? m.S : slot == MAT_OUT ? m.out : m.out + 3 * ACT_LD;
}

// the tape: rows of 64 floats.  No __restrict__: a slab is popped by other threads than pushed it (a barrier lies between)
__device__ __forceinline__ void matg_push(float* tape, int& tp, const float* lds, int rows, int tid) {
  float* t = tape + (size_t)tp * ACT_ROWS;
  for (int e = tid; e < rows * ACT_ROWS; e += ACT_THREADS) t[e] = lds[(e >> 6) * ACT_LD + (e & 63)];
  tp += rows;
}
__device__ __forceinline__ void matg_pop(const float* tape, int& tp, float* lds, int rows, int tid) {
  tp -= rows;
  const float* t = tape + (size_t)tp * ACT_ROWS;
  for (int e = tid; e < rows * ACT_ROWS; e += ACT_THREADS) lds[(e >> 6) * ACT_LD + (e & 63)] = t[e];
}
// where gradients meet: the first contribution is stored, a later one added
__device__ __forceinline__ void matg_meet(float* to, const float* from, int rows, bool add, int tid) {
  for (int e = tid; e < rows * ACT_ROWS; e += ACT_THREADS) {
    const int at = (e >> 6) * ACT_LD + (e & 63);
    to[at] = add ? to[at] + from[at] : from[at];
  }
}

// mat_post's GELU with the pre-activation taped, and its derivative applied to the incoming gradient: the thread that wrote the element (actor_layer's split)
__device__ __forceinline__ void matg_gelu(float* y, float* t, int Nout, int lane, int wave) {
  for (int o0 = wave * ACT_NB; o0 < Nout; o0 += ACT_WAVES * ACT_NB) {
#pragma unroll
    for (int j = 0; j < ACT_NB; j++) {
      if (o0 + j >= Nout) break;
      const int at = (o0 + j) * ACT_LD + lane;
      const float v = y[at];
      t[(o0 + j) * ACT_ROWS + lane] = v;
      y[at] = mat_gelu(v);
    }
  }
}
__device__ __forceinline__ void matg_gelu_back(float* d, const float* t, int Nout, int lane, int wave) {
  for (int o0 = wave * ACT_NB; o0 < Nout; o0 += ACT_WAVES * ACT_NB) {
#pragma unroll
    for (int j = 0; j < ACT_NB; j++) {
      if (o0 + j >= Nout) break;
      const int at = (o0 + j) * ACT_LD + lane;
      const float x = t[(o0 + j) * ACT_ROWS + lane];
      d[at] = d[at] * (0.5f * (1.0f + erff(x * 0.70710678f)) + x * expf(-0.5f * x * x) * 0.3989422804f);
    }
  }
}

// p of the lane's row: mat_attend's statements up to the division (kernels_mat.hpp), so the forward's bits; p_j = 0 outside J
__device__ __forceinline__ void matg_probs(const float* Q, const float* K, int E, int Aw, int g0, int last, float scale, int lane, float* e) {
  float s[MQE_MAX_AGENTS] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
  for (int k = 0; k < E; k++) {
    const float q = Q[k * ACT_LD + lane];
#pragma unroll
    for (int j = 0; j < MQE_MAX_AGENTS; j++)
      if (j < Aw) s[j] = fmaf(q, K[k * ACT_LD + g0 + j], s[j]);
  }
  float m = s[0] * scale, z = 0.0f;
#pragma unroll
  for (int j = 0; j < MQE_MAX_AGENTS; j++) {
    s[j] = s[j] * scale;
    m = (j <= last && s[j] > m) ? s[j] : m;
  }
#pragma unroll
  for (int j = 0; j < MQE_MAX_AGENTS; j++) {
    e[j] = j <= last ? expf(s[j] - m) : 0.0f;
    z = j == 0 ? e[0] : j <= last ? z + e[j] : z;
  }
#pragma unroll
  for (int j = 0; j < MQE_MAX_AGENTS; j++) e[j] = e[j] / z;
}

// backward of one head of attention: Q, K, V hold the taped q, k, v and receive dq, dk, dv in place; dY the gradient of y; P: 2 MQE_MAX_AGENTS rows
// ([j][row]: p, then ds).  Ends in a barrier
__device__ __forceinline__ void matg_attend_back(float* Q, float* K, float* V, const float* dY, float* P, int E, int Aw, bool masked, float scale, int lane, int wave) {
  const int i = lane & (Aw - 1), g0 = lane - i;
  const int last = masked ? i : Aw - 1;            // J(i) = {0 .. last}
  float* DS = P + MQE_MAX_AGENTS * ACT_LD;
  if (wave == 0) {
    float p[MQE_MAX_AGENTS], dp[MQE_MAX_AGENTS] = {0.0f, 0.0f, 0.0f, 0.0f};
    matg_probs(Q, K, E, Aw, g0, last, scale, lane, p);
#pragma unroll 4
    for (int n = 0; n < E; n++) {
      const float d = dY[n * ACT_LD + lane];
#pragma unroll
      for (int j = 0; j < MQE_MAX_AGENTS; j++)
        if (j < Aw) dp[j] = fmaf(d, V[n * ACT_LD + g0 + j], dp[j]);
    }
    float r = 0.0f;
#pragma unroll
    for (int j = 0; j < MQE_MAX_AGENTS; j++) r = j <= last ? fmaf(p[j], dp[j], r) : r;
#pragma unroll
    for (int j = 0; j < MQE_MAX_AGENTS; j++) {
      if (j < Aw) {
        P[j * ACT_LD + lane] = j <= last ? p[j] : 0.0f;
        DS[j * ACT_LD + lane] = j <= last ? p[j] * (dp[j] - r) : 0.0f;
      }
    }
  }
  __syncthreads();
  // the lane as row i: dq_i; the lane as column i: dk_i, dv_i over the rows ii whose J holds i (masked: ii >= i)
  float dsr[MQE_MAX_AGENTS], dsc[MQE_MAX_AGENTS], pc[MQE_MAX_AGENTS];
#pragma unroll
  for (int j = 0; j < MQE_MAX_AGENTS; j++) {
    const bool in = j < Aw;
    dsr[j] = in ? DS[j * ACT_LD + lane] : 0.0f;
    dsc[j] = in ? DS[i * ACT_LD + g0 + j] : 0.0f;
    pc[j] = in ? P[i * ACT_LD + g0 + j] : 0.0f;
  }
  for (int n = wave; n < E; n += ACT_WAVES) {
    float dq = 0.0f, dk = 0.0f, dv = 0.0f;
#pragma unroll
    for (int j = 0; j < MQE_MAX_AGENTS; j++) {
      if (j < Aw) {
        const float kj = K[n * ACT_LD + g0 + j], qj = Q[n * ACT_LD + g0 + j], dj = dY[n * ACT_LD + g0 + j];
        const float tq = fmaf(dsr[j], kj, dq), tk = fmaf(dsc[j], qj, dk), tv = fmaf(pc[j], dj, dv);
        dq = j <= last ? tq : dq;
        const bool col = masked ? j >= i : true;
        dk = col ? tk : dk;
        dv = col ? tv : dv;
      }
    }
    __builtin_amdgcn_wave_barrier();               // row n of Q, K, V is this wavefront's alone: every lane has read before any lane stores
    Q[n * ACT_LD + lane] = dq * scale;
    K[n * ACT_LD + lane] = dk * scale;
    V[n * ACT_LD + lane] = dv;
  }
  __syncthreads();
}

// the parameters of a Linear: the running offset, or one of the two narrow output layers behind both programs
__device__ __forceinline__ int matg_lin_at(const MatOp& op, int off, int tail, int E) {
  return op.where == MAT_RUNNING ? off : op.where == MAT_VALUE_OUT ? tail : tail + E + 1;
}

// the forward over both programs with the tape; -> the tape's height
__device__ __forceinline__ int matg_forward(const float* __restrict__ params, int dec, int tail, int D, int E, int Aw, const float* inv, const MatgLds& m, float* tape,
                                            int lane, int wave, int tid) {
  int tp = 0;
#pragma clang loop unroll(disable)
  for (int w = 0; w < 2; w++) {
    const MatOp* prog = w ? MAT_DEC : MAT_ENC;
    const int n = w ? MAT_DEC_N : MAT_ENC_N;
    int off = w ? dec : 0;
#pragma clang loop unroll(disable)
    for (int i = 0; i < n; i++) {
      const MatOp op = prog[i];
      const float* src = matg_slot(m, op.src, E, false);
      float* dst = matg_slot(m, op.dst, E, false);
      if (op.kind == MAT_LIN) {
        const int K = mat_width(op.kin, D, E), Nout = mat_width(op.nout, D, E);
        const int at = matg_lin_at(op, off, tail, E);
        const float* W = params + at;
        const float* b = W + (size_t)K * Nout;
        if (matg_keeps_x(prog, n, i)) matg_push(tape, tp, src, K, tid);
        if (((K | at) & 3) == 0) actor_layer<true>(W, b, K, Nout, src, dst, lane, wave, 0);      // mat_run's alignment test
        else actor_layer<false>(W, b, K, Nout, src, dst, lane, wave, 0);
        if (op.post == MAT_GELU) {
          matg_gelu(dst, tape + (size_t)tp * ACT_ROWS, Nout, lane, wave);
          tp += Nout;
        } else if (op.post == MAT_RES) mat_post(dst, matg_slot(m, op.res, E, false), Nout, MAT_RES, lane, wave);
        __syncthreads();
      } else if (op.kind == MAT_LN) {
        const int wd = mat_width(op.kin, D, E);
        const float* g = params + off;
        matg_push(tape, tp, src, wd, tid);
        ln_rows<ACT_LD>(src, dst, wd, g, g + wd, inv[op.kin == MAT_WD ? 0 : 1], m.part, m.stat, lane, wave);
        matg_push(tape, tp, m.stat, 2, tid);
      } else {
        const float* k = matg_slot(m, op.kin, E, false);
        const float* v = matg_slot(m, op.nout, E, false);
        matg_push(tape, tp, src, E, tid);
        matg_push(tape, tp, k, E, tid);
        matg_push(tape, tp, v, E, tid);
        mat_attend(src, k, v, dst, E, Aw, op.post != 0, inv[2], lane, wave);
        __syncthreads();
      }
      off += mat_op_floats(op, D, E);
    }
  }
  return tp;
}

// the reverse walk: out[0 .. 2] and out[3] hold the deltas of mean and value; pg: the workgroup's partial gradient
__device__ __forceinline__ void matg_backward(const float* __restrict__ params, float* __restrict__ pg, int dec, int tail, int D, int E, int Aw, const float* inv,
                                              const MatgLds& m, const float* tape, int tp, bool first, int lane, int wave, int tid) {
  unsigned live = (1u << MAT_OUT) | (1u << MAT_OUTV);
#pragma clang loop unroll(disable)
  for (int w = 1; w >= 0; w--) {
    const MatOp* prog = w ? MAT_DEC : MAT_ENC;
    const int n = w ? MAT_DEC_N : MAT_ENC_N;
    int off = w ? dec + mat_dec_floats(E) : mat_enc_floats(D, E);
#pragma clang loop unroll(disable)
    for (int i = n - 1; i >= 0; i--) {
      const MatOp op = prog[i];
      // what derives from the thread index is formed again in front of every operator (kernels_actor_critic.hpp, BPTT_FRESH): held across the walk, the
      // phases' LDS addresses stay in registers and the kernel spills
      asm volatile("" : "+v"(tid));
      lane = tid & 63;
      off -= mat_op_floats(op, D, E);
      float* dY = matg_slot(m, op.dst, E, true);
      if (op.kind == MAT_LIN) {
        const int K = mat_width(op.kin, D, E), Nout = mat_width(op.nout, D, E);
        const int at = matg_lin_at(op, off, tail, E);
        if (op.post == MAT_GELU) {
          tp -= Nout;
          matg_gelu_back(dY, tape + (size_t)tp * ACT_ROWS, Nout, lane, wave);
          __syncthreads();
        } else if (op.post == MAT_RES) {
          matg_meet(matg_slot(m, op.res, E, true), dY, Nout, (live >> op.res) & 1u, tid);
          live |= 1u << op.res;
        }
        const float* x = m.S;
        if (op.src != MAT_S) {
          x = m.T;
          if (matg_keeps_x(prog, n, i)) matg_pop(tape, tp, m.T, K, tid);      // otherwise the Linear walked just before left it there
        }
        __syncthreads();
        ppo_dw<ACT_LD, ACT_ROWS>(dY, x, K, Nout, pg + at, pg + at + (size_t)K * Nout, first, tid);
        if (op.src != MAT_S) {                       // nothing lies below s
          const bool add = (live >> op.src) & 1u;
          float* to = add ? m.X : matg_slot(m, op.src, E, true);
          ppo_dx<ACT_LD, true>(params + at, K, Nout, dY, to, lane, wave, 0);
          if (add) {
            __syncthreads();
            matg_meet(matg_slot(m, op.src, E, true), m.X, K, true, tid);
          }
          live |= 1u << op.src;
        }
        live &= ~(1u << op.dst);
        __syncthreads();
      } else if (op.kind == MAT_LN) {
        const int wd = mat_width(op.kin, D, E);
        const float* g = params + off;
        matg_pop(tape, tp, m.T, wd + 2, tid);        // a, then (mu, rstd)
        __syncthreads();
        const float* st = m.T + (size_t)wd * ACT_LD;
        if (op.src == MAT_O) {                       // obs_norm: dgamma and dbeta alone
          ln_back<ACT_LD, ACT_ROWS, 0>(m.T, dY, wd, g, inv[0], st, m.part, pg + off, pg + off + wd, first, 0, lane, lane, wave);
        } else {
          ln_back<ACT_LD, ACT_ROWS, 2>(m.T, dY, wd, g, inv[1], st, m.part, pg + off, pg + off + wd, first, 0, lane, lane, wave);
          live &= ~(1u << op.dst);
          matg_meet(matg_slot(m, op.src, E, true), m.T, wd, (live >> op.src) & 1u, tid);
          live |= 1u << op.src;
          __syncthreads();
        }
      } else {
        float* q = matg_slot(m, op.src, E, true);
        float* k = matg_slot(m, op.kin, E, true);
        float* v = matg_slot(m, op.nout, E, true);
        matg_pop(tape, tp, v, E, tid);
        matg_pop(tape, tp, k, E, tid);
        matg_pop(tape, tp, q, E, tid);
        __syncthreads();
        matg_attend_back(q, k, v, dY, m.part, E, Aw, op.post != 0, inv[2], lane, wave);
        live = (live & ~(1u << op.dst)) | (1u << op.src) | (1u << op.kin) | (1u << op.nout);
      }
    }
  }
}

// wavefront 0, behind the heads of a tile: ppo_store_sums' butterfly (32, 16, ..., 1) over the tile's seven sums, then lane 0 continues the workgroup's slot
// (f64, tiles in the workgroup's order; the first tile stores)
__device__ __forceinline__ void matg_add_sums(const PpoSums& S, int lane, double* __restrict__ pst, bool first) {
  double v[7] = {S.Lpi, S.Lv, S.Kl, S.Clip, S.gls[0], S.gls[1], S.gls[2]};
#pragma unroll
  for (int q = 0; q < 7; q++) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v[q] += __shfl_xor(v[q], m);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 7; q++) pst[q] = first ? v[q] : pst[q] + v[q];
  }
}

// ---- k_mat_grad -----------------------------------------------------------------------------------------------------------------------------------------
// tr: the minibatch as the flat list k_joint_expand wrote (count = M samples, group-major).  tape_all: PPO_MAX_WG tapes of tape_rows rows
extern "C" __global__ void __launch_bounds__(ACT_THREADS) k_mat_grad(const float* __restrict__ params, const ActorShapes* __restrict__ sh, PpoTraj tr, int log_std_off,
                                                                     int n_params, int D, int Aw, int tape_rows, float* __restrict__ part_all, double* __restrict__ pst,
                                                                     PpoLoss ls, float* tape_all) {
  extern __shared__ __attribute__((aligned(16))) unsigned char matg_lds[];
  long long* srow = reinterpret_cast<long long*>(matg_lds);
  float* eff = reinterpret_cast<float*>(matg_lds + 64 * 8);      // l_j = ln sigma_j
  float* rows = reinterpret_cast<float*>(matg_lds + MATG_HEAD_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int E = sh->actor.dims[1];
  MatgLds m;
  m.T = rows;
  m.G = m.T + (size_t)(MATG_MAX(D, E) + 2) * ACT_LD;
  m.X = m.G + (size_t)MATG_MAX(MAT_SLABS * E, E + D) * ACT_LD;
  m.stat = m.X + (size_t)E * ACT_LD;
  m.S = m.stat + 2 * ACT_LD;
  m.out = m.S + 3 * ACT_LD;
  m.part = m.out + 4 * ACT_LD;
  const int dec = mat_enc_floats(D, E), tail = dec + mat_dec_floats(E);
  float* pg = part_all + (size_t)blockIdx.x * n_params;
  float* tape = tape_all + (size_t)blockIdx.x * tape_rows * ACT_ROWS;
  if (tid < 3) eff[tid] = logf(0.5f * gru_sigmoid(params[log_std_off + tid]));
  const long long tiles = (tr.count + ACT_ROWS - 1) / ACT_ROWS;
  double* wg_pst = pst + (size_t)blockIdx.x * PPO_PST;
  bool first_tile = true;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // the tile's samples (past the end of the minibatch the last GROUP again), their observations and s
    if (tid < ACT_ROWS) {
      long long i = tile * ACT_ROWS + tid;
      if (i > tr.count - 1) i = tr.count - Aw + (tid & (Aw - 1));
      srow[tid] = ppo_unit(tr.index, tr.first, i, tr.n_total);
    }
    __syncthreads();
    for (int e = tid; e < ACT_ROWS * D; e += ACT_THREADS) {
      const int r = e / D, k = e - r * D;
      const long long s = srow[r];
      const long long t = s / tr.rows, rr = s - t * tr.rows;
      m.T[k * ACT_LD + r] = tr.packed[(size_t)t * (size_t)tr.stride + (size_t)rr * D + k];
    }
    for (int e = tid; e < 3 * ACT_ROWS; e += ACT_THREADS) {
      const int j = e >> 6, r = e & 63;
      m.S[j * ACT_LD + r] = (r & (Aw - 1)) ? tr.actions[(size_t)srow[r - 1] * 3 + j] : 0.0f;      // s_0 = 0, s_a = the action of agent a - 1: the row before
    }
    __syncthreads();
    const int tp = matg_forward(params, dec, tail, D, E, Aw, sh->inv_actor, m, tape, lane, wave, tid);
    if (wave == 0) {
      const bool valid = tile * ACT_ROWS + lane < tr.count;
      PpoSums S;                                     // of this tile; added to the workgroup's slot behind the heads, so that no sum is held across the walk
      ppo_actor_head<ACT_LD, ACT_ROWS>(eff, 0, m.out, srow, lane, lane, valid, tr.actions, tr.logp_old, tr.adv, ls, S);
      ppo_critic_head<ACT_LD, ACT_ROWS>(m.out, srow, lane, lane, valid, tr.value, tr.ret, ls, S);
      matg_add_sums(S, lane, wg_pst, first_tile);
    }
    __syncthreads();
    matg_backward(params, pg, dec, tail, D, E, Aw, sh->inv_actor, m, tape, tp, first_tile, lane, wave, tid);
    first_tile = false;
  }
}

// k_ppo_reduce with MAT's head: the three sums are dL/dl_j, l_j = ln sigma_j;  dl_j / dlog_std_j = 1 - sigmoid(log_std_j);  H = sum_j l_j + 1.5 (1 + ln(2 pi))
__global__ void __launch_bounds__(PPO_REDUCE_THREADS) k_mat_reduce(const float* __restrict__ part, const double* __restrict__ pst, int G, int n_params, int log_std_off,
                                                                   long long M, float value_coef, float entropy_coef, const float* __restrict__ params,
                                                                   float* __restrict__ grad, float* __restrict__ stats) {
  const int i = blockIdx.x * PPO_REDUCE_THREADS + threadIdx.x;
  if (i < log_std_off) {
    double a = 0.0;
    for (int b = 0; b < G; b++) a += (double)part[(size_t)b * n_params + i];
    grad[i] = (float)a;
  } else if (i < n_params) {
    double a = 0.0;
    for (int b = 0; b < G; b++) a += pst[(size_t)b * PPO_PST + 4 + (i - log_std_off)];
    const double sg = 1.0 / (1.0 + exp(-(double)params[i]));
    grad[i] = (float)((a - (double)entropy_coef) * (1.0 - sg));
  }
  if (i == 0 && stats != nullptr) {
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < G; b++)
      for (int q = 0; q < 4; q++) S[q] += pst[(size_t)b * PPO_PST + q];
    const double n = (double)M;
    double H = 1.5 * (1.0 + 1.8378770664093453);        // ln(2 pi)
    for (int j = 0; j < 3; j++) H += log(0.5 / (1.0 + exp(-(double)params[log_std_off + j])));
    const double Lpi = S[0] / n, Lv = S[1] / n;
    stats[0] = (float)Lpi;
    stats[1] = (float)Lv;
    stats[2] = (float)H;
    stats[3] = (float)(Lpi + (double)value_coef * Lv - (double)entropy_coef * H);
    stats[4] = (float)(S[2] / n);
    stats[5] = (float)(S[3] / n);
  }
}
