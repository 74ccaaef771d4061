// kernels_mat.hpp -- the Multi-Agent Transformer policy of an on-device rollout (MQE_ACTOR_TRANSFORMER; include/mqe_hip.h): the network as a
// program of three operators, its constants, its parameter order and its LDS rule, and the rollout kernel k_actor_mat.  A handle created
// without the bit never launches it.  The gradient through the attention is kernels_mat_grad.hpp's (k_mat_grad), asked for with MQE_PPO_TRANSFORMER;
// without that flag mqe_ppo_grad refuses such a handle, and a learner differentiates the torch twin (mqe.utils.actor_net.MATNet.evaluate).
//
// THE NETWORK is MAT as published (ma_transformer.py, continuous actions) at n_block = 1, n_head = 1, dec_actor = False; E = n_embd, D = the
// observation width, A' = the agents of an env.  LN = LayerNorm(eps = 1e-5) with weight and bias (kernels_ln.hpp: ln_rows, unchanged);
// every Linear has a bias and is actor_layer's chain (kernels_actor.hpp):  acc = b[o];  k ascending:  acc = fmaf(W[o][k], x[k], acc).
//     Attn(key, value, query; masked):  k = Wk key + bk, v = Wv value + bv, q = Wq query + bq;  out = Wp y + bp, with per row i of a group
//         s_j = 0;  k ascending:  s_j = fmaf(q_i[k], k_j[k], s_j);   s_j = s_j * c,  c = (float)(1.0 / sqrt((double)E)) formed on the host
//         J = {0 .. A' - 1}, masked: {0 .. i};   m = max over J of s_j;   e_j = expf(s_j - m);   z = e_0 + e_1 + ... (j ascending over J)
//         p_j = e_j / z;   y[n] = 0;  j ascending over J:  y[n] = fmaf(p_j, v_j[n], y[n])
//       an index outside J is EXCLUDED BY SELECT: it enters neither the maximum, nor the sum, nor y, and no infinity is ever formed.
//     Encoder  x = LN_E(GELU(Linear_{D->E}(LN_D(obs))));  x = LN_E(x + Attn(x, x, x; unmasked));  rep = LN_E(x + Linear(GELU(Linear(x))))
//              value = Linear_{E->1}(LN_E(GELU(Linear_{E->E}(rep))))
//     Decoder  s_0 = 0, s_a = the raw action of agent a - 1;  x = LN_E(GELU(Linear_{3->E}(s)));  x = LN_E(x + Attn(x, x, x; masked))
//              x = LN_E(rep + Attn(key = x, value = x, query = rep; masked));  x = LN_E(x + Linear(GELU(Linear(x))))
//              mean = Linear_{E->3}(LN_E(GELU(Linear_{E->E}(x))))
//     GELU(x)   = 0.5f * x * (1.0f + erff(x * 0.70710678f))           the exact erf form; a residual sum is one f32 addition x + out
//     sigma_j   = 0.5f * (1.0f / (1.0f + expf(-log_std_j)))           MAT's 0.5 sigmoid(log_std), NOT exp(log_std)
//     a_j       = fmaf(sigma_j, z_j, mean_j);   logp = sum over j ascending, from 0, of (-0.5 z_j^2 - logf(sigma_j)), - 1.5 ln(2 pi)
//   z_j is k_actor's draw, mqe_randn_key(seed, GLOBAL env id, MQE_RNG_ACTOR + n, agent * 3 + j); deterministic: z = 0.
//
// THE PROGRAM.  The walk is data: MAT_ENC and MAT_DEC below list the operators in the order they run -- a Linear (with GELU or a residual sum
// applied by the thread that wrote the element), a norm, an attention -- with the LDS slabs they read and write.  One interpreter loop
// (mat_run) executes them, so the kernel holds ONE copy of actor_layer (per alignment), of ln_rows and of the attention instead of thirty.
// PARAMETERS follow the program: every Linear is weight (out, in) row-major then bias, every norm weight then bias, in the order the operators
// run, encoder then decoder -- except the two narrow output layers, which come last: value_out (E -> 1), mean_out (E -> 3), then log_std.
// Behind an odd-sized tensor every later offset would leave the 16-byte grid and all E x E matrices would fall back to dword scalar loads;
// with E % 4 == 0 and an even D every one of them is read with 16-byte loads.  mat_enc_floats / mat_dec_floats are the closed counts.
//
// LAYOUT: k_actor's.  1024 threads = 16 wavefronts own 64 consecutive rows, LANE = ROW, activations in LDS as [k][row] with stride 65, weights
// wave-uniform through scalar loads (the parameter buffer and the shapes are `const ... * __restrict__` kernel arguments: kernels_gru.hpp, SCALAR
// WEIGHT LOADS).  A GROUP is the A' aligned rows of one env; A' divides 64, so a tile holds 64 / A' whole envs and no group straddles two tiles.
// ATTENTION.  Every wavefront forms all A' scores of its lane's row: the row's own q column and the group's k columns in LDS (lanes of a group
// read the same word: a broadcast; groups read consecutive banks), the chain above -- the same bits in all 16 wavefronts, no exchange.  The
// softmax stays in registers.  y is split over the wavefronts by feature, n = wave, wave + 16, ...  No cross-lane operation, no atomics.
// THE DECODER LOOP.  Acting is autoregressive: the decoder program runs A' times over ALL rows; behind pass a wavefront 0 draws for the rows
// whose agent is a, keeps their action and writes it into the NEXT row's column of s (slab S) as s_{a + 1}.  EVALUATION ORDER: everything a row
// computes is a function of its own lane's values and of its group's k / v columns at j <= i (masked attention, exclusion by select); at pass a
// those are final for row a, and later passes recompute them from the same inputs in the same order.  So row a's mean behind pass a has exactly
// the bits of one parallel pass over the final s -- what a learner's MATNet.evaluate restates.
// All global stores come behind the last pass, from wavefront 0, out of LDS.
//
// LDS RULE (actor_mat_lds_bytes, the one statement; mqe_actor_create refuses above MAT_LDS_LIMIT):  D rows of the observation, MAT_SLABS = 6 slabs
// of E rows (x, q, k, v, y and rep), 3 rows of s, 4 output rows (mean 0 .. 2, value), 4 rows of kept results (action 0 .. 2, logp) and the norm's
// 32 partial rows, each 65 floats.  E = 64, D = 128: 555 rows = 140.9 KiB.
#pragma once
#include "mqe_common.hpp"
#include "kernels_actor.hpp"
#include "kernels_ln.hpp"
#include "kernels_gru.hpp"

// the constant of the transformer section of include/mqe_hip.h: stated there in words, defined here (the header's ACTOR define set is pinned by
// the tests), mirrored in mqe/engine/abi.py; tests/test_mat.py compares the three
#define MQE_ACTOR_TRANSFORMER 32          // bit of the kind byte of mqe_actor_shape.activation: the two "networks" are MAT's encoder and decoder

#define MAT_LDS_LIMIT (160 * 1024)        // the LDS of a workgroup
#define MAT_SLABS 6                       // E-row slabs: B0 .. B4 and rep
#define MAT_FIXED_ROWS (3 + 4 + 4 + LN_PART)      // s, the output rows, the kept results, the norm's partials

static inline size_t actor_mat_lds_bytes(int D, int E) { return (size_t)(D + MAT_SLABS * E + MAT_FIXED_ROWS) * ACT_LD * sizeof(float); }
// floats of the encoder and of the decoder without their output layers, which follow both: value_out (E + 1), mean_out (3 E + 3), log_std (3)
__host__ __device__ inline int mat_enc_floats(int D, int E) { return 2 * D + D * E + 7 * E * E + 16 * E; }
__host__ __device__ inline int mat_dec_floats(int E) { return 11 * E * E + 25 * E; }
__host__ __device__ inline int mat_param_floats(int D, int E) { return mat_enc_floats(D, E) + mat_dec_floats(E) + (E + 1) + (3 * E + 3) + 3; }

enum { MAT_LIN, MAT_LN, MAT_ATT };                                                                      // operators
enum { MAT_O, MAT_B0, MAT_B1, MAT_B2, MAT_B3, MAT_B4, MAT_REP, MAT_S, MAT_OUT, MAT_OUTV };                // LDS slots
enum { MAT_WD, MAT_WE, MAT_W3, MAT_W1 };                                                                // widths: D, E, 3, 1
enum { MAT_PLAIN, MAT_GELU, MAT_RES };                                                                  // what follows a Linear
enum { MAT_RUNNING, MAT_VALUE_OUT, MAT_MEAN_OUT };                                                      // where a Linear's parameters are
// MAT_LIN: src -> dst, widths kin -> nout, post (MAT_RES: + slot res), where.  MAT_LN: src -> dst, width kin.  MAT_ATT: query src, key kin, value nout
// (slots) -> dst, post != 0: masked
struct MatOp { signed char kind, src, dst, kin, nout, post, res, where; };
#define MAT_ENC_OPS { \
  {MAT_LN, MAT_O, MAT_O, MAT_WD, 0, 0, 0, 0},                             /* obs_norm */ \
  {MAT_LIN, MAT_O, MAT_B0, MAT_WD, MAT_WE, MAT_GELU, 0, 0},               /* obs_fc */ \
  {MAT_LN, MAT_B0, MAT_B0, MAT_WE, 0, 0, 0, 0},                           /* ln */ \
  {MAT_LIN, MAT_B0, MAT_B2, MAT_WE, MAT_WE, MAT_PLAIN, 0, 0},             /* attn.key */ \
  {MAT_LIN, MAT_B0, MAT_B1, MAT_WE, MAT_WE, MAT_PLAIN, 0, 0},             /* attn.query */ \
  {MAT_LIN, MAT_B0, MAT_B3, MAT_WE, MAT_WE, MAT_PLAIN, 0, 0},             /* attn.value */ \
  {MAT_ATT, MAT_B1, MAT_B4, MAT_B2, MAT_B3, 0, 0, 0}, \
  {MAT_LIN, MAT_B4, MAT_B1, MAT_WE, MAT_WE, MAT_RES, MAT_B0, 0},          /* attn.proj */ \
  {MAT_LN, MAT_B1, MAT_B0, MAT_WE, 0, 0, 0, 0},                           /* ln1 */ \
  {MAT_LIN, MAT_B0, MAT_B1, MAT_WE, MAT_WE, MAT_GELU, 0, 0},              /* mlp0 */ \
  {MAT_LIN, MAT_B1, MAT_B2, MAT_WE, MAT_WE, MAT_RES, MAT_B0, 0},          /* mlp1 */ \
  {MAT_LN, MAT_B2, MAT_REP, MAT_WE, 0, 0, 0, 0},                          /* ln2 -> rep */ \
  {MAT_LIN, MAT_REP, MAT_B0, MAT_WE, MAT_WE, MAT_GELU, 0, 0},             /* head0 */ \
  {MAT_LN, MAT_B0, MAT_B0, MAT_WE, 0, 0, 0, 0},                           /* head_ln */ \
  {MAT_LIN, MAT_B0, MAT_OUTV, MAT_WE, MAT_W1, MAT_PLAIN, 0, MAT_VALUE_OUT}}
#define MAT_DEC_OPS { \
  {MAT_LIN, MAT_S, MAT_B0, MAT_W3, MAT_WE, MAT_GELU, 0, 0},               /* act_fc */ \
  {MAT_LN, MAT_B0, MAT_B0, MAT_WE, 0, 0, 0, 0},                           /* ln */ \
  {MAT_LIN, MAT_B0, MAT_B2, MAT_WE, MAT_WE, MAT_PLAIN, 0, 0},             /* attn1.key */ \
  {MAT_LIN, MAT_B0, MAT_B1, MAT_WE, MAT_WE, MAT_PLAIN, 0, 0},             /* attn1.query */ \
  {MAT_LIN, MAT_B0, MAT_B3, MAT_WE, MAT_WE, MAT_PLAIN, 0, 0},             /* attn1.value */ \
  {MAT_ATT, MAT_B1, MAT_B4, MAT_B2, MAT_B3, 1, 0, 0}, \
  {MAT_LIN, MAT_B4, MAT_B1, MAT_WE, MAT_WE, MAT_RES, MAT_B0, 0},          /* attn1.proj */ \
  {MAT_LN, MAT_B1, MAT_B0, MAT_WE, 0, 0, 0, 0},                           /* ln1 */ \
  {MAT_LIN, MAT_B0, MAT_B2, MAT_WE, MAT_WE, MAT_PLAIN, 0, 0},             /* attn2.key of x */ \
  {MAT_LIN, MAT_REP, MAT_B1, MAT_WE, MAT_WE, MAT_PLAIN, 0, 0},            /* attn2.query of rep */ \
  {MAT_LIN, MAT_B0, MAT_B3, MAT_WE, MAT_WE, MAT_PLAIN, 0, 0},             /* attn2.value of x */ \
  {MAT_ATT, MAT_B1, MAT_B4, MAT_B2, MAT_B3, 1, 0, 0}, \
  {MAT_LIN, MAT_B4, MAT_B1, MAT_WE, MAT_WE, MAT_RES, MAT_REP, 0},         /* attn2.proj */ \
  {MAT_LN, MAT_B1, MAT_B0, MAT_WE, 0, 0, 0, 0},                           /* ln2 */ \
  {MAT_LIN, MAT_B0, MAT_B1, MAT_WE, MAT_WE, MAT_GELU, 0, 0},              /* mlp0 */ \
  {MAT_LIN, MAT_B1, MAT_B2, MAT_WE, MAT_WE, MAT_RES, MAT_B0, 0},          /* mlp1 */ \
  {MAT_LN, MAT_B2, MAT_B0, MAT_WE, 0, 0, 0, 0},                           /* ln3 */ \
  {MAT_LIN, MAT_B0, MAT_B1, MAT_WE, MAT_WE, MAT_GELU, 0, 0},              /* head0 */ \
  {MAT_LN, MAT_B1, MAT_B1, MAT_WE, 0, 0, 0, 0},                           /* head_ln */ \
  {MAT_LIN, MAT_B1, MAT_OUT, MAT_WE, MAT_W3, MAT_PLAIN, 0, MAT_MEAN_OUT}}
#define MAT_ENC_N 15
#define MAT_DEC_N 20
// the one list, once for each side: the host walks it for the norm weights' offsets (mqe_actor_create), the kernel executes it
static const MatOp MAT_ENC_HOST[MAT_ENC_N] = MAT_ENC_OPS, MAT_DEC_HOST[MAT_DEC_N] = MAT_DEC_OPS;
static __device__ const MatOp MAT_ENC[MAT_ENC_N] = MAT_ENC_OPS, MAT_DEC[MAT_DEC_N] = MAT_DEC_OPS;

__host__ __device__ inline int mat_width(int code, int D, int E) { return code == MAT_WD ? D : code == MAT_WE ? E : code == MAT_W3 ? 3 : 1; }
// floats one operator takes from the running parameter offset
__host__ __device__ inline int mat_op_floats(const MatOp& op, int D, int E) {
  if (op.kind == MAT_LN) return 2 * mat_width(op.kin, D, E);
  if (op.kind == MAT_LIN && op.where == MAT_RUNNING) return (mat_width(op.kin, D, E) + 1) * mat_width(op.nout, D, E);
  return 0;
}

// the first LDS row of a slot: the observation, the six slabs, s, the output rows (the value is the fourth)
__device__ __forceinline__ float* mat_slot(float* lds, int slot, int D, int E) {
  const int row = slot == MAT_O ? 0 : slot <= MAT_REP ? D + (slot - MAT_B0) * E : D + MAT_SLABS * E + (slot == MAT_S ? 0 : slot == MAT_OUT ? 3 : 6);
  return lds + (size_t)row * ACT_LD;
}

__device__ __forceinline__ float mat_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678f)); }

// behind a Linear, by the thread that wrote the element (actor_layer's own split of the outputs: no barrier between): GELU, or the residual sum
__device__ __forceinline__ void mat_post(float* y, const float* res, int Nout, int post, int lane, int wave) {
  for (int o0 = wave * ACT_NB; o0 < Nout; o0 += ACT_WAVES * ACT_NB) {
#pragma unroll
    for (int j = 0; j < ACT_NB; j++) {
      if (o0 + j >= Nout) break;
      const int at = (o0 + j) * ACT_LD + lane;
      const float v = y[at];
      y[at] = post == MAT_GELU ? mat_gelu(v) : res[at] + v;
    }
  }
}

// one head of attention for the 64 rows of the workgroup: Q, K, V (LDS, [E][ACT_LD]) -> Y.  Aw is 1, 2 or 4; the lane's group is its Aw aligned rows
__device__ __forceinline__ void mat_attend(const float* Q, const float* K, const float* V, float* Y, int E, int Aw, bool masked, float scale, int lane, int wave) {
  const int i = lane & (Aw - 1), g0 = lane - i;
  const int last = masked ? i : Aw - 1;            // J = {0 .. last}
  float s[MQE_MAX_AGENTS] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
  for (int k = 0; k < E; k++) {
    const float q = Q[k * ACT_LD + lane];
#pragma unroll
    for (int j = 0; j < MQE_MAX_AGENTS; j++)
      if (j < Aw) s[j] = fmaf(q, K[k * ACT_LD + g0 + j], s[j]);
  }
  float m = s[0] * scale, e[MQE_MAX_AGENTS], z = 0.0f;
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
  for (int n = wave; n < E; n += ACT_WAVES) {
    float y = 0.0f;
#pragma unroll
    for (int j = 0; j < MQE_MAX_AGENTS; j++)
      if (j < Aw) {
        const float t = fmaf(e[j], V[n * ACT_LD + g0 + j], y);
        y = j <= last ? t : y;
      }
    Y[n * ACT_LD + lane] = y;
  }
}

// the interpreter: `n` operators of `prog` from parameter offset `off` on.  Every operator ends in a barrier (ln_rows in its own)
__device__ __forceinline__ void mat_run(const MatOp* prog, int n, const float* __restrict__ params, int off, int tail, int D, int E, int Aw,
                                        const float* inv, float* lds, float* part, int lane, int wave) {
#pragma clang loop unroll(disable)
  for (int i = 0; i < n; i++) {
    const MatOp op = prog[i];
    const float* src = mat_slot(lds, op.src, D, E);
    float* dst = mat_slot(lds, op.dst, D, E);
    if (op.kind == MAT_LIN) {
      const int K = mat_width(op.kin, D, E), Nout = mat_width(op.nout, D, E);
      const int at = op.where == MAT_RUNNING ? off : op.where == MAT_VALUE_OUT ? tail : tail + E + 1;
      const float* W = params + at;
      const float* b = W + (size_t)K * Nout;
      if (((K | at) & 3) == 0) actor_layer<true>(W, b, K, Nout, src, dst, lane, wave, 0);      // the ONE alignment test, as actor_layer_of's
      else actor_layer<false>(W, b, K, Nout, src, dst, lane, wave, 0);
      if (op.post != MAT_PLAIN) mat_post(dst, mat_slot(lds, op.res, D, E), Nout, op.post, lane, wave);
      __syncthreads();
    } else if (op.kind == MAT_LN) {
      const int w = mat_width(op.kin, D, E);
      const float* g = params + off;
      ln_rows<ACT_LD>(src, dst, w, g, g + w, inv[op.kin == MAT_WD ? 0 : 1], part, nullptr, lane, wave);
    } else {
      mat_attend(src, mat_slot(lds, op.kin, D, E), mat_slot(lds, op.nout, D, E), dst, E, Aw, op.post != 0, inv[2], lane, wave);
      __syncthreads();
    }
    off += mat_op_floats(op, D, E);
  }
}

// ---- k_actor_mat --------------------------------------------------------------------------------------------------------------------------------------
// k_actor's arguments in the recurrent kernels' form (the GruArgs are not read).  sh->actor.dims = {D, E, 3}; sh->inv_actor = {1 / D, 1 / E, c}
extern "C" __global__ void __launch_bounds__(ACT_THREADS) k_actor_mat(ActorArgs a, GruArgs, const float* __restrict__ params, const ActorShapes* __restrict__ sh) {
  extern __shared__ __attribute__((aligned(16))) float mat_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * ACT_ROWS, row = row0 + lane;
  const int D = a.D, E = sh->actor.dims[1], Aw = a.Aw;
  float* S = mat_slot(mat_lds, MAT_S, D, E);
  float* out = mat_slot(mat_lds, MAT_OUT, D, E);
  float* kept = out + 4 * ACT_LD;                          // [4][ACT_LD]: action 0 .. 2, logp
  float* part = kept + 4 * ACT_LD;                         // [LN_PART][ACT_LD]
  const bool sample = a.actions != nullptr;                // false: the value-only launch behind the last step
  const int dec = mat_enc_floats(D, E), tail = dec + mat_dec_floats(E);
  actor_load_obs(a.obs, row0, a.rows, D, mat_lds, tid);
  for (int e = tid; e < 3 * ACT_LD; e += ACT_THREADS) S[e] = 0.0f;      // s_0 = 0; the columns of later agents until they are published
  __syncthreads();
  mat_run(MAT_ENC, MAT_ENC_N, params, 0, tail, D, E, Aw, sh->inv_actor, mat_lds, part, lane, wave);
  if (sample) {
    // wavefront 0 holds the draw of its row across the passes: sigma, z and logp do not depend on the mean
    float sg[3] = {0.0f, 0.0f, 0.0f}, z[3] = {0.0f, 0.0f, 0.0f}, lp = 0.0f;
    const int ag = lane & (Aw - 1);
    if (wave == 0) {
      const int env = row / Aw;
#pragma unroll
      for (int j = 0; j < 3; j++) {
        sg[j] = 0.5f * gru_sigmoid(params[a.log_std_off + j]);
        z[j] = a.deterministic ? 0.0f : mqe_randn_key(a.seed, a.genv0 + (uint32_t)env, a.count, (uint32_t)(ag * 3 + j));
        lp += -0.5f * z[j] * z[j] - logf(sg[j]);
      }
      lp -= 3.0f * 0.9189385332046727f;       // 3 x 0.5 ln(2 pi)
    }
    for (int pass = 0; pass < Aw; pass++) {
      mat_run(MAT_DEC, MAT_DEC_N, params, dec, tail, D, E, Aw, sh->inv_actor, mat_lds, part, lane, wave);
      if (wave == 0 && ag == pass) {          // the rows whose agent is `pass`: their mean is final
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const float act = fmaf(sg[j], z[j], out[j * ACT_LD + lane]);
          kept[j * ACT_LD + lane] = act;
          if (pass + 1 < Aw) S[j * ACT_LD + lane + 1] = act;      // s_{a + 1}: the next row of the group, in this tile
        }
        kept[3 * ACT_LD + lane] = lp;
      }
      __syncthreads();
    }
  }
  // every global store of the kernel, behind the last weight load
  if (wave != 0 || row >= a.rows) return;
  if (sample) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const float act = kept[j * ACT_LD + lane];
      a.actions[(size_t)row * 3 + j] = act;
      a.stage[(size_t)row * 3 + j] = a.gain * act;
    }
    if (a.logp) a.logp[row] = kept[3 * ACT_LD + lane];
  }
  if (a.value) a.value[row] = out[3 * ACT_LD + lane];
}
