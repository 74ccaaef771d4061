// kernels_actor.hpp -- the primitives of the Gaussian actor (and optional critic) of an on-device rollout (mqe_rollout, include/mqe_hip.h): the
// shapes and the argument struct, one layer (actor_layer) and its dispatch by alignment (actor_layer_of), the observation load and the draw
// (actor_finish).  The network walk and the entry points k_actor / k_actor_ln are in kernels_actor_critic.hpp, behind the norm (kernels_ln.hpp).
// One launch per rollout step, in front of the five launches of the fused step; rows are R' = N x A' (env-major, the rows of
// MQE_T_WRAPPER_OBS).  Per row: the D task-observation floats -> actor MLP -> mean[3]; a = mean + exp(log_std) z with z from the
// engine's counter RNG; logp of the unclipped sample; critic MLP -> value.
//
// ARITHMETIC (all f32; a host twin can restate it): every pre-activation of every layer is
//     acc = b[o];  for k = 0, 1, ..., K - 1 (ascending):  acc = fmaf(W[o][k], x[k], acc)
// then tanhf(acc) or fmaxf(acc, 0) on hidden layers and nothing on the last.  z_j = mqe_randn_key(seed, GLOBAL env id,
// MQE_RNG_ACTOR + n, agent * 3 + j) (kernels_step.hpp: the one Box-Muller statement), n = the handle's count of post-physics steps when
// the launch is enqueued.  a_j = fmaf(expf(log_std_j), z_j, mean_j);  logp = sum over j ascending, from 0, of
// (-0.5 z_j^2 - log_std_j) - 0.5 ln(2 pi);  deterministic: z = 0.
//
// LAYOUT.  A workgroup is 1024 threads = 16 wavefronts and owns 64 consecutive rows: LANE = ROW in every wavefront, so no two rows of a
// wavefront ever take different paths (all control flow depends on the layer shapes and the wave index only; rows past R' are clamped
// on the load side and masked at the final stores).  The wavefronts split a layer's OUTPUT neurons in blocks of ACT_NB; activations
// live in LDS as [k][row] with a row stride of 65 floats, so a wavefront's read of x[k] and its write of y[o] hit 64 different banks
// and the coalesced observation load (consecutive lanes = consecutive k of one row) does too.
// WEIGHTS.  With lane = row a weight is the same for the whole wavefront: it is an SGPR operand of the FMA, fetched by scalar loads
// through the scalar data cache from L2 -- no LDS staging.  Every workgroup reads all <= 200 kB of them and they stay L2-resident (4 MB
// per XCD); staging them through LDS would cost a vector load, an LDS write and an LDS broadcast read per weight for a value that is
// used by ONE instruction of each wavefront.  What LDS bandwidth there is goes to the activations: one ds_read feeds ACT_NB FMAs.
// Rows of W whose start is 16-byte aligned (K % 4 == 0 and an aligned layer offset: 16 -> 64 -> 64 -> 3 and every power-of-two stack)
// are read in chunks of eight k with 16-byte scalar loads; the others in chunks of four k, a dword per load.  Same fmaf chain either way.
// WHY VALU AND NOT MFMA.  ~11 kFLOP per row for two 64 x 64 networks, 90 MFLOP = 45 M FMAs per launch at 8192 rows: at a CU's 128 f32 FMA
// lanes per clock that is ~150 us of ONE CU, about a microsecond spread over the 128 workgroups' CUs -- far below the 26 us measured
// (profiles/rollout.txt), so arithmetic throughput is not what the time goes to.  The matrix cores would force padded operand layouts on
// widths such as 7, 17 and 34 and a summation order a host twin cannot restate, for nothing.
// All global stores come after the last weight load, so the compiler keeps every weight load scalar.
#pragma once
#include "mqe_common.hpp"
#include "kernels_step.hpp"

#define ACT_ROWS 64        // rows per workgroup = lanes of a wavefront
#define ACT_THREADS 1024     // 16 wavefronts: 4 per SIMD, so that one wavefront's scalar-load latency is another's FMA time
#define ACT_WAVES (ACT_THREADS / 64)
#define ACT_NB 4           // output neurons a wavefront carries per pass over k
#define ACT_LD 65          // LDS row stride [k][row]: odd, so the transposing observation load is conflict-free too

struct ActorNet {
  int n_layers;                               // 0: no such network
  int dims[MQE_ACTOR_MAX_LAYERS + 1];         // in, hidden ..., out
  int w_off[MQE_ACTOR_MAX_LAYERS];            // offset of W[l] in the parameter buffer, floats; b[l] follows W[l]
};
// the shapes as the kernels read them (k_actor / k_actor_ln inside ActorArgs, k_ppo_grad / k_ln_grad from device memory: wave-uniform loads at the
// layer loops, words that need no registers).  The plain kernels read the two ActorNet only
struct ActorShapes {
  ActorNet actor, critic;
  float inv_actor[MQE_ACTOR_MAX_LAYERS], inv_critic[MQE_ACTOR_MAX_LAYERS];      // (float)(1.0 / dims[l]): the width of layer l's INPUT, the norms' 1 / n
  int hidden, feat;                                                             // MQE_ACTOR_LAYER_NORM / MQE_ACTOR_FEATURE_NORM (kernels_ln.hpp)
};
struct ActorArgs {
  const float* params;     // the flat parameter buffer (mqe_actor_params)
  const float* obs;        // [rows][D]
  float* actions;          // [rows][3] the unclipped sample (null: value-only launch)
  float* logp;             // [rows] or null
  float* value;            // [rows] or null
  float* stage;            // [rows][3] action_gain * a: what the following mqe_step reads
  ActorShapes sh;
  int log_std_off;
  int rows, D, Aw, ldh;    // ldh: widest activation vector (floats) = rows of one LDS buffer
  int relu, deterministic;
  float gain;
  uint32_t seed, genv0, count;     // RNG key: (seed, genv0 + env, count, agent * 3 + j)
};
static inline size_t actor_lds_bytes(int ldh) { return (size_t)(2 * ldh + 4) * ACT_LD * sizeof(float); }

// one layer for the 64 rows of the workgroup: x (LDS, [K][ACT_LD]) -> y (LDS, [Nout][ACT_LD]); W rows uniform per wavefront.
// The k loop runs in chunks: all scalar weight loads and LDS reads of a chunk are issued before the first FMA waits for them.
// LD: the LDS row stride (k_ppo_grad's 32-row tiles use 33; everything else ACT_LD).
template <bool VEC4, int LD = ACT_LD>
__device__ __forceinline__ void actor_layer(const float* __restrict__ W, const float* __restrict__ b, int K, int Nout, const float* x, float* y,
                                            int lane, int wave, int act) {
  for (int o0 = wave * ACT_NB; o0 < Nout; o0 += ACT_WAVES * ACT_NB) {
    const float* w[ACT_NB];
    float acc[ACT_NB];
#pragma unroll
    for (int j = 0; j < ACT_NB; j++) {
      const int o = min(o0 + j, Nout - 1);      // a short last block recomputes the last neuron and does not store it
      w[j] = W + (size_t)o * K;
      acc[j] = b[o];
    }
    int k = 0;
    if (VEC4) {
      for (; k + 8 <= K; k += 8) {
        float4 wa[ACT_NB], wb[ACT_NB];
        float xv[8];
#pragma unroll
        for (int j = 0; j < ACT_NB; j++) {
          wa[j] = *reinterpret_cast<const float4*>(__builtin_assume_aligned(w[j] + k, 16));
          wb[j] = *reinterpret_cast<const float4*>(__builtin_assume_aligned(w[j] + k + 4, 16));
        }
#pragma unroll
        for (int q = 0; q < 8; q++) xv[q] = x[(k + q) * LD + lane];
#pragma unroll
        for (int j = 0; j < ACT_NB; j++) {
          acc[j] = fmaf(wa[j].x, xv[0], acc[j]); acc[j] = fmaf(wa[j].y, xv[1], acc[j]);
          acc[j] = fmaf(wa[j].z, xv[2], acc[j]); acc[j] = fmaf(wa[j].w, xv[3], acc[j]);
          acc[j] = fmaf(wb[j].x, xv[4], acc[j]); acc[j] = fmaf(wb[j].y, xv[5], acc[j]);
          acc[j] = fmaf(wb[j].z, xv[6], acc[j]); acc[j] = fmaf(wb[j].w, xv[7], acc[j]);
        }
      }
    }
    for (; k + 4 <= K; k += 4) {
      float wv[ACT_NB][4], xv[4];
#pragma unroll
      for (int j = 0; j < ACT_NB; j++)
#pragma unroll
        for (int q = 0; q < 4; q++) wv[j][q] = w[j][k + q];
#pragma unroll
      for (int q = 0; q < 4; q++) xv[q] = x[(k + q) * LD + lane];
#pragma unroll
      for (int j = 0; j < ACT_NB; j++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[j] = fmaf(wv[j][q], xv[q], acc[j]);
    }
    for (; k < K; k++) {
      const float xk = x[k * LD + lane];
#pragma unroll
      for (int j = 0; j < ACT_NB; j++) acc[j] = fmaf(w[j][k], xk, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < ACT_NB; j++) {
      float v = acc[j];
      if (act == 1) v = tanhf(v);
      else if (act == 2) v = fmaxf(v, 0.0f);
      if (o0 + j < Nout) y[(o0 + j) * LD + lane] = v;
    }
  }
}

// layer l of a network: its weights by their offsets, no activation behind the last layer, and the ONE alignment test that picks the 16-byte loads
template <int LD>
__device__ __forceinline__ void actor_layer_of(const ActorNet& net, int l, const float* __restrict__ params, const float* x, float* dst, int lane, int wave,
                                               int hidden_act) {
  const int K = net.dims[l], Nout = net.dims[l + 1];
  const float* W = params + net.w_off[l];
  const float* b = W + (size_t)K * Nout;
  const bool last = l + 1 == net.n_layers;
  if (((K | net.w_off[l]) & 3) == 0) actor_layer<true, LD>(W, b, K, Nout, x, dst, lane, wave, last ? 0 : hidden_act);
  else actor_layer<false, LD>(W, b, K, Nout, x, dst, lane, wave, last ? 0 : hidden_act);
}

// the observation of the workgroup's 64 rows -> LDS [k][row]: coalesced (thread t reads float t of the 64 x D block), clamped at the end
__device__ __forceinline__ void actor_load_obs(const float* __restrict__ obs, int row0, int rows, int D, float* x, int tid) {
  const size_t last = (size_t)rows * D - 1;
  for (int e = tid; e < ACT_ROWS * D; e += ACT_THREADS) {
    const int r = e / D, k = e - r * D;
    const size_t g = (size_t)row0 * D + e;
    x[k * ACT_LD + r] = obs[g < last ? g : last];
  }
}

// wavefront 0, behind the networks: the draw, the log-probability and every global store of the kernel (behind the last weight load)
__device__ __forceinline__ void actor_finish(const ActorArgs& a, const float* out, bool sample, bool critic, int row0, int lane) {
  const int row = row0 + lane;
  float ls[3], act[3], lp = 0.0f;
  if (sample) {
    const int e = row / a.Aw, ag = row - e * a.Aw;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      ls[j] = a.params[a.log_std_off + j];
      const float z = a.deterministic ? 0.0f : mqe_randn_key(a.seed, a.genv0 + (uint32_t)e, a.count, (uint32_t)(ag * 3 + j));
      act[j] = fmaf(expf(ls[j]), z, out[j * ACT_LD + lane]);
      lp += -0.5f * z * z - ls[j];
    }
    lp -= 3.0f * 0.9189385332046727f;       // 3 x 0.5 ln(2 pi)
  }
  const float v = critic ? out[3 * ACT_LD + lane] : 0.0f;
  if (row >= a.rows) return;
  if (sample) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      a.actions[(size_t)row * 3 + j] = act[j];
      a.stage[(size_t)row * 3 + j] = a.gain * act[j];
    }
    if (a.logp) a.logp[row] = lp;
  }
  if (critic) a.value[row] = v;
}
