// kernels_vn.hpp -- k_vn_denorm / k_vn_moments / k_vn_apply: value normalisation (OpenRL / MAPPO ValueNorm) for the engine's critic: running,
// debiased statistics of the returns, kept as five floats behind log_std in the actor's parameter buffer (MQE_ACTOR_VALUE_NORM, MQE_GAE_VALUE_NORM,
// MQE_PPO_VALUE_NORM, MQE_PPO_VALUE_NORM_UPDATE; include/mqe_hip.h).  The critic predicts returns in units of (mu, sigma); k_gae, k_ppo_grad and
// k_actor are untouched: they read what these kernels wrote into engine-owned scratch.
//
// ARITHMETIC.  State w = (m, q, d, mu, sigma), all f32: running mean, running mean of squares, debiasing term, and the derived pair every consumer
// reads.  beta = 0.99999f widened to double, 1 - beta formed in f64; eps = 1e-5f; var_min = 1e-2f.
//   derived pair, a pure function of the STORED f32 (m, q, d), evaluated in f64 and rounded once each:
//     dc = max(d, eps);  mu = (float)(m / dc);  sigma = (float)sqrt(max(q / dc - (m / dc)^2, var_min))
//   (0, 0, 0) gives (0, 0.1f): sigma is never zero.
//   update over a minibatch of M returns x_i -- the samples the gradient kernel reads (THE SELECTION of kernels_ppo.hpp, ppo_unit):
//     S1 = sum x_i;  S2 = sum x_i^2 (f64 fma);  bm = S1 / M;  bq = S2 / M
//     m' = (float)(beta m + (1 - beta) bm);  q' = (float)(beta q + (1 - beta) bq);  d' = (float)(beta d + (1 - beta))
//   then the derived pair from the rounded (m', q', d').
//   de-normalise a critic output: fmaf(v, sigma, mu).   normalise a return: (float)(((double)x - mu) * (1.0 / (double)sigma)), with the stored f32
//   (mu, sigma) -- k_gae_normalize's pattern: the build's f32 division is the 2.5-ulp sequence and is not used.
// SUMMATION ORDER.  k_vn_moments: thread j of workgroup b adds samples i = b 256 + j, + G 256, ... in that order (f64); the 64 lanes of a wavefront
// by the xor butterfly 32, 16, 8, 4, 2, 1; the four wavefronts as (w0 + w1) + (w2 + w3) through LDS; workgroup b stores its pair at part[2 b].
// k_vn_apply adds the G pairs in index order (every workgroup copies them into LDS with one parallel load first; every thread then adds them).  G = min(VN_MAX_WG, ceil(M / 2048)) depends on M alone.  No floating-point atomics, no tickets, no
// spin waits: the same bits on every run.  f32 state inherits ValueNorm's cancellation limit: q / dc - mu^2 loses digits once mu^2 >> var.
//
// THE HAZARD.  Every workgroup of k_vn_apply needs the NEW (mu, sigma) while one of them stores the new state over the old.  So k_vn_moments also
// copies the old (m, q, d) behind the pairs (part[2 VN_MAX_WG ..]), and every workgroup of k_vn_apply derives the new state from that snapshot
// and the pairs -- redundantly, identically, never reading the state -- while workgroup 0 alone stores it.  Without an update k_vn_apply reads
// (mu, sigma) from the state and nothing writes it.
//
// LAYOUT.  256-thread workgroups.  The gather ret[index[i]] is 4-byte random reads over at most a few MB (L2 / Infinity Cache); a 409 600-sample
// minibatch is 128 workgroups x 12.5 loads per thread, not one serial chain, and a thread issues its loads in batches of VN_PER = 8 (index, then
// return) before it consumes them in order: a batch costs two memory round trips, not sixteen.  A batch that reaches past the minibatch loads its
// last sample again and skips it.  k_vn_apply writes each target at its own sample position (a duplicated index stores the same value twice).
// No scratch memory; static LDS: 64 bytes in k_vn_moments, 2 KiB (the pairs) in k_vn_apply.
#pragma once
#include "mqe_common.hpp"
#include "kernels_ppo.hpp"

// the constants of the value-normalisation section of include/mqe_hip.h: stated there in words, defined here (the header's ACTOR / GAE / PPO define
// sets are pinned by the tests), mirrored in mqe/engine/abi.py; tests/test_value_norm.py compares the three
#define MQE_ACTOR_VALUE_NORM 256          // mqe_actor_shape.activation, above the kind byte
#define MQE_VALUE_NORM_STATE 5            // floats behind log_std: m, q, d, mu, sigma
#define MQE_GAE_VALUE_NORM 8              // mqe_gae flags
#define MQE_PPO_VALUE_NORM 8              // mqe_ppo_grad flags
#define MQE_PPO_VALUE_NORM_UPDATE 16      // mqe_ppo_grad flags; needs MQE_PPO_VALUE_NORM

#define VN_THREADS 256
#define VN_PER 8                   // samples per thread the grids are sized for
#define VN_MAX_WG 128              // workgroups of k_vn_moments at most = pairs k_vn_apply adds
static_assert(2 * VN_MAX_WG <= VN_THREADS, "k_vn_apply copies the pairs into LDS with one load per thread");
#define VN_PART (2 * VN_MAX_WG + 4)      // doubles of the partials' scratch: the pairs, then the snapshot (m, q, d), pad
#define VN_BETA 0.99999f
#define VN_EPS 1e-5f
#define VN_VAR_MIN 1e-2f

// the derived pair of the stored triple (host: mqe_actor_create; device: k_vn_apply)
__host__ __device__ inline void vn_derive(float m, float q, float d, float* mu, float* sigma) {
  const double dc = (double)(d > VN_EPS ? d : VN_EPS);
  const double mean = (double)m / dc;
  const double var = (double)q / dc - mean * mean;
  *mu = (float)mean;
  *sigma = (float)sqrt(var > (double)VN_VAR_MIN ? var : (double)VN_VAR_MIN);
}

// out[i] = fmaf(v[i], sigma, mu), i < n = (T + 1) R'
__global__ void __launch_bounds__(VN_THREADS) k_vn_denorm(const float* __restrict__ v, const float* __restrict__ state, float* __restrict__ out, long long n) {
  const float mu = state[3], sigma = state[4];
  for (long long i = (long long)blockIdx.x * VN_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * VN_THREADS) out[i] = fmaf(v[i], sigma, mu);
}

// part[2 b], part[2 b + 1] = workgroup b's (sum x, sum x^2); workgroup 0 also copies the old (m, q, d) to part[2 VN_MAX_WG ..]
__global__ void __launch_bounds__(VN_THREADS) k_vn_moments(const float* __restrict__ ret, const int32_t* __restrict__ index, long long first, long long count,
                                                           long long n_total, const float* __restrict__ state, double* __restrict__ part) {
  __shared__ double red[2 * (VN_THREADS / 64)];
  double s1 = 0.0, s2 = 0.0;
  const long long stride = (long long)gridDim.x * VN_THREADS;
  for (long long i0 = (long long)blockIdx.x * VN_THREADS + threadIdx.x; i0 < count; i0 += VN_PER * stride) {
    long long smp[VN_PER];
    float x[VN_PER];
#pragma unroll
    for (int j = 0; j < VN_PER; j++) {
      const long long i = i0 + j * stride;
      smp[j] = ppo_unit(index, first, i < count ? i : count - 1, n_total);
    }
#pragma unroll
    for (int j = 0; j < VN_PER; j++) x[j] = ret[smp[j]];
#pragma unroll
    for (int j = 0; j < VN_PER; j++)
      if (i0 + j * stride < count) {
        s1 += (double)x[j];
        s2 = fma((double)x[j], (double)x[j], s2);
      }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    s1 += __shfl_xor(s1, m);
    s2 += __shfl_xor(s2, m);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[2 * wave] = s1;
    red[2 * wave + 1] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = (red[0] + red[2]) + (red[4] + red[6]);
    part[2 * (size_t)blockIdx.x + 1] = (red[1] + red[3]) + (red[5] + red[7]);
    if (blockIdx.x == 0) {
      part[2 * VN_MAX_WG] = (double)state[0];
      part[2 * VN_MAX_WG + 1] = (double)state[1];
      part[2 * VN_MAX_WG + 2] = (double)state[2];
    }
  }
}

// out[s] = the normalised ret[s] for the minibatch's samples s.  part != nullptr (an updating call): the new state from k_vn_moments' nparts pairs
// and snapshot, stored by workgroup 0; nullptr: (mu, sigma) as the state holds them
__global__ void __launch_bounds__(VN_THREADS) k_vn_apply(const float* __restrict__ ret, const int32_t* __restrict__ index, long long first, long long count,
                                                         long long n_total, float* state, const double* __restrict__ part, int nparts,
                                                         float* __restrict__ out) {
  __shared__ double pairs[2 * VN_MAX_WG];
  float mu, sigma;
  if (part != nullptr) {               // uniform
    if ((int)threadIdx.x < 2 * nparts) pairs[threadIdx.x] = part[threadIdx.x];      // 2 nparts <= 2 VN_MAX_WG = VN_THREADS
    __syncthreads();
    double S1 = 0.0, S2 = 0.0;
    for (int b = 0; b < nparts; b++) {
      S1 += pairs[2 * b];
      S2 += pairs[2 * b + 1];
    }
    const double beta = (double)VN_BETA, omb = 1.0 - beta, M = (double)count;
    const float m = (float)(beta * part[2 * VN_MAX_WG] + omb * (S1 / M));
    const float q = (float)(beta * part[2 * VN_MAX_WG + 1] + omb * (S2 / M));
    const float d = (float)(beta * part[2 * VN_MAX_WG + 2] + omb);
    vn_derive(m, q, d, &mu, &sigma);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      state[0] = m;
      state[1] = q;
      state[2] = d;
      state[3] = mu;
      state[4] = sigma;
    }
  } else {
    mu = state[3];
    sigma = state[4];
  }
  const double dmu = (double)mu, inv = 1.0 / (double)sigma;
  const long long stride = (long long)gridDim.x * VN_THREADS;
  for (long long i0 = (long long)blockIdx.x * VN_THREADS + threadIdx.x; i0 < count; i0 += VN_PER * stride) {
    long long smp[VN_PER];
    float x[VN_PER];
#pragma unroll
    for (int j = 0; j < VN_PER; j++) {
      const long long i = i0 + j * stride;
      smp[j] = ppo_unit(index, first, i < count ? i : count - 1, n_total);
    }
#pragma unroll
    for (int j = 0; j < VN_PER; j++) x[j] = ret[smp[j]];
#pragma unroll
    for (int j = 0; j < VN_PER; j++)
      if (i0 + j * stride < count) out[smp[j]] = (float)(((double)x[j] - dmu) * inv);
  }
}
