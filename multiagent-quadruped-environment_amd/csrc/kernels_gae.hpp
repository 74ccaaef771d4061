// kernels_gae.hpp -- k_gae / k_gae_normalize: GAE(lambda) advantages and returns of a trajectory in mqe_rollout's layout (mqe_gae,
// include/mqe_hip.h).  Rows are R' = N x A' (row r = env * A' + agent), the trajectory has T steps; value is [T + 1][R'].
//
// ARITHMETIC (all f32; a host twin can restate it).  Per row, t = T - 1, ..., 0 with adv = 0 in front and gl = gamma * lam (one f32
// product, made once); d = done[t][env], to = time_outs ? (time_outs[t][env] & d) : 0, v = value[t][r], vn = value[t + 1][r]:
//     rr    = to ? fmaf(gamma, v, reward[t][r]) : reward[t][r]
//     delta = (d ? rr : fmaf(gamma, vn, rr)) - v
//     adv   = d ? delta : fmaf(gl, adv, delta)
//     ret   = adv + v
// Selects, never products with a mask: a done step's vn and adv never enter the arithmetic.
// MQE_GAE_NORMALIZE (f64): every lane sums adv and adv * adv (fma) of its row in f64, t descending; the 64 lanes of a workgroup are added by
// the xor butterfly 32, 16, 8, 4, 2, 1; workgroup b stores its pair at part[2 b].  k_gae_normalize adds the pairs in index order:
// S = sum adv, Q = sum adv^2, n = T R';  mean = S / n;  std = sqrt(max((Q - S mean) / (n - 1), 0));  adv <- (float)((adv - mean) *
// (1 / (std + 1e-8f))) evaluated in f64 with the f64 mean and std, one rounding to f32 at the store.  No atomics: the same bits every run.
//
// LAYOUT.  One row per lane, 64-thread workgroups = one wavefront each (128 of them at 8192 rows, spread over the CUs).  Every load and
// store of a step is one coalesced line per array; the done / time-out bytes of a wavefront are 64 / A' consecutive bytes.  The recursion is
// serial in t, its loads are not: the t loop runs in batches of GAE_U = 8 steps whose 4 loads each are issued together, and the NEXT batch's
// loads are issued before the current batch's fmaf chain starts (register double buffer), so 16 steps = 64 loads per lane are in flight
// while 8 steps of arithmetic (4 dependent operations each) retire.  Depth 8 because the kernel is latency-bound with one wavefront per
// CU: a batch costs one memory round trip (~1-2 us) whatever its size, T = 200 is 25 round trips, and 2 x 8 x 4 data registers keep the
// kernel far from any occupancy limit; 16 would halve the trips for twice the registers with nothing else to buy at a cost already
// below a tenth of a percent of the rollout.  A batch that reaches below t = 0 loads step 0 again (clamped) and skips the arithmetic
// under a wavefront-uniform branch.  Lanes past R' load the last row and store nothing.  No LDS, no scratch.
#pragma once
#include "mqe_common.hpp"

#define GAE_THREADS 64       // one wavefront: lane = row
#define GAE_U 8              // steps per batch of loads
#define GAE_NORM_THREADS 256

struct GaeStep { float rew, v; uint32_t d, to; };

// rew_off: floats from the start of a packed row to its rewards (N A' D); the done bytes follow the R' rewards
template <bool TO>
__global__ void __launch_bounds__(GAE_THREADS) k_gae(const float* __restrict__ packed, long long stride, long long rew_off, const float* __restrict__ value,
                                                     const uint8_t* __restrict__ time_outs, float gamma, float lam, int T, int rows, int N, int Aw,
                                                     float* __restrict__ adv_out, float* __restrict__ ret_out, double* __restrict__ part) {
  const int row = blockIdx.x * GAE_THREADS + threadIdx.x;
  const bool live = row < rows;
  const int r = live ? row : rows - 1;
  const int e = r / Aw;
  const float gl = gamma * lam;
  const float* rew = packed + rew_off + r;                                                   // + (t + 1) * stride
  const uint8_t* done = reinterpret_cast<const uint8_t*>(packed + rew_off + rows) + e;      // + (t + 1) * stride * 4
  GaeStep cur[GAE_U], nxt[GAE_U];
#define GAE_LOAD(b, t_hi)                                                          \
  _Pragma("unroll") for (int j = 0; j < GAE_U; j++) {                              \
    const size_t t = (size_t)max((t_hi) - j, 0);                                   \
    b[j].rew = rew[(t + 1) * (size_t)stride];                                      \
    b[j].v = value[t * rows + r];                                                  \
    b[j].d = done[(t + 1) * (size_t)stride * 4];                                   \
    b[j].to = TO ? time_outs[t * N + e] : 0;                                       \
  }
  float vn = value[(size_t)T * rows + r];
  float adv = 0.0f;
  double s1 = 0.0, s2 = 0.0;
  GAE_LOAD(cur, T - 1)
  for (int th = T - 1; th >= 0; th -= GAE_U) {
    GAE_LOAD(nxt, th - GAE_U)
#pragma unroll
    for (int j = 0; j < GAE_U; j++) {
      const int t = th - j;
      if (t >= 0) {                      // uniform
        const bool d = cur[j].d != 0;
        const bool to = (cur[j].to & cur[j].d) != 0;
        const float v = cur[j].v;
        const float rr = to ? fmaf(gamma, v, cur[j].rew) : cur[j].rew;
        const float delta = (d ? rr : fmaf(gamma, vn, rr)) - v;
        adv = d ? delta : fmaf(gl, adv, delta);
        const float ret = adv + v;
        vn = v;
        s1 += (double)adv;
        s2 = fma((double)adv, (double)adv, s2);
        if (live) {
          adv_out[(size_t)t * rows + row] = adv;
          ret_out[(size_t)t * rows + row] = ret;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < GAE_U; j++) cur[j] = nxt[j];
  }
#undef GAE_LOAD
  if (part == nullptr) return;           // uniform
  if (!live) s1 = s2 = 0.0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    s1 += __shfl_xor(s1, m);
    s2 += __shfl_xor(s2, m);
  }
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = s1;
    part[2 * (size_t)blockIdx.x + 1] = s2;
  }
}

// n = T R' values; nparts pairs of k_gae.  Every workgroup forms mean and std itself (the pairs are a few kB, L2-hot) and rewrites its
// share of adv; workgroup 0 stores (mean, std) as f32
__global__ void __launch_bounds__(GAE_NORM_THREADS) k_gae_normalize(float* __restrict__ adv, long long n, const double* __restrict__ part, int nparts,
                                                                    float* __restrict__ stats) {
  double S = 0.0, Q = 0.0;
  for (int i = 0; i < nparts; i++) {
    S += part[2 * i];
    Q += part[2 * i + 1];
  }
  const double mean = S / (double)n;
  const double sd = sqrt(fmax((Q - S * mean) / (double)(n - 1), 0.0));
  const double inv = 1.0 / (sd + (double)1e-8f);
  for (long long i = (long long)blockIdx.x * GAE_NORM_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * GAE_NORM_THREADS)
    adv[i] = (float)(((double)adv[i] - mean) * inv);
  if (blockIdx.x == 0 && threadIdx.x == 0 && stats != nullptr) {
    stats[0] = (float)mean;
    stats[1] = (float)sd;
  }
}
