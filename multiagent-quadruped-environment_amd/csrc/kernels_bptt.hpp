// kernels_bptt.hpp -- the PPO gradient of the RECURRENT actor-critic: truncated back-propagation through time through the GRU cell of
// kernels_gru.hpp (MQE_PPO_BPTT; include/mqe_hip.h, the recurrent section).  This file holds the constants, the LDS rule, the chunk addressing, the
// cell's backward and k_bptt_expand; the walk over the steps and the entry points k_bptt_grad<RT> / k_bptt_ln_grad<RT> are in
// kernels_actor_critic.hpp, beside the other walks.  The loss, its kinks, the statistics, the partial-gradient chains, k_ppo_reduce and Adam are
// kernels_ppo.hpp's, unchanged: what is new is WHICH samples a lane walks and the state that links them.
//
// CHUNKS (OpenRL / MAPPO's recurrent generator at data_chunk_length = L).  A trajectory of T steps over R' rows is T / L chunks per row; chunk
// c = (t0 / L) R' + r covers steps t0 .. t0 + L - 1 of row r, 0 <= c < (T / L) R'.  A minibatch is `count` chunks -- THE SELECTION of kernels_ppo.hpp
// with the chunk as its unit -- and M = count L samples: 1 / M = (float)(1.0 / (count L)).  A LANE IS A CHUNK: tile i of
// the minibatch is chunks i RT .. i RT + RT - 1, and workgroup b of G = min(tiles, PPO_MAX_WG) walks tiles b, b + G, ... (the fixed grid of k_ppo_grad).
// STATE.  Step 0 of a chunk starts both cells from the recorded tail of packed row t0 (offset P4, row r: the actor's Ha floats, then the critic's
// Hc), masked by row t0's done byte of the row's env: data, no gradient.  Step j > 0 starts from the h' this kernel computed at step j - 1 with the
// CURRENT parameters, masked by packed row t0 + j's done byte (a masked state is exactly 0.0f): k_actor_gru's rule.
//
// THE WALK, per tile and per network (actor, then critic):
//   forward sweep   steps 0 .. L - 2: observation, base, cell (gru_layer); keeps ONLY each step's masked input state h_in(j), in per-workgroup
//                   global scratch [L][H][RT] (L2-resident; L H RT floats a workgroup).  Step L - 1 needs no sweep: the backward recomputes it.
//   backward sweep  steps L - 1 .. 0: re-reads the observation and h_in(j), recomputes the base and the gates into LDS (the forward's own
//                   expressions: the forward's bits), the norm behind the cell and the head; the loss head of kernels_ppo.hpp; then
//                   head backward -> dh' (+ the carried state gradient where row t0 + j + 1 is not a reset) -> the cell's backward below ->
//                   dW_ih, dx through the last hidden layer's norm or activation derivative, dW_hh, the carried dh -> ppo_backward from the last
//                   hidden layer down.  Recomputing costs about one more forward and keeps the scratch at the input states.
// THE CELL'S BACKWARD, per unit, f32 (bptt_gates_back; dh' = the head's gradient, through LayerNorm(H) under the hidden norm -- ln_back without an
// activation derivative, its gamma / beta gradients go to gru.norm.* -- plus the carried dh of step j + 1 times that step's mask):
//     dn = dh' (1 - z);  dz = dh' (h - n);  dh = dh' z
//     da_n = dn (1 - n^2);  da_r = (da_n gh_n) r (1 - r);  da_z = dz z (1 - z)
//     dgi = (da_r, da_z, da_n);  dgh = (da_r, da_z, da_n r)
//     dW_ih += dgi x^T, db_ih += dgi;  dW_hh += dgh h_in^T, db_hh += dgh  (ppo_dw: the workgroup's chains, `first` on its first tile's step L - 1 only)
//     dx = W_ih^T dgi (ppo_dx);  dh += W_hh^T dgh (ppo_dx, RAW).  The dh that step 0 produces is dropped: the recorded state is data.
// No floating-point atomics: the same bits on every run.  Chunks past the end of the minibatch repeat the last one and carry delta = 0 at every
// step, so their dh' and carried dh are 0 too: +0 to every chain.
//
// LDS (THE RULE: bptt_lds_rows, bptt_lds_bytes; mirrored by abi.bptt_lds_rows / abi.bptt_row_tile).  The image of k_ppo_grad / k_ln_grad -- the
// observation, every hidden output of the larger network, [U, statistics, partials], 4 output rows -- plus, per unit of the wider cell Hm =
// max(Ha, Hc), BPTT_CELL_ROWS = 7 rows: h_in, the four gate rows (r, z, n, gh_n, turned in place into da_r, da_z, da_n, da_n r), h' (then dh', then
// dh' z) and the carried dh; with a norm 2 more rows (mu, rstd of the norm behind the cell: LN_STAT's slots are taken by the norms in front of the
// layers).  Behind the rows: the step's sample numbers, the chunks' first sample numbers (64-bit each), the done bytes of two steps and the seven
// running statistics of wavefront 0's lanes (f64; in registers across the whole walk they were the first thing the allocator spilled).
//     rows = ppo_lds_rows or ln_lds_rows + 7 Hm (+ 2 with a norm);   bytes = (rows (RT + 1) + 2 + 20 x 64) x 4
// RT = 64 where that fits 160 KiB, else 32; the first mqe_ppo_grad refuses, naming the width, what does not fit at 32.  Two 64 x 64 networks at
// D <= 30 take 64-row tiles without the norms (D + 128 + 448 + 4 rows); with both norms they take 32-row tiles.  Every recurrent shape with all
// widths <= 64 and D <= 128 fits: the largest, three 64-wide hidden layers at D = 128 with both norms, is 128 + 192 + 448 + 128 + 8 + 32 + 2 + 4 =
// 942 rows = 126.4 KiB at 32 rows.  The widest accepted cells are 147 wide (D = 16, one hidden layer, no norm: 16 + 147 + 1029 + 4 = 1196 rows = 159.2 KiB).
#pragma once
#include "mqe_common.hpp"
#include "kernels_actor.hpp"
#include "kernels_ppo.hpp"
#include "kernels_ln.hpp"
#include "kernels_gru.hpp"

// the constants of the recurrent section of include/mqe_hip.h that belong to mqe_ppo_grad: stated there in words, defined here (the define sets of the
// header and of kernels_gru.hpp are pinned by the tests), mirrored in mqe/engine/abi.py; tests/test_bptt.py compares the three
#define MQE_PPO_BPTT 32                   // mqe_ppo_grad flags: index_dev / first / count are chunks of L steps, the gradient runs through the cells
#define MQE_PPO_CHUNK_SHIFT 8             // bits 8 .. 15 of flags hold L
#define MQE_PPO_MAX_CHUNK 64              // 1 <= L <= 64

#define BPTT_CELL_ROWS 7                  // LDS rows per unit of the wider cell: h_in, r, z, n, gh_n, h', the carried dh
#define BPTT_LDS_LIMIT (160 * 1024)

// THE LDS RULE.  base: ppo_lds_rows (kernels_ppo.hpp) or, with a norm, ln_lds_rows (kernels_ln.hpp); Hm = max(Ha, Hc)
static inline int bptt_lds_rows(int base, int Hm, bool ln) { return base + BPTT_CELL_ROWS * Hm + (ln ? 2 : 0); }
static inline size_t bptt_lds_bytes(int rows, int rt) { return ((size_t)rows * (rt + 1) + 2 + 20 * 64) * sizeof(float); }

// what the recurrent gradient kernels take beside k_ppo_grad's arguments
struct BpttArgs {
  long long tail_off, done_off;     // floats from the start of a packed row to its tail (P4) and to its done bytes (R' (D + 1))
  long long n_chunks;               // (T / L) R'
  int L, Aw, Ha, Hc, Hm;
};

// THE CHUNK ADDRESSING: the flat sample number of step 0 of chunk c; step j of it lies j rows further (bptt_load_step, k_bptt_expand)
__device__ __forceinline__ long long bptt_first_sample(long long c, int rows, int L) {
  const long long tc = c / rows, r = c - tc * rows;
  return tc * L * rows + r;
}
// the first sample number of the tile's chunks (past the end of the minibatch the last one again)
template <int RT>
__device__ __forceinline__ void bptt_chunks(long long* crow, const PpoTraj& tr, const BpttArgs& b, long long tile, int tid) {
  if (tid < RT) {
    long long i = tile * RT + tid;
    if (i > tr.count - 1) i = tr.count - 1;
    crow[tid] = bptt_first_sample(ppo_unit(tr.index, tr.first, i, b.n_chunks), tr.rows, b.L);
  }
}
// step j of the tile's chunks: its sample numbers, its done bytes (dn: one int per row) and its observations -> LDS [k][row].  The caller's barrier follows
template <int LD, int RT>
__device__ __forceinline__ void bptt_load_step(float* lds, long long* srow, int* dn, const long long* crow, const float* __restrict__ packed, long long stride,
                                               int rows, const BpttArgs& b, int j, int D, int tid) {
  if (tid < RT) {
    const long long s = crow[tid] + (long long)j * rows;
    const long long t = s / rows, rr = s - t * rows;
    srow[tid] = s;
    dn[tid] = reinterpret_cast<const uint8_t*>(packed + (size_t)t * (size_t)stride + b.done_off)[rr / b.Aw];
  }
  __syncthreads();
  for (int e = tid; e < RT * D; e += ACT_THREADS) {
    const int r = e / D, k = e - r * D;
    const long long s = srow[r];
    const long long t = s / rows, rr = s - t * rows;
    lds[k * LD + r] = packed[(size_t)t * (size_t)stride + (size_t)rr * D + k];
  }
}
// the state step 0 starts from: the recorded tail of the step's packed row, H floats at `hoff` of the row's Hs, masked by the step's done byte
template <int LD, int RT>
__device__ __forceinline__ void bptt_load_tail(float* hin, const long long* srow, const int* dn, const float* __restrict__ packed, long long stride, int rows,
                                               const BpttArgs& b, int hoff, int H, int tid) {
  const int Hs = b.Ha + b.Hc;
  for (int e = tid; e < RT * H; e += ACT_THREADS) {
    const int r = e / H, k = e - r * H;
    const long long s = srow[r];
    const long long t = s / rows, rr = s - t * rows;
    const float v = packed[(size_t)t * (size_t)stride + (size_t)b.tail_off + (size_t)rr * Hs + hoff + k];
    hin[k * LD + r] = dn[r] ? 0.0f : v;
  }
}
// h_in of a step <-> the workgroup's scratch [H][RT], coalesced.  mask (or null): the done bytes of the step the state goes INTO
template <int LD, int RT>
__device__ __forceinline__ void bptt_keep_state(const float* src, float* hin, const int* mask, float* __restrict__ scr, int H, int tid) {
  for (int e = tid; e < RT * H; e += ACT_THREADS) {
    const int k = e / RT, r = e & (RT - 1);
    const float v = (mask != nullptr && mask[r]) ? 0.0f : src[k * LD + r];
    hin[k * LD + r] = v;
    scr[e] = v;
  }
}
template <int LD, int RT>
__device__ __forceinline__ void bptt_fetch_state(float* hin, const float* __restrict__ scr, int H, int tid) {
  for (int e = tid; e < RT * H; e += ACT_THREADS) hin[(e / RT) * LD + (e & (RT - 1))] = scr[e];
}

// THE CELL'S BACKWARD per unit, in place (the file's first comment): g = the rows r, z, n, gh_n of gru_cell -> da_r, da_z, da_n, da_n r;
// hp = dh' without the carried part -> dh' z; carry: the dh of step j + 1, added where that step is no reset (mask: its done bytes; null: the last step)
template <int LD>
__device__ __forceinline__ void bptt_gates_back(int H, float* g, float* hp, const float* hin, const float* carry, const int* mask, int row, int wave) {
  const size_t G = (size_t)H * LD;
  for (int u = wave; u < H; u += ACT_WAVES) {
    const int i = u * LD + row;
    float dhp = hp[i];
    if (mask != nullptr) dhp += mask[row] ? 0.0f : carry[i];
    const float r = g[i], z = g[G + i], n = g[2 * G + i], ghn = g[3 * G + i], h = hin[i];
    const float dn = dhp * (1.0f - z), dz = dhp * (h - n);
    const float dan = dn * fmaf(-n, n, 1.0f);
    const float dar = (dan * ghn) * r * (1.0f - r);
    const float daz = dz * z * (1.0f - z);
    g[i] = dar;
    g[G + i] = daz;
    g[2 * G + i] = dan;
    g[3 * G + i] = dan * r;
    hp[i] = dhp * z;
  }
}
// the running statistics of wavefront 0's lanes between the steps: LDS [7][64] doubles <-> PpoSums (STORE: S -> LDS; otherwise LDS -> the result)
template <bool STORE>
__device__ __forceinline__ PpoSums bptt_sums(double* sums, int lane, PpoSums S) {
  double* v[7] = {&S.Lpi, &S.Lv, &S.Kl, &S.Clip, &S.gls[0], &S.gls[1], &S.gls[2]};
#pragma unroll
  for (int q = 0; q < 7; q++) {
    if (STORE) sums[q * 64 + lane] = *v[q];
    else *v[q] = sums[q * 64 + lane];
  }
  return S;
}
// dst = src (+ add) over the H rows of a cell buffer, lane = row
template <int LD, bool ADD>
__device__ __forceinline__ void bptt_rows(float* dst, const float* src, int H, int row, int wave) {
  for (int u = wave; u < H; u += ACT_WAVES) dst[u * LD + row] = ADD ? dst[u * LD + row] + src[u * LD + row] : src[u * LD + row];
}

// the minibatch's count L flat sample numbers s = (t0 + j) R' + r, chunk-major: what k_vn_moments / k_vn_apply (kernels_vn.hpp) read as their index list
#define BPTT_EXPAND_THREADS 256
__global__ void __launch_bounds__(BPTT_EXPAND_THREADS) k_bptt_expand(const int32_t* __restrict__ index, long long first, long long count, long long n_chunks, int rows,
                                                                     int L, int32_t* __restrict__ out) {
  for (long long e = (long long)blockIdx.x * BPTT_EXPAND_THREADS + threadIdx.x; e < count * L; e += (long long)gridDim.x * BPTT_EXPAND_THREADS) {
    const long long i = e / L;
    const int j = (int)(e - i * L);
    out[e] = (int32_t)(bptt_first_sample(ppo_unit(index, first, i, n_chunks), rows, L) + (long long)j * rows);
  }
}
