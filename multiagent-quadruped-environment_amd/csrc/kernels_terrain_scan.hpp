// kernels_terrain_scan.hpp -- k_height_scan: legged_gym's measured_heights (reference legged_robot.py:1047-1061 _init_height_points,
// :1094-1097 _reward_base_height, :1033-1045 _draw_debug_vis; the call site go1.py:235-236) -- the height of the static surface under a
// yaw-aligned grid of points around every robot's base, from the current root state.  Upstream's own _get_heights is absent from the
// reference snapshot (its call site is commented out), so the numbers are UNPINNED by any reference program: the meaning is the
// published legged_gym one, the surface is the one this engine's physics collides with (include/mqe_hip.h, mqe_measure_heights, is the
// specification; tests/height_ref.py restates it in float64).
//   world point of robot r, grid point p = root_xy + Rz (px, py), Rz = upstream's quat_apply_yaw (mqe/utils/math.py:38-42): the rotation
//     of the normalised quaternion (0, 0, qz, qw) -- the twist about z, not the Euler yaw of a tilted body; identity when qz^2 + qw^2 < 1e-18;
//   H(x, y): the cell and the weights as the sphere lanes' terrain test takes them (kernels_physics.hpp: clamp to the raster, bilinear
//     map_sample_dev), ground_z + the relief's sample; inside a wall footprint (the wall SDF's sample <= 0) the wall top of the nearer
//     raster point (wall_top, or wall_height) when that is higher; with MQE_HSCAN_SCENERY the tops of the static scenery boxes whose
//     footprint holds the point.  Robots, free NPCs and the 1-dof link are never seen.
// Mapping: one thread per output element, element i of a workgroup = float i of its slab of the [R][P] output, so that consecutive
// threads write consecutive floats whatever P is (plain 4 B stores: a wavefront's store is one contiguous 256 B run at any 4 B alignment
// of out_dev, which 16 B stores would only match with a phase-dependent head and tail for no fewer memory requests per element of the
// nine gathers each one costs anyway; the compiler pairs the two entries of a raster row into one 8 B load).  A 256-thread workgroup
// owns ha.rpg WHOLE robots -- the host picks rpg so that rpg * P fills the workgroup's passes (187 points: 15 robots = 2805 elements =
// 11 passes, 0.4 % idle lanes; one robot would idle 27 %) -- stages the point table (P x 2 floats, <= 8 kB) and each robot's (x, y,
// cos, sin) in LDS once, and splits i into (robot, point) by a multiplication with the host's reciprocal of P: no quaternion work and
// no integer division per element.  20 VGPRs, no scratch; 7.9 us for 8192 robots x 187 points on one MI355X, 17.8 us for 32768
// (profiles/height_scan.txt).
#pragma once
#include "kernels_physics.hpp"

#define HSCAN_THREADS 256
#define HSCAN_MAX_RPG 32
// magic = floor(2^32 / P) + 1: umulhi(i, magic) == i / P for i < 2^32 / P (i < rpg * P <= 2^15 here); P == 1 has no 32-bit magic (0)
// The maps travel as kernel arguments, not through DevModel: a pointer argument is known to be global memory (global_load, no flat
// aperture test per gather), and the loop's constants need no second round of scalar loads behind the model pointer.
struct HscanArgs {
  float* out; const float* pts; const float* root;
  const float *ground_height, *wall_sdf, *wall_top;      // DevModel's maps: relief or null, wall SDF, per-cell wall tops or null
  int nx, ny; float hs, ground_z, wall_height;
  int P, rpg; unsigned magic; int flags;
};

__global__ void __launch_bounds__(HSCAN_THREADS) k_height_scan(const DevModel* __restrict__ m, HscanArgs ha) {
  __shared__ float2 s_pts[MQE_MAX_HEIGHT_POINTS];
  __shared__ float4 s_rob[HSCAN_MAX_RPG];            // root x, y, cos, sin of the twist about z
  __shared__ float4 s_npc[HSCAN_MAX_RPG];            // the env's scenery actor (NPC 0) root, MQE_HSCAN_SCENERY only
  const int tid = threadIdx.x, P = ha.P;
  const int r0 = blockIdx.x * ha.rpg;
  const int nrob = min(ha.rpg, m->R - r0);
  const int n_static = (ha.flags & MQE_HSCAN_SCENERY) ? m->n_static : 0;
  for (int p = tid; p < P; p += HSCAN_THREADS) s_pts[p] = reinterpret_cast<const float2*>(ha.pts)[p];
  if (tid < nrob) {
    const int A = m->A, r = r0 + tid, e = r / A, a = r - e * A;
    const float* env = ha.root + (size_t)e * (A + m->P) * 13;
    const float* row = env + a * 13;
    const float qz = row[5], qw = row[6], n2 = qz * qz + qw * qw;
    float c = 1.0f, s = 0.0f;
    if (n2 >= 1e-18f) { c = (qw * qw - qz * qz) / n2; s = 2.0f * qw * qz / n2; }
    s_rob[tid] = make_float4(row[0], row[1], c, s);
    if (n_static > 0) s_npc[tid] = make_float4(env[A * 13], env[A * 13 + 1], env[A * 13 + 2], 0.0f);
  }
  __syncthreads();
  const int n = nrob * P;
  float* out = ha.out + (size_t)r0 * P;
  const float hs = ha.hs, ground_z = ha.ground_z;
  const int nx = ha.nx, ny = ha.ny;
  const float* __restrict__ gh = ha.ground_height;
  const float* __restrict__ sdf = ha.wall_sdf;
  const float* __restrict__ wtop = ha.wall_top;
  for (int i = tid; i < n; i += HSCAN_THREADS) {
    const int rl = P == 1 ? i : (int)__umulhi((unsigned)i, ha.magic);
    const float2 pt = s_pts[i - rl * P];
    const float4 rb = s_rob[rl];
    const float x = rb.x + (rb.z * pt.x - rb.w * pt.y), y = rb.y + (rb.w * pt.x + rb.z * pt.y);
    // the clamp in this form puts a NaN on 0; an index is formed from nothing but the clamped value
    const float fx = fminf(fmaxf(x / hs, 0.0f), (float)(nx - 1)), fy = fminf(fmaxf(y / hs, 0.0f), (float)(ny - 1));
    const int ix = max(min((int)fx, nx - 2), 0), iy = max(min((int)fy, ny - 2), 0);
    const float tx = fx - ix, ty = fy - iy;
    const size_t cell = (size_t)ix * ny + iy;
    float gx, gy;
    float g = ground_z;
    if (gh != nullptr) g += map_sample_dev(gh + cell, ny, tx, ty, hs, gx, gy);
    float H = g;
    if (sdf != nullptr && map_sample_dev(sdf + cell, ny, tx, ty, hs, gx, gy) <= 0.0f) {
      // inside a wall footprint: the top of the wall nearest to the point's own cell, a world z as the physics compares it
      const float top = wtop != nullptr ? wtop[(size_t)(tx < 0.5f ? ix : ix + 1) * ny + (ty < 0.5f ? iy : iy + 1)] : ha.wall_height;
      H = fmaxf(g, top);
    }
    if (n_static > 0) {
      const float4 nb = s_npc[rl];
      for (int bx = 0; bx < n_static; bx++)
        if (fabsf(x - (nb.x + m->sb_center[bx][0])) <= m->sb_half[bx][0] && fabsf(y - (nb.y + m->sb_center[bx][1])) <= m->sb_half[bx][1])
          H = fmaxf(H, nb.z + m->sb_center[bx][2] + m->sb_half[bx][2]);
    }
    out[i] = H;
  }
}
