// kernels_bodies.hpp -- k_rigid_body_state: Isaac Gym's rigid-body state tensor (reference legged_robot_field.py:196-197,
// gym.acquire_rigid_body_state_tensor; refreshed in post_physics_step, :117-119) from the current root and dof state.
// MQE_T_RIGID_BODY_STATE is f32 [N][NBR][13], the rows of MQE_T_CONTACT_FORCE in their order; columns as the root state: origin of the
// link frame (3), quaternion xyzw (4), linear velocity of that origin (3), angular velocity (3), all in the world frame.
//   robot rows (17 per robot): base = the root row copied (bit-equal); hip / thigh / calf by the chain walk shared with the depth camera
//     (robot_link_walk); foot = its calf translated by the foot joint's origin (the centre of the foot's collision sphere, go1.urdf
//     *_foot_fixed), with the calf's rotation and angular velocity;
//   free NPCs (ball, sheep, box): the NPC's root row;
//   1-dof link scenes (2 rows per NPC): the fixed base's root row, then the link: base origin + seesaw_joint_offset, then a rotation about
//     +y / +z or a slide along +y by the NPC dof -- world-aligned, as the physics places it (kernels_physics.hpp, "seesaw geometry");
//   static scenery: each of its npc_reported_bodies rows is the actor's root pose with zero velocity (the physics holds collapsed boxes,
//     not per-link frames).
// One thread per row, ra.epg whole envs per 256-thread workgroup; the rows are staged in LDS at the 16 B phase of the block's first
// float and leave as one contiguous block of 16 B stores (the partial words at either end as single floats).
#pragma once
#include "kernels_camera.hpp"

#define RBS_THREADS 256
struct RbsArgs { float* out; int epg; float foot[4][3]; };     // envs per workgroup; foot origin in the calf frame, per leg

__device__ __forceinline__ void rbs_quat_from_R(const float* R, const float* ref_q, float* q) {
  // Shepperd: the largest of w, x, y, z first; then normalised and put on the hemisphere of ref_q (the robot's base quaternion)
  float x, y, z, w;
  const float tr = R[0] + R[4] + R[8];
  if (tr > 0.0f) {
    const float s = 2.0f * sqrtf(tr + 1.0f), is = 1.0f / s;
    w = 0.25f * s; x = (R[7] - R[5]) * is; y = (R[2] - R[6]) * is; z = (R[3] - R[1]) * is;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const float s = 2.0f * sqrtf(1.0f + R[0] - R[4] - R[8]), is = 1.0f / s;
    w = (R[7] - R[5]) * is; x = 0.25f * s; y = (R[1] + R[3]) * is; z = (R[2] + R[6]) * is;
  } else if (R[4] > R[8]) {
    const float s = 2.0f * sqrtf(1.0f + R[4] - R[0] - R[8]), is = 1.0f / s;
    w = (R[2] - R[6]) * is; x = (R[1] + R[3]) * is; y = 0.25f * s; z = (R[5] + R[7]) * is;
  } else {
    const float s = 2.0f * sqrtf(1.0f + R[8] - R[0] - R[4]), is = 1.0f / s;
    w = (R[3] - R[1]) * is; x = (R[2] + R[6]) * is; y = (R[5] + R[7]) * is; z = 0.25f * s;
  }
  float in = 1.0f / sqrtf(x * x + y * y + z * z + w * w);
  if (x * ref_q[0] + y * ref_q[1] + z * ref_q[2] + w * ref_q[3] < 0.0f) in = -in;
  q[0] = x * in; q[1] = y * in; q[2] = z * in; q[3] = w * in;
}

__device__ __forceinline__ void rbs_put(float* o, CV3 p, const float* q, CV3 v, CV3 w) {
  o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
  o[7] = v.x; o[8] = v.y; o[9] = v.z; o[10] = w.x; o[11] = w.y; o[12] = w.z;
}

__global__ void __launch_bounds__(RBS_THREADS) k_rigid_body_state(const DevModel* __restrict__ m, DevState st, RbsArgs ra) {
  __shared__ float4 s_rows4[(RBS_THREADS * 13 + 3 + 3) / 4];
  float* s_rows = (float*)s_rows4;
  const int tid = threadIdx.x, A = m->A, P = m->P, NBR = m->NBR;
  const int e0 = blockIdx.x * ra.epg;
  const int nrow = min(ra.epg, m->N - e0) * NBR;
  const size_t g0 = (size_t)e0 * NBR * 13;           // the block's first float in the output
  const int ph = (int)(g0 & 3);                        // ... and its phase in a 16 B word: LDS float ph + j holds output float g0 + j
  if (tid < nrow) {
    const int el = tid / NBR, row = tid - el * NBR;
    const size_t e = (size_t)(e0 + el);
    const float* root = st.root + e * (A + P) * 13;
    const float* dof = st.dof + e * m->ND * 2;
    float* o = s_rows + ph + tid * 13;
    const CV3 zero = cv(0.0f, 0.0f, 0.0f);
    if (row < MQE_NREP * A) {
      const int r = row / MQE_NREP, k = row - r * MQE_NREP;
      const float* rr = root + r * 13;
      if (k == 0) {
        for (int c = 0; c < 13; c++) o[c] = rr[c];
      } else {
        const int leg = (k - 1) >> 2, j = (k - 1) & 3;         // j: hip, thigh, calf, foot
        float R[9], q[4];
        CV3 p, w, v;
        robot_link_walk<true>(m->robot, rr, dof + r * 24, 1 + leg * 3 + min(j, 2), R, p, w, v);
        if (j == 3) {
          const CV3 d = cmul(R, cv(ra.foot[leg][0], ra.foot[leg][1], ra.foot[leg][2]));
          p = p + d;
          v = v + ccross(w, d);
        }
        rbs_quat_from_R(R, rr + 3, q);
        rbs_put(o, p, q, v, w);
      }
    } else {
      const int k = row - MQE_NREP * A;
      if (m->has_seesaw) {                              // 2 rows per NPC: the fixed base, the 1-dof link
        const int pn = k >> 1;
        const float* rb = root + (A + pn) * 13;
        if ((k & 1) == 0) {
          for (int c = 0; c < 13; c++) o[c] = rb[c];
        } else {
          const float th = dof[(12 * A + pn) * 2], thd = dof[(12 * A + pn) * 2 + 1];
          CV3 p = cv(rb[0] + m->ss_joint_offset[0], rb[1] + m->ss_joint_offset[1], rb[2] + m->ss_joint_offset[2]);
          float q[4] = {0.0f, 0.0f, 0.0f, 1.0f};
          CV3 v = zero, w = zero;
          if (m->ss_axis == 3) {                        // slider along +y
            p.y += th; v = cv(0.0f, thd, 0.0f);
          } else {                                      // hinge about +z (door) / +y (plank)
            float sh, ch;
            sincosf(0.5f * th, &sh, &ch);
            q[3] = ch;
            if (m->ss_axis == 2) { q[2] = sh; w = cv(0.0f, 0.0f, thd); }
            else { q[1] = sh; w = cv(0.0f, thd, 0.0f); }
          }
          rbs_put(o, p, q, v, w);
        }
      } else if (m->npc_kind == MQE_NPC_STATIC) {      // npc_reported_bodies rows per actor: its root pose, at rest
        const int pn = k / ((NBR - MQE_NREP * A) / P);
        const float* rb = root + (A + pn) * 13;
        rbs_put(o, cv(rb[0], rb[1], rb[2]), rb + 3, zero, zero);
      } else {                                          // free NPCs: one row each, the root row
        const float* rb = root + (A + k) * 13;
        for (int c = 0; c < 13; c++) o[c] = rb[c];
      }
    }
  }
  __syncthreads();
  const int n = 13 * nrow;
  const int head = min((4 - ph) & 3, n);               // floats before the first whole 16 B word of the block
  const int nvec = (n - head) >> 2;
  float* out = ra.out + g0;
  float4* out4 = (float4*)(out + head);
  const float4* src4 = s_rows4 + (ph + head) / 4;
  for (int i = tid; i < nvec; i += RBS_THREADS) out4[i] = src4[i];
  const int tail = head + 4 * nvec;
  if (tid < head) out[tid] = s_rows[ph + tid];
  else if (tid >= 4 && tid - 4 < n - tail) out[tail + tid - 4] = s_rows[ph + tail + tid - 4];
}
