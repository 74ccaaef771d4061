// kernels_camera.hpp -- k_depth_camera: the onboard forward depth camera of LeggedRobotField (reference legged_robot_field.py:23-93,
// 196-223: gym.create_camera_sensor + attach_camera_to_body(FOLLOW_TRANSFORM) + get_camera_image_gpu_tensor(IMAGE_DEPTH)) as a ray
// caster over the geometry the physics collides with.  The reference renders with Isaac Gym's rasteriser, which is closed and absent:
// there is no image to compare with, so the contract is geometric -- for every pixel the distance ALONG THE OPTICAL AXIS to the first
// surface of: the ground (slab plane or relief map), the wall prisms (signed-distance map + wall tops), the OTHER robots' collision
// primitives (the URDF's boxes, capsules, spheres), the free NPCs (spheres / the box), the 1-dof link's plank and platform, the scenery
// boxes -- reported as Isaac Gym's IMAGE_DEPTH does: NEGATIVE depth in metres, -inf where nothing is hit within `far`.
// Camera frame = the body-local transform (position, ZYX Euler) of cfg.sensor.forward_camera on the base link, looking along its +x with
// +z up (Isaac Gym's attach convention); pixel (0, 0) is the top-left corner, the horizontal field of view is given, the vertical one
// follows from the aspect ratio.  Known answers: tests/test_camera_gpu.py.
// One 256-thread workgroup per env: the link frames of its robots by forward kinematics into LDS, the primitives in world coordinates
// behind them, then thread = pixel, looping over the env's cameras.
// The rules -- the staging of an env, the ground, the wall march, the bodies -- are __device__ functions that k_view (kernels_view.hpp,
// the free camera of episode recording) calls as well; they also report which surface was hit and its normal, which this kernel ignores.
// Its images are bit for bit those of the kernel that held the rules inline (profiles/view_render.txt).
#pragma once
#include "mqe_common.hpp"
#include "kernels_physics.hpp"      // map_sample_dev: the bilinear sample and its gradient

struct CamArgs { float* out; int H, W; float tan_half_h; float pos[3]; float rpy[3]; float far_; };

struct CV3 { float x, y, z; };
__device__ __forceinline__ CV3 cv(float x, float y, float z) { CV3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ CV3 operator+(CV3 a, CV3 b) { return cv(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ CV3 operator-(CV3 a, CV3 b) { return cv(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ CV3 operator*(float s, CV3 a) { return cv(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float cdot(CV3 a, CV3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ CV3 cmul(const float* R, CV3 v) {      // R v, row-major
  return cv(R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z);
}
__device__ __forceinline__ CV3 cmulT(const float* R, CV3 v) {     // R^T v
  return cv(R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z, R[2] * v.x + R[5] * v.y + R[8] * v.z);
}
__device__ __forceinline__ void cmat(const float* A, const float* B, float* C) {
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) C[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
}
__device__ __forceinline__ void cquat(const float* q, float* R) {    // (x, y, z, w), normalised here
  float x = q[0], y = q[1], z = q[2], w = q[3];
  const float in = 1.0f / sqrtf(x * x + y * y + z * z + w * w);
  x *= in; y *= in; z *= in; w *= in;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
__device__ __forceinline__ void caxis(CV3 a, float q, float* R) {    // rotation by q about the unit axis a
  const float c = cosf(q), s = sinf(q), t = 1 - c;
  R[0] = t * a.x * a.x + c; R[1] = t * a.x * a.y - s * a.z; R[2] = t * a.x * a.z + s * a.y;
  R[3] = t * a.x * a.y + s * a.z; R[4] = t * a.y * a.y + c; R[5] = t * a.y * a.z - s * a.x;
  R[6] = t * a.x * a.z - s * a.y; R[7] = t * a.y * a.z + s * a.x; R[8] = t * a.z * a.z + c;
}
__device__ __forceinline__ CV3 ccross(CV3 a, CV3 b) { return cv(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
// World frame of body bb of one robot (0 = base, 1 + 3 leg + {0, 1, 2} = hip, thigh, calf) by walking its chain from the base (<= 3
// joints): rotation R (row-major) and origin p, from the robot's root row (pos, quat xyzw, ...) and its 12 (angle, speed) dof pairs:
// p_b = p_parent + R_parent offset_b, R_b = R_parent Rot(axis_b, q_b).  VEL: also the world angular velocity w and the world velocity v
// of the frame's origin, w_b = w_parent + (R_b axis_b) qd_b, v_b = v_parent + w_parent x (p_b - p_parent), from the root row's linvel /
// angvel.  Shared by k_depth_camera (poses) and k_rigid_body_state (kernels_bodies.hpp).
template <bool VEL>
__device__ __forceinline__ void robot_link_walk(const mqe_robot_model& rm, const float* root13, const float* dof24, int bb, float* R, CV3& p,
                                                CV3& w, CV3& v) {
  cquat(root13 + 3, R);
  p = cv(root13[0], root13[1], root13[2]);
  if (VEL) { v = cv(root13[7], root13[8], root13[9]); w = cv(root13[10], root13[11], root13[12]); }
  if (bb > 0) {
    const int leg = (bb - 1) / 3, t = (bb - 1) - leg * 3;
    for (int k = 0; k <= t; k++) {
      const int b = 1 + leg * 3 + k;
      const CV3 d = cmul(R, cv(rm.joint_offset[b][0], rm.joint_offset[b][1], rm.joint_offset[b][2]));
      p = p + d;
      if (VEL) v = v + ccross(w, d);
      const CV3 ax = cv(rm.joint_axis[b][0], rm.joint_axis[b][1], rm.joint_axis[b][2]);
      float Rj[9], Rn[9];
      caxis(ax, dof24[(b - 1) * 2], Rj);
      cmat(R, Rj, Rn);
      for (int i = 0; i < 9; i++) R[i] = Rn[i];
      if (VEL) w = w + dof24[(b - 1) * 2 + 1] * cmul(R, ax);
    }
  }
}
// ray o + t d (d NOT normalised: t is the depth along the optical axis), nearest t in (tmin, best) or best
__device__ __forceinline__ float ray_sphere(CV3 o, CV3 d, CV3 c, float r, float best) {
  const CV3 oc = o - c;
  const float a = cdot(d, d), b = cdot(d, oc), cc = cdot(oc, oc) - r * r;
  const float h = b * b - a * cc;
  if (h < 0.0f || cc < 0.0f) return best;                     // miss, or the eye is inside
  const float t = (-b - sqrtf(h)) / a;
  return (t > 1e-4f && t < best) ? t : best;
}
__device__ __forceinline__ float ray_capsule(CV3 o, CV3 d, CV3 c, CV3 u, float r, float best) {
  const CV3 pa = c - u, ba = 2.0f * u, oa = o - pa;
  const float baba = cdot(ba, ba), bard = cdot(ba, d), baoa = cdot(ba, oa), rdoa = cdot(d, oa), oaoa = cdot(oa, oa), dd = cdot(d, d);
  if (baba < 1e-12f) return ray_sphere(o, d, c, r, best);
  const float a = baba * dd - bard * bard, b = baba * rdoa - baoa * bard, cc = baba * oaoa - baoa * baoa - r * r * baba;
  const float h = b * b - a * cc;
  if (h >= 0.0f && a > 1e-12f) {
    const float t = (-b - sqrtf(h)) / a;
    const float y = baoa + t * bard;
    if (y > 0.0f && y < baba) return (t > 1e-4f && t < best) ? t : best;
  }
  float t1 = ray_sphere(o, d, pa, r, best);
  return ray_sphere(o, d, c + u, r, t1);
}
__device__ __forceinline__ float ray_box(CV3 o, CV3 d, CV3 c, const float* R, CV3 h, float best) {      // oriented box: slabs in its frame
  const CV3 ol = cmulT(R, o - c), dl = cmulT(R, d);
  float t0 = 1e-4f, t1 = best;
  const float oo[3] = {ol.x, ol.y, ol.z}, dv[3] = {dl.x, dl.y, dl.z}, hh[3] = {h.x, h.y, h.z};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (fabsf(dv[k]) < 1e-9f) { if (fabsf(oo[k]) > hh[k]) return best; continue; }
    const float inv = 1.0f / dv[k];
    float ta = (-hh[k] - oo[k]) * inv, tb = (hh[k] - oo[k]) * inv;
    if (ta > tb) { const float s = ta; ta = tb; tb = s; }
    t0 = fmaxf(t0, ta); t1 = fminf(t1, tb);
    if (t0 > t1) return best;
  }
  return (fabsf(oo[0]) <= hh[0] && fabsf(oo[1]) <= hh[1] && fabsf(oo[2]) <= hh[2]) ? best : t0;      // (an eye inside the box sees nothing of it)
}

#define CAM_LINK 12          // floats per link frame in LDS: R (9), origin (3)
#define CAM_PRIM 16          // floats per primitive: type, link, radius, -, centre (3), -, half-axis / half extents (3), -, (4 spare)
#define CAM_LINK_FLOATS (MQE_MAX_AGENTS * MQE_NBODY * CAM_LINK)
#define CAM_PRIM_FLOATS (MQE_MAX_AGENTS * MQE_MAX_PRIMS * CAM_PRIM)

// ---- what both casters share (k_depth_camera below, k_view in kernels_view.hpp): one statement of every rule ---------------------------
// The nearest hit of one ray so far: t (starts at `far`), the id word of the surface that set it (include/mqe_hip.h, MQE_VIEW_ID; 0 =
// nothing) and that surface's outward normal at the hit point.  k_depth_camera reads t alone (id and n then cost nothing: they are dead).
struct CamHit { float t; int id; CV3 n; };
__device__ __forceinline__ CV3 cunit(CV3 v) { return (1.0f / sqrtf(cdot(v, v))) * v; }
__device__ __forceinline__ void hit_sphere(CamHit& h, CV3 o, CV3 d, CV3 c, float r, int id) {
  const float t = ray_sphere(o, d, c, r, h.t);
  if (t < h.t) { h.t = t; h.id = id; h.n = cunit(o + t * d - c); }                 // (p - c) / r
}
__device__ __forceinline__ void hit_capsule(CamHit& h, CV3 o, CV3 d, CV3 c, CV3 u, float r, int id) {
  const float t = ray_capsule(o, d, c, u, r, h.t);
  if (t < h.t) {                                                                   // p minus the closest point of the segment
    const CV3 p = o + t * d, pa = c - u, ba = 2.0f * u;
    const float baba = cdot(ba, ba);
    const float s = baba < 1e-12f ? 0.5f : clampf(cdot(p - pa, ba) / baba, 0.0f, 1.0f);
    h.t = t; h.id = id; h.n = cunit(p - (pa + s * ba));
  }
}
__device__ __forceinline__ void hit_box(CamHit& h, CV3 o, CV3 d, CV3 c, const float* R, CV3 hb, int id) {
  const float t = ray_box(o, d, c, R, hb, h.t);
  if (t < h.t) {                                                                   // the axis of the face the entry slab belongs to
    const CV3 ol = cmulT(R, o - c), dl = cmulT(R, d);
    const float oo[3] = {ol.x, ol.y, ol.z}, dv[3] = {dl.x, dl.y, dl.z}, hh[3] = {hb.x, hb.y, hb.z};
    float tin = -3.0e38f, din = 1.0f;
    int kin = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (fabsf(dv[k]) < 1e-9f) continue;
      const float inv = 1.0f / dv[k];
      const float ta = fminf((-hh[k] - oo[k]) * inv, (hh[k] - oo[k]) * inv);
      if (ta > tin) { tin = ta; kin = k; din = dv[k]; }
    }
    const CV3 ax = kin == 0 ? cv(R[0], R[3], R[6]) : (kin == 1 ? cv(R[1], R[4], R[7]) : cv(R[2], R[5], R[8]));
    h.t = t; h.id = id; h.n = (din > 0.0f ? -1.0f : 1.0f) * ax;
  }
}
// true: no point of the ball (c, r) lies on the ray nearer than `best` (the eye outside it) -- what is inside the ball need not be tested
__device__ __forceinline__ bool ray_clear_of_ball(CV3 o, CV3 d, CV3 c, float r, float best) {
  const CV3 oc = o - c;
  const float a = cdot(d, d), b = cdot(d, oc), cc = cdot(oc, oc) - r * r;
  if (cc <= 0.0f) return false;
  const float hq = b * b - a * cc;
  if (hq < 0.0f || b > 0.0f) return true;
  return -b - sqrtf(hq) >= best * a;
}
__device__ __forceinline__ int ground_id(CV3 p) {        // class ground + the 1 m checker: parity of floor(x) + floor(y) of the hit point
  return MQE_VIEW_GROUND | ((((int)floorf(p.x) + (int)floorf(p.y)) & 1) << 24);
}

// The env's link frames (thread = (robot, body), walking its chain from the base: <= 3 joints) and, behind a barrier, its robots'
// primitives in world coordinates, into LDS; a second barrier, then every thread may read both.  Called by all 256 threads.
__device__ __forceinline__ void cam_stage_env(const DevModel* __restrict__ m, const float* root, const float* dof, float* s_link, float* s_prim, int tid) {
  const int A = m->A, npr = m->robot.n_prims;
  const mqe_robot_model& rm = m->robot;
  if (tid < A * MQE_NBODY) {
    const int r = tid / MQE_NBODY, bb = tid - r * MQE_NBODY;
    float R[9];
    CV3 p, w_, v_;
    robot_link_walk<false>(rm, root + r * 13, dof + r * 24, bb, R, p, w_, v_);
    float* L = s_link + tid * CAM_LINK;
    for (int i = 0; i < 9; i++) L[i] = R[i];
    L[9] = p.x; L[10] = p.y; L[11] = p.z;
  }
  __syncthreads();
  if (tid < A * npr) {
    const int r = tid / npr, q = tid - r * npr;
    const int link = r * MQE_NBODY + rm.prim_body[q];
    const float* L = s_link + link * CAM_LINK;
    const CV3 c = cv(L[9], L[10], L[11]) + cmul(L, cv(rm.prim_center[q][0], rm.prim_center[q][1], rm.prim_center[q][2]));
    float* Q = s_prim + tid * CAM_PRIM;
    Q[0] = (float)rm.prim_type[q]; Q[1] = (float)link; Q[2] = rm.prim_half[q][0];
    Q[4] = c.x; Q[5] = c.y; Q[6] = c.z;
    if (rm.prim_type[q] == MQE_PRIM_BOX) { Q[8] = rm.prim_half[q][0]; Q[9] = rm.prim_half[q][1]; Q[10] = rm.prim_half[q][2]; }
    else { const CV3 u = cmul(L, cv(rm.prim_axis[q][0], rm.prim_axis[q][1], rm.prim_axis[q][2])); Q[8] = u.x; Q[9] = u.y; Q[10] = u.z; }
  }
  __syncthreads();
}

// ground: the slab plane, or the relief map marched in half cells and bisected.  STEP_BY_PRODUCT: march step k stands at t = k dt instead
// of at the f32 sum of k steps.  The sum drifts by ~sqrt(k) ulp, which moves the bisection's grid of dt / 64 against the float64
// specification's and puts ~0.2 % of a low camera's ground pixels one grid cell (2e-4 m at the shipped raster) off; the product does
// not drift.  k_view marches by the product; k_depth_camera keeps the sum, and with it its images bit for bit.
template <bool STEP_BY_PRODUCT>
__device__ __forceinline__ void cam_ground(const DevModel* __restrict__ m, CV3 o, CV3 d, CamHit& h) {
  const float hs = m->hs;
  const int nx = m->sdf_nx, ny = m->sdf_ny;
  if (m->ground_height == nullptr) {
    if (d.z < -1e-9f) {
      const float t = (m->ground_z - o.z) / d.z;
      if (t > 1e-4f && t < h.t) { h.t = t; h.id = ground_id(o + t * d); h.n = cv(0.0f, 0.0f, 1.0f); }
    }
  } else {
    const float dxy = sqrtf(d.x * d.x + d.y * d.y);
    const float dt = dxy > 1e-6f ? 0.5f * hs / dxy : 0.05f;
    auto hgt = [&](CV3 p) -> float {
      float fx = fminf(fmaxf(p.x / hs, 0.0f), (float)(nx - 1)), fy = fminf(fmaxf(p.y / hs, 0.0f), (float)(ny - 1));
      int ix = min((int)fx, nx - 2), iy = min((int)fy, ny - 2);
      const float tx = fx - ix, ty = fy - iy;
      const float* g = m->ground_height + (size_t)ix * ny + iy;
      const float b0 = g[0] + (g[1] - g[0]) * ty, b1 = g[ny] + (g[ny + 1] - g[ny]) * ty;
      return m->ground_z + b0 + (b1 - b0) * tx;
    };
    float tp = 0.0f;
    int k = 1;
    for (float t = dt; t < h.t; t = STEP_BY_PRODUCT ? (float)(++k) * dt : t + dt) {
      const CV3 p = o + t * d;
      if (p.z < hgt(p)) {
        float lo = tp, hi = t;
        for (int it = 0; it < 6; it++) { const float mid = 0.5f * (lo + hi); const CV3 pm = o + mid * d; if (pm.z < hgt(pm)) hi = mid; else lo = mid; }
        // the normal: normalize(-gx, -gy, 1) from the bilinear sample's own gradient at the hit point
        const CV3 ph = o + hi * d;
        const float fx = fminf(fmaxf(ph.x / hs, 0.0f), (float)(nx - 1)), fy = fminf(fmaxf(ph.y / hs, 0.0f), (float)(ny - 1));
        const int ix = min((int)fx, nx - 2), iy = min((int)fy, ny - 2);
        float gx, gy;
        map_sample_dev(m->ground_height + (size_t)ix * ny + iy, ny, fx - ix, fy - iy, hs, gx, gy);
        h.t = hi; h.id = ground_id(ph); h.n = cunit(cv(-gx, -gy, 1.0f));
        break;
      }
      tp = t;
    }
  }
}

// wall prisms: march over the signed-distance map of the wall set (a step never crosses more than the distance to the nearest wall)
__device__ __forceinline__ void cam_walls(const DevModel* __restrict__ m, CV3 o, CV3 d, CamHit& h) {
  const float hs = m->hs;
  const int nx = m->sdf_nx, ny = m->sdf_ny;
  const float dxy = sqrtf(d.x * d.x + d.y * d.y);
  if (dxy > 1e-6f && m->wall_sdf != nullptr) {
    float t = 1e-4f;
    for (int it = 0; it < 400 && t < h.t; it++) {
      const CV3 p = o + t * d;
      const float fxr = p.x / hs, fyr = p.y / hs;
      if (fxr < 0.0f || fyr < 0.0f || fxr > (float)(nx - 1) || fyr > (float)(ny - 1)) break;       // left the map
      int ix = min((int)fxr, nx - 2), iy = min((int)fyr, ny - 2);
      const float tx = fxr - ix, ty = fyr - iy;
      const float* sd = m->wall_sdf + (size_t)ix * ny + iy;
      const float a0 = sd[0] + (sd[1] - sd[0]) * ty, a1 = sd[ny] + (sd[ny + 1] - sd[ny]) * ty;
      const float s = a0 + (a1 - a0) * tx;
      if (s <= 0.002f) {                                     // on / inside a wall's footprint: below its top it is the wall
        const float top = m->wall_top != nullptr ? m->wall_top[(size_t)(tx < 0.5f ? ix : ix + 1) * ny + (ty < 0.5f ? iy : iy + 1)] : m->wall_height;
        if (p.z <= top && p.z >= m->ground_z - 1e-3f) {
          // the normal: up within 1 mm of the wall's top, else the horizontal gradient of the bilinear SDF sample
          float gx, gy;
          map_sample_dev(sd, ny, tx, ty, hs, gx, gy);
          float gl = sqrtf(gx * gx + gy * gy);
          if (gl < 1e-6f) { gx = 1.0f; gy = 0.0f; gl = 1.0f; }
          h.t = t; h.id = MQE_VIEW_WALL; h.n = top - p.z <= 1e-3f ? cv(0.0f, 0.0f, 1.0f) : cv(gx / gl, gy / gl, 0.0f);
          break;
        }
        t += 0.25f * hs / dxy;                               // above it: the ray may still come down onto the top face
      } else t += fmaxf(s, 0.002f) / dxy;
    }
  }
}

// everything that moves: the robots' primitives (robot `skip` left out: the onboard camera does not see its own robot; -1: none),
// the free NPCs (ball, sheep: spheres in the body frame; the box), the 1-dof link's base and link, the scenery boxes.  A robot is
// entered only if the ray meets the ball (base origin, feature_reach) nearer than the hit so far, a flock member likewise.
__device__ __forceinline__ void cam_bodies(const DevModel* __restrict__ m, const float* root, const float* dof, const float* s_link, const float* s_prim,
                                           CV3 o, CV3 d, int skip, CamHit& h) {
  const int A = m->A, npr = m->robot.n_prims;
  for (int r = 0; r < A; r++) {
    if (r == skip) continue;
    const float* B = s_link + (r * MQE_NBODY) * CAM_LINK;
    if (ray_clear_of_ball(o, d, cv(B[9], B[10], B[11]), m->robot.feature_reach + 1e-3f, h.t)) continue;
    for (int q = 0; q < npr; q++) {
      const float* Q = s_prim + (r * npr + q) * CAM_PRIM;
      const int type = (int)Q[0], id = MQE_VIEW_ID(MQE_VIEW_ROBOT, r, q);
      const CV3 c = cv(Q[4], Q[5], Q[6]);
      if (type == MQE_PRIM_BOX) hit_box(h, o, d, c, s_link + (int)Q[1] * CAM_LINK, cv(Q[8], Q[9], Q[10]), id);
      else if (type == MQE_PRIM_CAPSULE) hit_capsule(h, o, d, c, cv(Q[8], Q[9], Q[10]), Q[2], id);
      else hit_sphere(h, o, d, c, Q[2], id);
    }
  }
  if (m->has_box) {
    for (int p = 0; p < m->n_npc_dyn; p++) {
      float Rb[9];
      cquat(root + (A + p) * 13 + 3, Rb);
      hit_box(h, o, d, cv(root[(A + p) * 13], root[(A + p) * 13 + 1], root[(A + p) * 13 + 2]), Rb, cv(m->npc_box_half[0], m->npc_box_half[1], m->npc_box_half[2]),
              MQE_VIEW_ID(MQE_VIEW_NPC, p, 0));
    }
  } else {
    const int ns = m->npc_n_spheres;
    float reach = 0.0f;                                        // of one NPC's spheres about its origin
    for (int k = 0; k < ns; k++) {
      const float* sc = m->npc_sphere_center[k];
      reach = fmaxf(reach, sqrtf(sc[0] * sc[0] + sc[1] * sc[1] + sc[2] * sc[2]) + m->npc_sphere_radius[k]);
    }
    for (int p = 0; p < m->n_npc_dyn; p++) {
      const CV3 pb = cv(root[(A + p) * 13], root[(A + p) * 13 + 1], root[(A + p) * 13 + 2]);
      if (ns > 1 && ray_clear_of_ball(o, d, pb, reach + 1e-3f, h.t)) continue;
      float Rb[9];
      cquat(root + (A + p) * 13 + 3, Rb);
      for (int k = 0; k < ns; k++)
        hit_sphere(h, o, d, pb + cmul(Rb, cv(m->npc_sphere_center[k][0], m->npc_sphere_center[k][1], m->npc_sphere_center[k][2])), m->npc_sphere_radius[k],
                   MQE_VIEW_ID(MQE_VIEW_NPC, p, 0));
    }
  }
  const float I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (m->has_seesaw) {
    const CV3 sb = cv(root[A * 13], root[A * 13 + 1], root[A * 13 + 2]);
    if (m->ss_base_half[0] > 0.0f) hit_box(h, o, d, sb, I3, cv(m->ss_base_half[0], m->ss_base_half[1], m->ss_base_half[2]), MQE_VIEW_ID(MQE_VIEW_LINK_SCENE, 0, 0));
    CV3 piv = sb + cv(m->ss_joint_offset[0], m->ss_joint_offset[1], m->ss_joint_offset[2]);
    const float th = dof[(12 * A) * 2];
    float Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (m->ss_axis == 3) piv.y += th; else caxis(m->ss_axis == 2 ? cv(0, 0, 1) : cv(0, 1, 0), th, Rp);
    const CV3 pc = piv + cmul(Rp, cv(m->ss_plank_center[0], m->ss_plank_center[1], m->ss_plank_center[2]));
    if (m->ss_link_cyl) hit_capsule(h, o, d, pc, cv(0, 0, fmaxf(m->ss_plank_half[2] - m->ss_plank_half[0], 0.0f)), m->ss_plank_half[0], MQE_VIEW_ID(MQE_VIEW_LINK_SCENE, 0, 1));      // upright cylinder ~ capsule
    else hit_box(h, o, d, pc, Rp, cv(m->ss_plank_half[0], m->ss_plank_half[1], m->ss_plank_half[2]), MQE_VIEW_ID(MQE_VIEW_LINK_SCENE, 0, 1));
  }
  for (int bx = 0; bx < m->n_static; bx++) {
    const CV3 nb = cv(root[A * 13], root[A * 13 + 1], root[A * 13 + 2]);
    hit_box(h, o, d, nb + cv(m->sb_center[bx][0], m->sb_center[bx][1], m->sb_center[bx][2]), I3, cv(m->sb_half[bx][0], m->sb_half[bx][1], m->sb_half[bx][2]),
            MQE_VIEW_ID(MQE_VIEW_SCENERY, bx, 0));
  }
}

__global__ void __launch_bounds__(256) k_depth_camera(const DevModel* __restrict__ m, DevState st, CamArgs ca) {
  __shared__ float s_link[CAM_LINK_FLOATS];
  __shared__ float s_prim[CAM_PRIM_FLOATS];
  const int e = blockIdx.x, tid = threadIdx.x;
  const int A = m->A, P = m->P;
  const float* root = st.root + (size_t)e * (A + P) * 13;
  const float* dof = st.dof + (size_t)e * m->ND * 2;
  cam_stage_env(m, root, dof, s_link, s_prim, tid);
  // ---- rays --------------------------------------------------------------------------------------------------------------------------
  float Rc[9];                                                   // camera in the base frame: ZYX Euler (yaw, pitch, roll) = Rz Ry Rx
  {
    float Rz[9], Ry[9], Rx[9], T[9];
    caxis(cv(0, 0, 1), ca.rpy[2], Rz); caxis(cv(0, 1, 0), ca.rpy[1], Ry); caxis(cv(1, 0, 0), ca.rpy[0], Rx);
    cmat(Rz, Ry, T); cmat(T, Rx, Rc);
  }
  const int npix = ca.H * ca.W;
  const float tan_v = ca.tan_half_h * (float)ca.H / (float)ca.W;
  for (int idx = tid; idx < A * npix; idx += blockDim.x) {
    const int a = idx / npix, pix = idx - a * npix, pi = pix / ca.W, pj = pix - pi * ca.W;
    const float* B = s_link + (a * MQE_NBODY) * CAM_LINK;          // the base link of robot a
    float Rw[9];
    cmat(B, Rc, Rw);
    const CV3 o = cv(B[9], B[10], B[11]) + cmul(B, cv(ca.pos[0], ca.pos[1], ca.pos[2]));
    const float yc = -(2.0f * (pj + 0.5f) / ca.W - 1.0f) * ca.tan_half_h;      // column 0 = the camera's left (+y)
    const float zc = -(2.0f * (pi + 0.5f) / ca.H - 1.0f) * tan_v;               // row 0 = the top (+z)
    const CV3 d = cmul(Rw, cv(1.0f, yc, zc));                                    // t = depth along the optical axis
    CamHit h;
    h.t = ca.far_; h.id = 0; h.n = cv(0.0f, 0.0f, 0.0f);
    cam_ground<false>(m, o, d, h);
    cam_walls(m, o, d, h);
    cam_bodies(m, root, dof, s_link, s_prim, o, d, a, h);                        // the OTHER robots
    ca.out[((size_t)e * A + a) * npix + pix] = h.t < ca.far_ ? -h.t : __uint_as_float(0xFF800000u);       // -inf (the build drops inf arithmetic: written as its bit pattern)
  }
}
