// kernels_view.hpp -- k_view: one image of ONE env from a free camera, for episode recording (upstream's FloatingCameraSensor on env 0,
// mqe/utils/helpers.py:276-298, driven by the state machine of legged_robot.py:916-957).  Isaac Gym's rasteriser is closed, so this is the
// depth camera's answer once more: a ray caster over the geometry the physics collides with, by k_depth_camera's own rules (the
// functions of kernels_camera.hpp: cam_ground, cam_walls, cam_bodies -- every robot of the env, no own-robot exclusion), which also keeps
// WHICH surface won and its normal, and shades the pixel from those two alone.  include/mqe_hip.h (mqe_render_view) is the
// specification: conventions, surfaces, normal rules, id word, colour formula.  Known answers and the oracle's caster: tests/test_view_gpu.py.
// Mapping: k_depth_camera's one workgroup per env would put a 360 x 240 image's 86 400 rays on one compute unit of 256.  Here the grid
// is the image in 16 x 16-pixel tiles, one 256-thread workgroup per tile, and each wavefront owns an 8 x 8 block of its tile: its 64 rays
// are neighbours, so the marches run about equally long and the per-robot / per-NPC ball tests branch wave-uniformly almost everywhere.
// Every workgroup rebuilds the env's link frames and world-space primitives in LDS (7.6 kB, <= 52 chain walks): no workspace, no second
// launch.  Threads outside the image cast their ray like the others (they pass the barriers) and are masked at the store.
#pragma once
#include "kernels_camera.hpp"

#define VIEW_TILE 16
struct ViewArgs {
  uint32_t* rgba; float4* geom; int32_t* id;       // each may be null
  int env, H, W; float tan_half_h;
  float eye[3], f[3], l[3], u[3];                  // the camera: position, forward, left, up (unit, orthogonal; built on the host in double)
  float far_;
};

__constant__ float c_view_palette[MQE_VIEW_PALETTE_ROWS][3] = MQE_VIEW_PALETTE;

// colour of a pixel from its id word and normal alone (include/mqe_hip.h): r | g << 8 | b << 16 | 255 << 24
__device__ __forceinline__ uint32_t view_colour(int id, CV3 n) {
  const int cls = id & 255;
  const int sky[3] = MQE_VIEW_SKY;
  if (cls == MQE_VIEW_NONE) return (uint32_t)sky[0] | (uint32_t)sky[1] << 8 | (uint32_t)sky[2] << 16 | 0xFF000000u;
  const float L[3] = MQE_VIEW_LIGHT;
  const int row = cls == MQE_VIEW_GROUND ? 0 : (cls == MQE_VIEW_WALL ? 1 : (cls == MQE_VIEW_ROBOT ? 2 + ((id >> 8) & 3) : cls + 2));
  const float k = cls == MQE_VIEW_GROUND ? ((id & MQE_VIEW_CHECKER_BIT) ? 1.0f + MQE_VIEW_CHECKER : 1.0f - MQE_VIEW_CHECKER) : 1.0f;
  const float shade = MQE_VIEW_AMBIENT + MQE_VIEW_DIFFUSE * fmaxf(0.0f, n.x * L[0] + n.y * L[1] + n.z * L[2]);
  uint32_t px = 0xFF000000u;
#pragma unroll
  for (int c = 0; c < 3; c++) px |= (uint32_t)(255.0f * fminf(1.0f, c_view_palette[row][c] * k * shade) + 0.5f) << (8 * c);
  return px;
}

__global__ void __launch_bounds__(256) k_view(const DevModel* __restrict__ m, DevState st, ViewArgs va) {
  __shared__ float s_link[CAM_LINK_FLOATS];
  __shared__ float s_prim[CAM_PRIM_FLOATS];
  const int tid = threadIdx.x;
  const int A = m->A, P = m->P;
  const float* root = st.root + (size_t)va.env * (A + P) * 13;
  const float* dof = st.dof + (size_t)va.env * m->ND * 2;
  cam_stage_env(m, root, dof, s_link, s_prim, tid);
  const int wave = tid >> 6, lane = tid & 63;                       // wavefront = an 8 x 8 block of the tile, lane = a pixel of it, row-major
  const int pj = blockIdx.x * VIEW_TILE + (wave & 1) * 8 + (lane & 7), pi = blockIdx.y * VIEW_TILE + (wave >> 1) * 8 + (lane >> 3);
  const float tan_v = va.tan_half_h * (float)va.H / (float)va.W;
  const float yc = -(2.0f * (pj + 0.5f) / va.W - 1.0f) * va.tan_half_h;      // column 0 = the camera's left (+y)
  const float zc = -(2.0f * (pi + 0.5f) / va.H - 1.0f) * tan_v;               // row 0 = the top (+z)
  const CV3 o = cv(va.eye[0], va.eye[1], va.eye[2]);
  const CV3 d = cv(va.f[0] + va.l[0] * yc + va.u[0] * zc, va.f[1] + va.l[1] * yc + va.u[1] * zc, va.f[2] + va.l[2] * yc + va.u[2] * zc);
  CamHit h;
  h.t = va.far_; h.id = MQE_VIEW_NONE; h.n = cv(0.0f, 0.0f, 0.0f);
  cam_ground<true>(m, o, d, h);
  cam_walls(m, o, d, h);
  cam_bodies(m, root, dof, s_link, s_prim, o, d, -1, h);
  if (cdot(h.n, d) > 0.0f) h.n = cv(-h.n.x, -h.n.y, -h.n.z);         // towards the eye
  if (pi < va.H && pj < va.W) {
    const size_t pix = (size_t)pi * va.W + pj;
    if (va.rgba != nullptr) va.rgba[pix] = view_colour(h.id, h.n);
    if (va.geom != nullptr) va.geom[pix] = make_float4(h.id != MQE_VIEW_NONE ? -h.t : __uint_as_float(0xFF800000u), h.n.x, h.n.y, h.n.z);      // -inf as its bit pattern
    if (va.id != nullptr) va.id[pix] = h.id;
  }
}
