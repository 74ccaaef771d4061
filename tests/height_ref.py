"""float64 numpy restatement of the terrain height scan's specification (include/mqe_hip.h, mqe_measure_heights): the height of the static
surface under a yaw-aligned grid around every robot.  Takes the terrain object's maps (wall_sdf, ground_height, wall_top, wall_height,
ground_z) and the descriptor's scenery boxes; shares no code with the kernel."""
import numpy as np


def quat_apply_yaw_cs(quat_xyzw):
    """(..., 4) -> (cos, sin) of upstream's quat_apply_yaw (mqe/utils/math.py:38-42): the rotation of the normalised (0, 0, qz, qw);
    identity where qz^2 + qw^2 < 1e-18"""
    q = np.asarray(quat_xyzw, np.float64)
    z, w = q[..., 2], q[..., 3]
    n2 = z * z + w * w
    ok = n2 >= 1e-18
    d = np.where(ok, n2, 1.0)
    return np.where(ok, (w * w - z * z) / d, 1.0), np.where(ok, 2.0 * w * z / d, 0.0)


def world_points(root_rows, points_xy):
    """root rows (R, >= 7) and base-frame grid (P, 2) -> world x, y, each (R, P)"""
    r, p = np.asarray(root_rows, np.float64), np.asarray(points_xy, np.float64)
    c, s = quat_apply_yaw_cs(r[:, 3:7])
    x = r[:, 0:1] + c[:, None] * p[None, :, 0] - s[:, None] * p[None, :, 1]
    y = r[:, 1:2] + s[:, None] * p[None, :, 0] + c[:, None] * p[None, :, 1]
    return x, y


def _cell(v, hs, n):
    with np.errstate(invalid="ignore"):
        f = np.minimum(np.maximum(v / hs, 0.0), float(n - 1))
    f = np.where(np.isnan(f), 0.0, f)              # fmin(fmax(NaN, 0), limit) = 0
    i = np.minimum(f.astype(np.int64), n - 2)
    return i, f - i


def _bilinear(m, ix, iy, tx, ty):
    m = np.asarray(m, np.float64)
    s00, s01, s10, s11 = m[ix, iy], m[ix, iy + 1], m[ix + 1, iy], m[ix + 1, iy + 1]
    a0, a1 = s00 + (s01 - s00) * ty, s10 + (s11 - s10) * ty
    return a0 + (a1 - a0) * tx


def surface_height(x, y, terrain, hs, boxes=None, detail=False):
    """H(x, y) of the specification, float64, any shape.  terrain: an object with wall_sdf, wall_height, ground_z and optionally
    ground_height / wall_top (None: absent); hs: the raster spacing the engine holds (desc.horizontal_scale); boxes: None (terrain only) or
    a list of (centre xyz (...,3) broadcastable to x, half xyz) world-aligned scenery boxes.  detail: also the wall SDF's sample, tx, ty."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    sdf = np.asarray(terrain.wall_sdf, np.float64)
    nx, ny = sdf.shape
    ix, tx = _cell(x, hs, nx)
    iy, ty = _cell(y, hs, ny)
    g = np.full(x.shape, float(terrain.ground_z))
    gh = getattr(terrain, "ground_height", None)
    if gh is not None:
        g = g + _bilinear(gh, ix, iy, tx, ty)
    s = _bilinear(sdf, ix, iy, tx, ty)
    wt = getattr(terrain, "wall_top", None)
    if wt is not None:
        top = np.asarray(wt, np.float64)[np.where(tx < 0.5, ix, ix + 1), np.where(ty < 0.5, iy, iy + 1)]
    else:
        top = np.full(x.shape, float(terrain.wall_height))
    H = np.where(s <= 0.0, np.maximum(g, top), g)
    for c, h in boxes or ():
        c, h = np.asarray(c, np.float64), np.asarray(h, np.float64)
        inside = (np.abs(x - c[..., 0]) <= h[0]) & (np.abs(y - c[..., 1]) <= h[1])
        H = np.where(inside, np.maximum(H, c[..., 2] + h[2]), H)
    return (H, s, tx, ty) if detail else H


def scenery_boxes(desc, root3, num_agents):
    """the descriptor's static scenery boxes as surface_height's `boxes`, one centre per robot: root3 (N, A + P, 13) root state; centre =
    the env's first NPC root + static_box_center"""
    nb = np.asarray(root3, np.float64)[:, num_agents, :3]                      # (N, 3)
    nb = np.repeat(nb, num_agents, axis=0)[:, None, :]                          # (R, 1, 3)
    return [(nb + np.array([desc.static_box_center[b][k] for k in range(3)], np.float64),
             np.array([desc.static_box_half[b][k] for k in range(3)], np.float64)) for b in range(int(desc.n_static_boxes))]


def measured_heights(root3, num_agents, points_xy, terrain, hs, desc=None, scenery=False, detail=False):
    """(R, P) float64 heights for a root-state tensor (N, A + P, 13) (numpy) and a (P, 2) grid"""
    root3 = np.asarray(root3)
    rows = root3[:, :num_agents].reshape(-1, root3.shape[-1])
    x, y = world_points(rows, points_xy)
    boxes = scenery_boxes(desc, root3, num_agents) if scenery and desc is not None else None
    return surface_height(x, y, terrain, hs, boxes, detail)
