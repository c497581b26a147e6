"""Deterministic synthetic instances of the MIQP path: seed -> ModelParameters.

Constants follow DefaultSettings() (src/miqp_planner_data.hpp:190-242) and the way MiqpPlanner fills
ModelParameters (src/miqp_planner.cpp:95-133 solver/global block, :348-378 weights); the region tables are the
fitted tables of the reference fixtures (planner_miqp_amd/data/region_tables_*.json).  Geometry: straight
two-lane road, cars merging into the lane y = -1.75, optional constant-velocity rectangular obstacles."""
import json
import math
import os

import numpy as np

from .ctypes_types import ModelParameters

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
_TABLES = {}

CONFIGS = {
    # name: (cars, steps, regions, environment pieces, obstacles)
    "cfg2": (1, 20, 16, 1, 0),
    "cfg3": (2, 20, 32, 2, 0),
    "cfg4": (2, 20, 32, 2, 4),
    "mini": (2, 8, 32, 1, 0),
    "mini1": (1, 10, 32, 1, 1),
    "mini3": (3, 6, 32, 1, 0),
    "mini4": (4, 6, 32, 1, 0),
    "mini3b": (3, 8, 32, 1, 0),
    "mini4b": (4, 8, 32, 1, 0),
    "cfg5s": (4, 10, 32, 2, 0),   # reduced stand-in of cfg5 (4 cars) that the CPU oracle finishes in seconds
    "cfg5": (4, 30, 64, 2, 0),
}


def tables(R):
    if R not in _TABLES:
        _TABLES[R] = json.load(open(os.path.join(_DATA, "region_tables_%d.json" % R)))
    return _TABLES[R]


def region_of(frac, vx, vy):
    """common/parameter/regions.cpp:16-33 CalculateRegionIdx: sector that contains the velocity direction"""
    th = math.atan2(vy, vx) % (2 * math.pi)
    R = len(frac)
    return int(th / (2 * math.pi / R)) % R


def generate(config="cfg3", seed=0, gap=0.01, max_time=10.0):
    """config: a name of CONFIGS or a tuple (cars, steps, regions, environment pieces, obstacles[, obstacle edges]);
    more than two environment pieces split the road into overlapping rectangles, more than four obstacle edges make the
    obstacles regular polygons around the same rectangle's circumscribed ellipse"""
    cfg = CONFIGS[config] if isinstance(config, str) else tuple(config)
    C_, N, R, E, O = cfg[:5]
    LO = cfg[5] if len(cfg) > 5 else 4
    rng = np.random.Generator(np.random.MT19937(seed))
    T = tables(R)
    p = ModelParameters()
    p.NumSteps, p.nr_regions, p.NumCars, p.nr_obstacles, p.nr_environments = N, R, C_, O, E
    p.max_lines_obstacles = LO if O > 0 else 0
    p.max_solution_time, p.relative_mip_gap_tolerance = max_time, gap
    p.ts = 0.25
    eps = 1e-6
    p.min_vel_x_y, p.max_vel_x_y = float(T["min_vel_x_y"]) - eps, float(T["max_vel_x_y"]) + eps
    p.total_min_acc, p.total_max_acc = float(T["total_min_acc"]) - eps, float(T["total_max_acc"]) + eps
    p.total_min_jerk, p.total_max_jerk = float(T["total_min_jerk"]) - eps, float(T["total_max_jerk"]) + eps
    p.agent_safety_distance = np.zeros(N)
    p.agent_safety_distance_slack = np.full(N, 3.0)
    p.maximum_slack, p.WEIGHTS_SLACK, p.WEIGHTS_SLACK_OBSTACLE = 3.0, 30.0, 2000.0
    p.minimum_region_change_speed = float(T["minimum_region_change_speed"])
    lam = 0.5
    scale = np.array([lam if c == 0 or C_ == 1 else (1 - lam) / (C_ - 1) for c in range(C_)])
    if C_ == 1:
        scale[:] = lam
    p.WEIGHTS_POS_X = 2.0 * scale; p.WEIGHTS_POS_Y = 2.0 * scale
    p.WEIGHTS_VEL_X = 0.0 * scale; p.WEIGHTS_VEL_Y = 0.0 * scale
    p.WEIGHTS_ACC_X = 0.0 * scale; p.WEIGHTS_ACC_Y = 0.0 * scale
    p.WEIGHTS_JERK_X = 1.0 * scale; p.WEIGHTS_JERK_Y = 1.0 * scale
    p.WheelBase = np.full(C_, 2.8); p.CollisionRadius = np.full(C_, 1.0)
    frac = np.array(T["fraction_parameters"], float).reshape(R, 4)
    p.fraction_parameters = frac
    for k in ["POLY_SINT_UB", "POLY_SINT_LB", "POLY_COSS_UB", "POLY_COSS_LB", "POLY_KAPPA_AX_MAX", "POLY_KAPPA_AX_MIN"]:
        setattr(p, k, np.array(T[k], float).reshape(R, 3))
    for k in ["min_acc_x", "max_acc_x", "min_acc_y", "max_acc_y", "min_jerk_x", "max_jerk_x", "min_jerk_y", "max_jerk_y"]:
        setattr(p, k, np.tile(np.array(T[k], float).reshape(1, R), (C_, 1)))
    x0 = np.zeros((C_, 6)); xr = np.zeros((C_, N)); yr = np.zeros((C_, N)); vxr = np.zeros((C_, N)); vyr = np.zeros((C_, N))
    init = np.zeros(C_, int); poss = np.zeros((C_, R), int)
    for c in range(C_):
        lane = 1.75 if c % 2 == 0 else -1.75
        sgn = -1.0 if lane > 0 else 1.0
        px = 8.0 * c + rng.uniform(-2, 2); v0 = rng.uniform(4, 9); vdes = rng.uniform(5, 10)
        x0[c] = [px, v0, 0.0, lane, 0.1 * sgn, 0.0]
        xr[c] = px + vdes * p.ts * np.arange(N); yr[c] = -1.75; vxr[c] = vdes
        j0 = region_of(frac, v0, 0.1 * sgn)
        init[c] = j0 + 1
        jr = region_of(frac, vdes, 0.0)
        for j in (j0, jr, (jr - 1) % R):          # heading 0 lies on the border of regions R and 1
            for dj in (-1, 0, 1):
                poss[c, (j + dj) % R] = 1
    p.IntitialState, p.x_ref, p.y_ref, p.vx_ref, p.vy_ref = x0, xr, yr, vxr, vyr
    p.initial_region, p.possible_region = init, poss
    if E == 1:
        p.MultiEnvironmentConvexPolygon = [np.array([[-10, -5.25], [150, -5.25], [150, 5.25], [-10, 5.25]], float)]
    elif E == 2:
        p.MultiEnvironmentConvexPolygon = [np.array([[-10, -5.25], [75, -5.25], [75, 5.25], [-10, 5.25]], float),
                                           np.array([[65, -5.25], [150, -5.25], [150, 5.25], [65, 5.25]], float)]
    elif E > 2:
        w = 160.0 / E
        p.MultiEnvironmentConvexPolygon = [np.array([[-10 + e * w - 5, -5.25], [-10 + (e + 1) * w + 5, -5.25], [-10 + (e + 1) * w + 5, 5.25], [-10 + e * w - 5, 5.25]], float)
                                           for e in range(E)]
    else:
        p.MultiEnvironmentConvexPolygon = []
    obs = []
    for o in range(O):
        ox = rng.uniform(20, 80); ov = rng.uniform(0, 6); oy = 1.75 if rng.uniform() < 0.5 else -1.75
        hl, hw = 4.8 / 2 + 1.0, 1.8 / 2 + 1.0     # rectangle inflated by the collision radius
        per_t = []
        for i in range(N):
            cx = ox + ov * p.ts * i
            if LO == 4:
                per_t.append(np.array([[cx - hl, oy - hw], [cx + hl, oy - hw], [cx + hl, oy + hw], [cx - hl, oy + hw]], float))
            else:   # counter-clockwise LO-gon on the ellipse through the rectangle's corners
                a = 2 * math.pi * (np.arange(LO) + 0.5) / LO
                per_t.append(np.stack([cx + math.sqrt(2) * hl * np.cos(a), oy + math.sqrt(2) * hw * np.sin(a)], 1))
        obs.append(per_t)
    p.ObstacleConvexPolygon = obs
    p.obstacle_is_soft = [0] * O
    return p


def advance(params, record, steps=1, extra_possible=()):
    """the next cycle's ModelParameters of a synthetic instance in a receding horizon, ``steps`` steps after ``params`` was solved to ``record``
    (a RawResults): the initial state of every car is the record's state at step ``steps`` and initial_region its active region there; the
    references are moved on by steps * ts * (vx_ref, vy_ref); every obstacle polygon is moved ``steps`` steps along its constant velocity (the
    displacement between its first two steps).  Everything else is unchanged.  ``extra_possible``: (car, region index from 0) pairs that become
    possible regions of the new instance as well, so that its possible-region indices are not those of ``params``.  ``params`` is left as it is."""
    q = params.copy()
    Cn, N = int(q.NumCars), int(q.NumSteps)
    s = int(steps)
    if not 1 <= s <= N - 1:
        raise ValueError("steps outside 1 .. NumSteps - 1")
    x0 = np.array(q.IntitialState, float).reshape(Cn, 6)
    init = np.array(q.initial_region, int).reshape(Cn)
    for c in range(Cn):
        x0[c] = [record.pos_x[c, s], record.vel_x[c, s], record.acc_x[c, s], record.pos_y[c, s], record.vel_y[c, s], record.acc_y[c, s]]
        init[c] = int(np.argmax(record.active_region[c, s])) + 1
    q.IntitialState, q.initial_region = x0, init
    vx, vy = np.array(q.vx_ref, float).reshape(Cn, N), np.array(q.vy_ref, float).reshape(Cn, N)
    q.x_ref = np.array(q.x_ref, float).reshape(Cn, N) + s * q.ts * vx
    q.y_ref = np.array(q.y_ref, float).reshape(Cn, N) + s * q.ts * vy
    q.ObstacleConvexPolygon = [[np.asarray(o[i], float) + s * (np.asarray(o[1], float) - np.asarray(o[0], float)) for i in range(N)] for o in q.ObstacleConvexPolygon]
    poss = np.array(q.possible_region, int).reshape(Cn, -1)
    for c, j in extra_possible:
        poss[int(c), int(j)] = 1
    q.possible_region = poss
    return q
