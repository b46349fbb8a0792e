"""What the LED tests share without a device: the usual set of test spheres around a robot and the share of the touched pixels that may differ
from raster.overlay_leds (tests/test_gpu_leds.py, tests/rerender_model.py, tests/test_gpu_rerender_maps.py)."""
import math

import numpy as np


def led_share(touched):
    """Of `touched` pixels -- those the oracle's overlay changes -- how many may be off by more than 1: a sample at a sphere's silhouette, or where
    a sphere cuts a mesh or the ground, can fall on either side between float32 and float64."""
    return 0.04 * touched + 4


def sphere_set(pos, ang, st, seed):
    """World-space test spheres in front of a robot at (pos, ang) among objects in the states `st` (frame_parity.obj_states' form): free ones with
    halos, one cutting the ground, one through the nearest mesh object, one hidden behind it, one across the near plane, one at the image
    border, overlapping pairs (depth writes between spheres)."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, dtype=np.float64)
    d = np.array([math.cos(ang), 0.0, -math.sin(ang)])
    r = np.array([math.sin(ang), 0.0, math.cos(ang)])
    up = np.array([0.0, 1.0, 0.0])
    out = []
    for k in range(6):                                     # free spheres + halos, two of them overlapping on screen
        c = pos + d * rng.uniform(0.25, 0.9) + r * rng.uniform(-0.25, 0.25) + up * rng.uniform(0.03, 0.15)
        col = [(1, 0, 0), (0.5, 0.5, 0.5), (0, 0, 1), (0.5, 0, 0), (0, 0, 0.2), (0.2, 0.9, 0.3)][k]
        rad = rng.uniform(0.01, 0.035)
        out.append([*c, rad, *col, 1.0])
        out.append([*c, rad * (1.5 + 2.5 * float(np.mean(col))), *col, 0.2])
    c = pos + d * 0.4 + r * 0.05
    out.append([*c, 0.04, 0, 1, 0, 1.0])                   # centre on the road surface: half of it below the tile plane
    out.append([*(pos + d * 0.066 + up * 0.1), 0.05, 1, 1, 0, 1.0])   # around the camera: across the near plane
    out.append([*(pos + d * 0.5 + r * 0.62 + up * 0.05), 0.06, 1, 0, 1, 0.2])   # at the image border
    objs = [(np.linalg.norm(np.asarray(s["pos"]) - pos), np.asarray(s["pos"], dtype=np.float64)) for s in st if s["visible"]]
    if objs:
        p = min(objs, key=lambda t: t[0])[1]
        out.append([*(p + up * 0.05), 0.05, 0, 0.6, 1, 1.0])           # through the nearest object's mesh
        away = (p - pos) / max(np.linalg.norm(p - pos), 1e-6)
        out.append([*(p + away * 0.12 + up * 0.03), 0.02, 1, 1, 1, 1.0])   # behind it
    return np.asarray(out, np.float32)
