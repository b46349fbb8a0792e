"""The class ids of dtsim_labels (include/dtsim.h) and the host's default tables.

The device writes three ids on its own -- NONE (a pixel the distortion table leaves without a source), SKY, GROUND -- and otherwise what two
host tables say: a class per texel of every texture (read for tile textures at the nearest texel of the hit) and a class per mesh.  The
defaults built here: tiles take FLOOR / ROAD / MARK_* (3 .. 7), meshes a class per kind of object from OBJECT_FIRST = 8 up.  A user's own
tables go through BatchedSimulator.set_label_assets; ids are free in 0 .. 255, and CLASS_NAMES / CLASS_IDS only describe the defaults.

The marking rule, on the ORIGINAL texel (r, g, b) of a drivable tile that assets.segment_texture (the reference's own paint / asphalt
split) did not black out, in integers and in this order:  r > 2 g -> red;  2 b < r -> yellow;  else white.  Red paint has almost no green,
yellow paint almost no blue, white paint neither: the fixtures' (200, 40, 36), (238, 200, 36) and (232, 232, 226) and the paint of
tests/golden/assets fall on the right side of both (tests/test_label_model_host.py)."""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import _ffi
from .maps import DRIVABLE

NONE, SKY, GROUND = _ffi.LABEL_NONE, _ffi.LABEL_SKY, _ffi.LABEL_GROUND
FLOOR, ROAD = _ffi.LABEL_FLOOR, _ffi.LABEL_ROAD                       # a non-drivable tile; the asphalt of a drivable one
MARK_WHITE, MARK_YELLOW, MARK_RED = _ffi.LABEL_MARK_WHITE, _ffi.LABEL_MARK_YELLOW, _ffi.LABEL_MARK_RED
OBJECT_FIRST = _ffi.LABEL_OBJECT_FIRST

# the default object classes, in id order from OBJECT_FIRST: (class name, prefixes of the mesh kinds it takes); the last one takes the rest.
# "duckiebot" stands before "duckie": the first matching prefix wins.
_OBJECT_CLASSES = (("duckiebot", ("duckiebot",)), ("duckie", ("duckie",)), ("cone", ("cone",)), ("sign", ("sign",)),
                   ("trafficlight", ("trafficlight",)), ("building", ("building", "house")), ("tree", ("tree",)),
                   ("vehicle", ("bus", "truck")), ("barrier", ("barrier",)), ("object", ()))

CLASS_NAMES = {NONE: "none", SKY: "sky", GROUND: "ground", FLOOR: "floor", ROAD: "road", MARK_WHITE: "mark_white",
               MARK_YELLOW: "mark_yellow", MARK_RED: "mark_red",
               **{OBJECT_FIRST + i: name for i, (name, _) in enumerate(_OBJECT_CLASSES)}}
CLASS_IDS = {name: i for i, name in CLASS_NAMES.items()}


def mesh_class(kind: str) -> int:
    """The default class id of one mesh kind (a map object's kind, or a mesh key such as "duckiebot:red" or "sign_stop")."""
    base = str(kind).split(":", 1)[0]
    for i, (_, prefixes) in enumerate(_OBJECT_CLASSES):
        if any(base.startswith(p) for p in prefixes):
            return OBJECT_FIRST + i
    return OBJECT_FIRST + len(_OBJECT_CLASSES) - 1


def mesh_classes(kinds: Sequence[str]) -> np.ndarray:
    """[len(kinds)] uint8: the default class of every mesh kind, in the order given (dtsim_set_label_assets' mesh_class)."""
    return np.array([mesh_class(k) for k in kinds], dtype=np.uint8)


def marking_class(rgb) -> np.ndarray:
    """The marking rule on [..., 3] (or more channels) uint8 texels: MARK_RED / MARK_YELLOW / MARK_WHITE."""
    a = np.asarray(rgb)
    r, g, b = (a[..., k].astype(np.int64) for k in range(3))
    return np.where(r > 2 * g, MARK_RED, np.where(2 * b < r, MARK_YELLOW, MARK_WHITE)).astype(np.uint8)


def texel_classes(texture_rgba, segmented_rgba, kind: str) -> np.ndarray:
    """[h, w] uint8: the default class of every texel of a tile texture of kind `kind`, in the texture's own row order.  texture_rgba: the
    texture as installed ([h, w, 4] uint8), segmented_rgba: assets.segment_texture of it.  A kind without lane curves (not in maps.DRIVABLE)
    is FLOOR throughout; on a drivable kind a texel is ROAD where the segmentation blacked it out, else a marking by marking_class."""
    tex, seg = np.asarray(texture_rgba), np.asarray(segmented_rgba)
    if tex.shape != seg.shape or tex.ndim != 3 or tex.shape[2] < 3:
        raise ValueError(f"texel_classes: texture {tex.shape} and its segmented version {seg.shape} must be one [h, w, 4] shape")
    if kind not in DRIVABLE:
        return np.full(tex.shape[:2], FLOOR, np.uint8)
    road = (seg[..., :3] == 0).all(axis=-1)
    return np.where(road, ROAD, marking_class(tex)).astype(np.uint8)
