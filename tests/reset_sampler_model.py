"""The device-side reset sampler (csrc/physics.hip sample_init, the `rs` branches of apply_init and duckie_step, sampler_next_map) and
its generator (csrc/philox_rng.h), restated in numpy.  physics.hip is compiled with -ffp-contract=off and the sampler is integer and IEEE
double arithmetic, so everything here is meant to equal the device bit for bit -- except rng_normal, whose log and cos are the math
library's (glibc here through `math`, ocml on the device).

  a. generator    Philox4x32-10 on uint64 arrays masked to 32 bits, philox_init's key / counter layout, the draw functions
  b. sample_reset what sample_init decides for a batch of envs, in its draw order, with the rounding the device applies before a value
                  can be read back
  c. streams      the creation draws of kind 1 / kind 2 objects, finish_walk's redraw, the map draw, and blocks_used: the counter blocks
                  (ctr0, ctr1) each of them consumes

No GPU, no oracle.  Vectorised over envs: a Stream holds one row of words per env and a read position per env, so draws whose number
depends on the env (tile rejection) advance only the envs that take them."""
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

U = np.uint64
M32 = U(0xFFFFFFFF)
TAG_OBJECT, TAG_MAP = 0x4F424A00, 0x4D415000              # DT_RNG_TAG_OBJECT, DT_RNG_TAG_MAP
OBJ_EVENT_CREATE = 0xFFFFFF00                              # DT_OBJ_EVENT_CREATE
OBJ_EVENT_CREATE_FIRST = 0xFFFFFFFF                        # where it stood first: every later block carried into the next slot's row
TWO_PI = 6.283185307179586
TILE_TRIES = 4096
FALLBACK_POSE = (1.0, 1.0, 1.0)                            # x, z, angle (simulator.py:732-736)


def obj_event_walk(step_count):
    """DT_OBJ_EVENT_WALK: two blocks per step, the redraw takes 5 words"""
    return 2 * int(step_count)


# ---------------------------------------------------------------- a. generator --
def philox4x32_10(ctr, key):
    """ctr: 4, key: 2 uint64 arrays (values < 2^32, broadcastable) -> the 4 output words (Salmon et al. 2011)."""
    c0, c1, c2, c3 = (np.asarray(c, U) for c in ctr)
    k0, k1 = (np.asarray(k, U) for k in key)
    for _ in range(10):
        p0, p1 = U(0xD2511F53) * c0, U(0xCD9E8D57) * c2
        n0, n2 = (p1 >> U(32)) ^ c1 ^ k0, (p0 >> U(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0, k1 = (k0 + U(0x9E3779B9)) & M32, (k1 + U(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def stream_blocks(ctr0, ctr1, n_words):
    """the counter blocks [(ctr0, ctr1)] that a stream starting at (ctr0, ctr1) generates to hand out n_words words: philox_refill counts
    ctr0 up and carries into ctr1"""
    out = []
    for b in range((int(n_words) + 3) // 4):
        v = int(ctr0) + b
        out.append((v & 0xFFFFFFFF, (int(ctr1) + (v >> 32)) & 0xFFFFFFFF))
    return out


class Stream:
    """philox_init(seed, env, episode) for every env of `env` (array), optionally moved to the counter row (ctr0, ctr1) as philox_object
    and sampler_next_map do; the draw functions of philox_rng.h on top.  `mask` (bool [E]): only those envs draw (the others get the
    value of their next word without consuming it)."""

    def __init__(self, seed, env, episode, ctr0=0, ctr1=0):
        self.env = np.atleast_1d(np.asarray(env)).astype(U)
        E = self.env.size
        seed = np.broadcast_to(np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in np.atleast_1d(np.asarray(seed, object))], U), (E,))   # one, or one per env
        self.episode = np.broadcast_to(np.asarray(episode).astype(U), (E,))
        self.key0 = seed & M32
        self.key1 = (seed >> U(32)) ^ ((self.env * U(0x9E3779B1) + U(0x7F4A7C15)) & M32)
        self.ctr0, self.ctr1 = np.broadcast_to(np.asarray(ctr0).astype(U), (E,)), np.broadcast_to(np.asarray(ctr1).astype(U), (E,))
        self.pos = np.zeros(E, np.int64)
        self.words = np.zeros((E, 0), U)

    def ensure(self, n_words):
        have = self.words.shape[1]
        if n_words <= have:
            return
        nb0, nb1 = have // 4, (max(int(n_words), 2 * have, 64) + 3) // 4
        v = self.ctr0[:, None] + np.arange(nb0, nb1, dtype=U)[None, :]
        c0, c1 = v & M32, (self.ctr1[:, None] + (v >> U(32))) & M32
        o = philox4x32_10((c0, c1, self.episode[:, None], self.env[:, None]), (self.key0[:, None], self.key1[:, None]))
        blk = np.stack([o[3], o[2], o[1], o[0]], axis=2)          # rng_u32 hands out out[3], out[2], out[1], out[0]
        self.words = np.concatenate([self.words, blk.reshape(self.env.size, -1)], axis=1)

    def blocks(self, e=0):
        """the counter blocks env row e has consumed so far"""
        return stream_blocks(self.ctr0[e], self.ctr1[e], self.pos[e])

    def u32(self, mask=None):
        self.ensure(int(self.pos.max()) + 1)
        w = self.words[np.arange(self.env.size), self.pos]
        self.pos = self.pos + (1 if mask is None else mask.astype(np.int64))
        return w

    def double(self, mask=None):
        a, b = self.u32(mask) >> U(5), self.u32(mask) >> U(6)
        return (a.astype(np.float64) * 67108864.0 + b.astype(np.float64)) / 9007199254740992.0

    def uniform(self, lo, hi, mask=None):
        lo, hi = np.float64(lo), np.float64(hi)
        return lo + (hi - lo) * self.double(mask)

    def below(self, n, mask=None):
        return ((self.u32(mask) * U(n)) >> U(32)).astype(np.int64)

    def normal(self, loc, scale, mask=None):
        """Box-Muller; log and cos through `math` (the C library's), one env at a time"""
        u1, u2 = 1.0 - self.double(mask), self.double(mask)
        return np.array([loc + scale * math.sqrt(-2.0 * math.log(a)) * math.cos(TWO_PI * b) for a, b in zip(u1.tolist(), u2.tolist())],
                        np.float64)


# ---------------------------------------------------------------- b. the reset --
@dataclass
class SamplerCfg:
    """the fields of dtsim_reset_sampler that bear on one map"""
    domain_rand: bool
    dynamics_rand: bool = False
    max_attempts: int = 5000
    accept_start_angle_deg: float = 60.0
    color_sky: Sequence[float] = (0.45, 0.82, 1.0)
    color_ground: Sequence[float] = (0.15, 0.15, 0.15)
    start_tile: Optional[Tuple[int, int]] = None            # user_tile_start, else the map's start_tile, else None: drawn
    start_pose: Optional[Tuple[float, float, float]] = None  # (x, z, angle) relative to the start tile

    @classmethod
    def for_map(cls, mt, *, domain_rand, dynamics_rand=False, accept_start_angle_deg=60.0, user_tile_start=None, **kw):
        """the rule of BatchedSimulator.install_reset_sampler"""
        tile = tuple(int(v) for v in user_tile_start) if user_tile_start else (tuple(int(v) for v in mt.start_tile) if mt.start_tile is not None else None)
        sp = mt.start_pose
        pose = None if sp is None else (float(sp[0][0]), float(sp[0][2]), float(sp[1]))
        return cls(bool(domain_rand), bool(dynamics_rand), accept_start_angle_deg=float(accept_start_angle_deg), start_tile=tile, start_pose=pose, **kw)

    @classmethod
    def from_ffi(cls, rs, map_id=0):
        """from an installed _ffi.ResetSampler"""
        tile = (int(rs.start_tile[map_id][0]), int(rs.start_tile[map_id][1]))
        pose = tuple(float(v) for v in rs.start_pose[map_id]) if rs.has_start_pose[map_id] else None
        return cls(bool(rs.domain_rand), bool(rs.dynamics_rand), int(rs.max_attempts), float(rs.accept_start_angle_deg), tuple(rs.color_sky),
                   tuple(rs.color_ground), tile if tile[0] >= 0 else None, pose)


HORIZON_MODES = [(None, 0.1), ((0.64, 0.71, 0.28), 0.1), ((0.15, 0.15, 0.15), 0.4), ((0.9, 0.9, 0.9), 0.4)]   # None: color_sky


def _perturb3(g, v, scale):
    """_perturb (simulator.py:1065-1085): v[k] * U(1 - scale, 1 + scale); v: [3] or [E, 3], scale: scalar or [E]"""
    v = np.broadcast_to(np.asarray(v, np.float64), (g.env.size, 3))
    lo, hi = 1.0 - np.asarray(scale, np.float64), 1.0 + np.asarray(scale, np.float64)
    return np.stack([v[:, k] * (lo + (hi - lo) * g.double()) for k in range(3)], axis=1)


def sample_reset(seed, env, episode, map_tables, sampler_cfg, camera_rand=False):
    """sample_init for the envs of `env` (array) at `episode` (scalar or array).  Returns a dict of [E, ...] arrays:
      cam [E,6] f4, colors [E,16] f4, wheel_dist, trim, war, wal (f8), horz_mode, visible [E, n_obj] u1, tile [E,2],
      fixed_pose ((x, z, angle) [E,3] or None: the map's start_pose), words [E]: words consumed before the spawn loop,
      candidates(k0, k1) -> [E, k1 - k0, 3]: spawn candidates (x, z, angle) k0 .. k1 - 1 as the stream yields them, stream: the Stream."""
    mt, cfg = map_tables, sampler_cfg
    g = Stream(seed, env, episode)
    E, dr = g.env.size, bool(cfg.domain_rand)
    f_angle, f_fov, f_height = g.uniform(0.8, 1.2), g.uniform(0.8, 1.2), g.uniform(0.92, 1.08)          # 1. camera factors
    noise = np.stack([g.uniform(-0.005, 0.005) for _ in range(3)], axis=1)                              # 2. camera noise
    horz = g.below(4)                                                                                   # 3. horz_mode
    lp = np.stack([g.uniform(-150, 150), g.uniform(170, 220), g.uniform(-150, 150)], axis=1)            # 4. light position
    trim = g.normal(0.0, 0.02)                                                                          # 5. trim
    sky, gnd = np.array(cfg.color_sky, np.float64), np.array(cfg.color_ground, np.float64)
    if dr:                                                                                              # 6. colours by _perturb
        base = np.stack([np.broadcast_to(sky if b is None else np.array(b), (3,)) for b, _ in HORIZON_MODES])[horz]
        horizon = _perturb3(g, base, np.array([s for _, s in HORIZON_MODES])[horz])
        light = np.concatenate([lp, np.zeros((E, 1))], axis=1)
        ambient, diffuse, ground = _perturb3(g, [0.25] * 3, 0.3), _perturb3(g, [0.35] * 3, 0.99), _perturb3(g, gnd, 0.3)
        wheel_dist = 0.102 * g.uniform(0.9, 1.1)                                                        # 7. wheel distance
    else:
        horizon, light = np.broadcast_to(sky, (E, 3)), np.broadcast_to(np.array([0.0, 3.0, 0.0, 1.0]), (E, 4))
        ambient, diffuse, ground = (np.broadcast_to(np.array(v, np.float64), (E, 3)) for v in ([0.25] * 3, [0.35] * 3, gnd))
        wheel_dist = np.full(E, 0.102)
    scale_cam = dr or bool(camera_rand)
    one = np.ones(E)
    rad = 3.141592653589793 / 180.0
    cam = np.stack([0.108 * (f_height if scale_cam else one), (19.15 * (f_angle if scale_cam else one)) * rad,
                    (75.0 * (f_fov if scale_cam else one)) * rad], axis=1)
    if camera_rand and not dr:
        noise = np.zeros_like(noise)
    dyn = bool(cfg.dynamics_rand)
    out = {"cam": np.concatenate([cam, noise], axis=1).astype(np.float32),
           "colors": np.concatenate([horizon, ground, ambient, diffuse, light], axis=1).astype(np.float32),
           "wheel_dist": wheel_dist, "trim": trim, "horz_mode": horz,
           "war": 15.0 * (1.0 + trim) if dyn else np.full(E, 15.0), "wal": 15.0 * (1.0 - trim) if dyn else np.full(E, 15.0)}
    # 8. optional objects (a dynamic object's slot word is its slot: never optional on the device)
    vis = np.ones((E, len(mt.objects)), np.uint8)
    for o, ob in enumerate(mt.objects):
        if ob.optional and ob.dyn_slot < 0 and dr:
            vis[:, o] = g.below(2) == 0
    out["visible"] = vis
    # 9. start tile: uniform over the drivable tiles by rejection over rng_below(n_tiles)
    if cfg.start_tile is not None:
        ti, tj = np.full(E, cfg.start_tile[0], np.int64), np.full(E, cfg.start_tile[1], np.int64)
    else:
        drivable = np.zeros(mt.grid_w * mt.grid_h, bool)
        for i, j in mt.drivable_tiles:
            drivable[j * mt.grid_w + i] = True
        t_of, open_ = np.full(E, -1, np.int64), np.ones(E, bool)
        for _ in range(TILE_TRIES):
            if not open_.any():
                break
            t = g.below(mt.grid_w * mt.grid_h, open_)
            hit = open_ & drivable[t]
            t_of[hit], open_ = t[hit], open_ & ~hit
        ti, tj = np.where(t_of >= 0, t_of % mt.grid_w, 0), np.where(t_of >= 0, t_of // mt.grid_w, 0)
    out["tile"] = np.stack([ti, tj], axis=1)
    out["words"], out["stream"] = g.pos.copy(), g
    ts = np.float64(mt.tile_size)
    out["fixed_pose"] = None
    if cfg.start_pose is not None:                                # no rejection loop, no further draws
        sp = cfg.start_pose
        out["fixed_pose"] = np.stack([ti * ts + sp[0], tj * ts + sp[1], np.full(E, sp[2])], axis=1)
    p0 = g.pos.copy()
    fi, fj = ti.astype(np.float64), tj.astype(np.float64)

    def candidates(k0, k1):                                       # 10. (x, z, angle) of attempts k0 .. k1 - 1
        g.ensure(int(p0.max()) + 6 * k1)
        idx = p0[:, None, None] + 6 * np.arange(k0, k1)[None, :, None] + np.arange(6)[None, None, :]
        w = g.words[np.arange(E)[:, None, None], idx]
        u = ((w[..., 0::2] >> U(5)).astype(np.float64) * 67108864.0 + (w[..., 1::2] >> U(6)).astype(np.float64)) / 9007199254740992.0
        x = (fi[:, None] + ((fi[:, None] + 1.0) - fi[:, None]) * u[..., 0]) * ts
        z = (fj[:, None] + ((fj[:, None] + 1.0) - fj[:, None]) * u[..., 1]) * ts
        return np.stack([x, z, 0.0 + (TWO_PI - 0.0) * u[..., 2]], axis=2)
    out["candidates"] = candidates
    return out


# ---------------------------------------------------------------- c. object and map streams --
def create_duckie(seed, env, episode, slot, domain_rand, create_event=OBJ_EVENT_CREATE):
    """DuckieObj.__init__ with the sampler installed (apply_init, kind 1): (vel, wait, wiggle, stream); vel and wait None without
    domain randomisation (the map's values stay), the wiggle is always drawn"""
    g = Stream(seed, env, episode, create_event, TAG_OBJECT + slot)
    wait = vel = None
    if domain_rand:
        wait = (3 + g.below(17)).astype(np.float64)
        vel = np.abs(g.normal(0.02, 0.005))
    wiggle = 3.141592653589793 / (14 + g.below(3)).astype(np.float64)
    return vel, wait, wiggle, g


def create_duckiebot(seed, env, episode, slot, gain=2.0, trim=0.0, create_event=OBJ_EVENT_CREATE):
    """DuckiebotObj.__init__ under domain randomisation (apply_init, kind 2): FIELD_OBJ_PARAMS (vel, wait = gain, wiggle = trim) and the
    five FIELD_OBJ_EXTRA words, and the stream"""
    g = Stream(seed, env, episode, create_event, TAG_OBJECT + slot)
    follow, vel = g.uniform(0.3, 0.4), g.uniform(0.05, 0.15)
    wait, wiggle = gain + g.uniform(-0.3, 0.3), trim + g.uniform(-0.1, 0.1) + 2
    ext = [follow, 0.0318 + 0.0002 * g.uniform(-1.0, 1.0), 0.102 + 0.01 * g.uniform(-1.0, 1.0), (0.13 + 0.02) + 0.01 * g.uniform(-1.0, 1.0),
           0.18 + 0.01 * g.uniform(-1.0, 1.0)]
    return np.stack([vel, wait, wiggle], axis=1), np.stack(ext, axis=1), g


def finish_walk(seed, env, episode, slot, step_count, vel_before):
    """duckie_step's redraw under domain randomisation at the step_count where the walk ended: (vel, wait, stream)"""
    g = Stream(seed, env, episode, obj_event_walk(step_count), TAG_OBJECT + slot)
    mag = np.abs(g.normal(0.02, 0.005))
    vel_before = np.asarray(vel_before, np.float64)
    vel = np.where(vel_before > 0, -mag, np.where(vel_before < 0, mag, -0.0 * mag))
    return vel, (3 + g.below(17)).astype(np.float64), g


def next_map(seed, env, episode, n_maps):
    """sampler_next_map for map_cycle == 2: (map id, stream)"""
    g = Stream(seed, env, episode, 0, TAG_MAP)
    return g.below(n_maps), g


WORDS = {"create_duckie": 6, "create_duckie_no_dr": 1, "create_duckiebot": 16, "walk": 5, "map": 1}


def blocks_used(event, create_event=OBJ_EVENT_CREATE):
    """the counter blocks (ctr0, ctr1) of one event of an env's episode:
      ("reset", n_words)            the reset stream, n_words deep (sample_reset's `words` + 6 per spawn attempt)
      ("map",)                      the map draw
      ("create", slot, kind)        the creation stream of a kind 1 (domain-randomised DuckieObj) or kind 2 (DuckiebotObj) object
      ("walk", slot, step_count)    finish_walk's redraw
    The word counts are WORDS, which tests/test_reset_sampler_model_host.py holds to what the streams above consume."""
    if event[0] == "reset":
        return stream_blocks(0, 0, event[1])
    if event[0] == "map":
        return stream_blocks(0, TAG_MAP, WORDS["map"])
    if event[0] == "create":
        return stream_blocks(create_event, TAG_OBJECT + event[1], WORDS["create_duckie" if event[2] == 1 else "create_duckiebot"])
    if event[0] == "walk":
        return stream_blocks(obj_event_walk(event[2]), TAG_OBJECT + event[1], WORDS["walk"])
    raise ValueError(event)
