"""GPU: the render order (k_env_sort) and the quad-record rasters behind it at batches past 8192 envs and at chunk counts that leave most
of the workgroup map (raster_wg / raster_wg_grid) padding.

The batches replicate the states of tests/render_order_scenes.py -- half of them ON a border of the sort key, where two float32
evaluations of bin_of may differ -- by its layout, which puts border states on the path that computes the bin twice (slots >= 8192) and in the
last chunks.  Per pipeline and batch size:

  order     DTSIM_FIELD_RENDER_POS is a permutation, and along it the keys of the clear envs never decrease (the host key is exact for them)
  written   the frame batch is filled with a per-env sentinel before the pass; afterwards every replica's frame equals that of its state's
            first replica byte for byte, and no frame holds its sentinel over a whole raster tile row -- a (tile, chunk) that no workgroup
            took, or a position that two envs shared, shows here
  oracle    six states (two clear, two on a tile border, one on a quadrant border, one off the grid), from slots on both sides of
            8192, against the oracle at the pipeline's row of tests/frame_parity.py
  again     a second pass from the same state gives the same bytes
  masked    (N = 8193, 9217) the masks of tests/test_gpu_masked_render.py, plus the slots >= 8192 alone and the border states' replicas alone
  two maps  (N = 8193, the object forms) both *_only_duckies maps over alternating slots: the map term of the key

The frames are 128 x 48 (six 128 x 8 raster tiles, 18 KB per env: 16385 envs are 300 MB); all frame comparisons run on the device.
The oracle comparison alone renders the batch again at 160 x 120: at 128 x 48 the oracle's own float32 headroom holds
(tests/test_render_order_scenes_host.py), but a frame that low is road from edge to edge in some states, and the byte-weight filter of the
shared-camera rasters is off by one on 2 - 3 % of the textured channel values (tests/test_crowd_scenes_host.py) -- measured over all 96
states at 128 x 48: mean 0.0246 (k_raster_v3, k_raster_q) and 0.0471 (+light) in the worst state against the row's 0.02, beyond +-2 within
the row; at 160 x 120 every state of every pipeline is within its row (worst mean 0.0081).  The row stays as it is."""
import ctypes as C

import numpy as np
import pytest

import frame_parity as fp
import render_order_scenes as ro
from dtsim import BatchedSimulator, _ffi
from dtsim import distortion as pdist
from dtsim import reset as R
from test_gpu_masked_render import MASKS, PIPELINES as MASKED_PIPELINES, make_mask

pytestmark = pytest.mark.gpu

W, H = 128, 48                                         # the smallest camera tried: every pipeline below still reports itself at it
ORACLE_SIZE = ro.ORACLE_SIZE                           # the camera of the oracle comparison
assert W % ro.TILE_W == 0                              # a tile row is a whole run of a frame row
PIPELINES = {k: v for k, v in MASKED_PIPELINES.items() if k != "generic_segment"}       # (the generic raster renders in env order)
ROWS = {"small_loop": fp.ORACLE_PLANE, "small_loop_only_duckies": fp.ORACLE_MESH}
TWO_MAPS = ["loop_only_duckies", "small_loop_only_duckies"]
K = ro.N_STATES
SENTINEL_STEP = 7                                      # env e's sentinel: bytes [7 e, 7 e + F) of one seeded random sequence


def _templates(sim, n_maps):
    """[K * n_maps, sizeof(InitState)] bytes: state s on map m at row s * n_maps + m, with reset()'s draws of a seeded env (colours, light and
    camera of domain randomisation where the handle has it) and the pose of the state list."""
    out = (_ffi.InitState * (K * n_maps))()
    for s in range(K):
        for m in range(n_maps):
            st, _, _ = R.draw_prefix(R.EnvResetState(ro.SEED + s), sim.maps[m], domain_rand=sim.domain_rand, camera_rand=False, dynamics_rand=False,
                                     color_sky=sim.color_sky, color_ground=sim.color_ground, num_tris_distractors=sim.num_tris_distractors,
                                     n_visible_draw=(), user_tile_start=None)
            st.pos[:] = [float(ro.X[s]), 0.0, float(ro.Z[s])]
            st.angle, st.map_id = float(ro.A[s]), m
            out[s * n_maps + m] = st
    return np.frombuffer(out, dtype=np.uint8).reshape(K * n_maps, C.sizeof(_ffi.InitState)).copy()


class Batch:
    """N envs of a pipeline at the states of the list: slot e holds state lay[e] (on map e % n_maps), written through a host-fed reset."""

    def __init__(self, pipe, N, monkeypatch, maps=None, size=(W, H)):
        import torch
        self.W, self.H = size
        self.F = self.W * self.H * 3
        map_name, kw, _, self.want, old = PIPELINES[pipe]
        if old:
            monkeypatch.setenv("DTSIM_RASTER_OLD", old)
        self.pipe, self.N, self.map_name = pipe, N, map_name
        self.n_maps = len(maps) if maps else 1
        self.sim = sim = BatchedSimulator(maps or map_name, N, camera_width=self.W, camera_height=self.H, distortion=True, seed=ro.SEED, max_steps=100000,
                                          do_reset=False, **kw)
        self.lay = ro.layout(N)
        self.mid = np.arange(N) % self.n_maps
        self.group = self.lay * self.n_maps + self.mid                                  # replicas: same state, same map
        states = (_ffi.InitState * N).from_buffer_copy(_templates(sim, self.n_maps)[self.group].tobytes())
        sim.reset(states=states)
        if sim.light_capture:                          # a light of its own per state, so that the per-position light records differ
            col = sim.read(_ffi.FIELD_COLORS).copy()
            s = self.lay.astype(np.float64)
            col[:, 12:16] = np.stack([0.6 * np.cos(0.7 * s), 2.0 + 0.02 * s, 0.6 * np.sin(0.7 * s), np.ones(N)], axis=1)
            sim.write(_ffi.FIELD_COLORS, col)
        pos, ang = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE)
        assert np.array_equal(pos[:, 0], ro.X[self.lay]) and np.array_equal(pos[:, 2], ro.Z[self.lay]) and np.array_equal(ang, ro.A[self.lay])
        assert np.array_equal(sim.read(_ffi.FIELD_MAP_ID), self.mid)
        self.key = ro.host_key(ro.X[self.lay], ro.Z[self.lay], ro.A[self.lay], self.mid)
        self.clear = ~ro.BORDER[self.lay]
        self.dev = torch.device(f"cuda:{sim.device_index}")
        self.frames = torch.as_tensor(sim.frames_device(), device=self.dev).view(N, self.F)
        g = torch.Generator().manual_seed(ro.SEED)
        self.sentinel = torch.randint(0, 256, (self.F + SENTINEL_STEP * N,), dtype=torch.uint8, generator=g).to(self.dev).as_strided((N, self.F), (SENTINEL_STEP, 1))
        groups, first = np.unique(self.group, return_index=True)
        self.first = np.full(K * self.n_maps, -1, np.int64)
        self.first[groups] = first                     # group -> its first slot (-1: a batch with fewer slots than states)
        self.first_of = torch.as_tensor(self.first[self.group], device=self.dev)

    def fill(self):
        import torch
        self.sim.sync()
        self.frames.copy_(self.sentinel)
        torch.cuda.synchronize(self.dev)               # (the library's stream does not wait for torch's)

    def render(self, mask=None):
        """One pass; (a copy of the frame batch [N, F] on the device, the order)."""
        import torch
        self.sim.render(mask=None if mask is None else torch.as_tensor(mask, device=self.dev))
        assert self.sim.render_pipeline == self.want, (self.pipe, self.N, self.sim.render_pipeline)
        self.sim.sync()
        return self.frames.clone(), self.sim.read(_ffi.FIELD_RENDER_POS).copy()

    def where(self, e, row, rpos):
        """An env and a frame row, for a message: (env, state, kind, position, chunk, raster tile)."""
        p = int(rpos[e])
        return dict(env=int(e), state=int(self.lay[e]), kind=str(ro.KIND[self.lay[e]]), position=p, chunk=p // ro.ENVS_PER_CHUNK,
                    tile=int(row) // ro.TILE_H * (self.W // ro.TILE_W))

    def first_difference(self, a, b, rows, rpos):
        """None if a == b on the envs `rows` (bool [N] on the host, or None: all), else where() of the first byte that differs."""
        import torch
        bad = (a != b).any(dim=1)
        if rows is not None:
            bad &= torch.as_tensor(rows, device=self.dev)
        if not bool(bad.any()):
            return None
        e = int(torch.nonzero(bad)[0])
        byte = int(torch.nonzero(a[e] != b[e])[0])
        return self.where(e, byte // (self.W * 3), rpos), f"{int(bad.sum())} envs differ"

    def stale(self, fr, rows, rpos):
        """None if no frame of the envs `rows` holds its sentinel over a whole raster tile row, else where() of the first such row."""
        import torch
        run = (fr == self.sentinel).view(self.N, self.H, self.W // ro.TILE_W, ro.TILE_W * 3).all(dim=3).any(dim=2)       # [N, H]
        if rows is not None:
            run &= torch.as_tensor(rows, device=self.dev)[:, None]
        if not bool(run.any()):
            return None
        e, y = (int(v) for v in torch.nonzero(run)[0])
        return self.where(e, y, rpos), f"{int(run.any(dim=1).sum())} envs hold sentinel rows, {int(run.sum())} rows in all"

    def check_full_pass(self):
        """order + written, for a full pass over a sentinel-filled batch; (frames, order)."""
        self.fill()
        fr, rpos = self.render()
        if self.N > ro.ENVS_PER_CHUNK:
            assert not np.array_equal(rpos, np.arange(self.N))                          # the sorted order is in use
        assert ro.order_fault(rpos, self.key, self.clear) is None, (self.pipe, self.N, ro.order_fault(rpos, self.key, self.clear))
        assert self.stale(fr, None, rpos) is None, (self.pipe, self.N, "sentinel left", self.stale(fr, None, rpos))
        d = self.first_difference(fr, fr[self.first_of], None, rpos)
        assert d is None, (self.pipe, self.N, "a replica differs from its state's first replica", d)
        return fr, rpos

    def close(self):
        del self.frames, self.sentinel
        self.sim.close()


def _oracle_slots(b):
    """The slots of the six compared states: the first replica of three, and of the others the first replica past slot 8192 (the last
    replica in a batch that has none there)."""
    out = []
    for i, s in enumerate(ro.ORACLE_STATES):
        slots = np.flatnonzero(b.lay == s)
        if not len(slots):
            continue                                   # (N = 65: a batch with fewer slots than states)
        past = slots[slots >= ro.KEEP_ENVS]
        out.append(int(slots[0] if i % 2 == 0 else (past[0] if len(past) else slots[-1])))
    return out


CASES = [(p, n) for p in PIPELINES for n in ro.BATCH_SIZES]          # (every size on every pipeline: the largest case takes about a second)


@pytest.mark.parametrize("pipe,N", CASES, ids=[f"{p}-{n}" for p, n in CASES])
def test_every_frame_is_written_once_in_the_sorted_order(pipe, N, monkeypatch):
    b = Batch(pipe, N, monkeypatch)
    try:
        fr, rpos = b.check_full_pass()
        # again: the order may differ, the frames may not
        again, rpos2 = b.render()
        assert ro.order_fault(rpos2, b.key, b.clear) is None, (pipe, N, "second pass", ro.order_fault(rpos2, b.key, b.clear))
        d = b.first_difference(again, fr, None, rpos2)
        assert d is None, (pipe, N, "the second pass differs", d)
    finally:
        b.close()
    # against the oracle, at ORACLE_SIZE (the module's docstring): the same batch with a larger camera
    b = Batch(pipe, N, monkeypatch, size=ORACLE_SIZE)
    try:
        import torch
        b.sim.render()
        assert b.sim.render_pipeline == b.want, (pipe, N, b.sim.render_pipeline)
        b.sim.sync()
        rpos = b.sim.read(_ffi.FIELD_RENDER_POS)
        assert ro.order_fault(rpos, b.key, b.clear) is None, (pipe, N, ORACLE_SIZE, ro.order_fault(rpos, b.key, b.clear))
        slots = _oracle_slots(b)
        if N >= ro.KEEP_ENVS + K:                      # (8193: the one slot past 8192 holds state 0)
            assert min(slots) < ro.KEEP_ENVS <= max(slots)
        picked = b.frames[torch.as_tensor(slots, device=b.dev)].cpu().numpy().reshape(len(slots), b.H, b.W, 3)
        colors = b.sim.read(_ffi.FIELD_COLORS) if b.sim.light_capture else None
        worst, _ = fp.compare_envs(b.sim, picked, slots, fp.scene(b.map_name), pdist.distortion_maps(b.W, b.H), ROWS[b.map_name], dr=b.sim.domain_rand,
                                   colors=colors)
        assert len({picked[i].tobytes() for i in range(len(slots))}) == len(slots) and picked.std() > 10.0     # views, and each its own
        print(f"{pipe} N={N} ({-(-N // 64)} chunks): order exact on {int(b.clear.sum())} clear envs, {int((~b.clear).sum())} border envs placed; "
              f"{len(slots)} envs (slots {slots}, positions {rpos[slots].tolist()}) against the oracle: worst {worst}")
    finally:
        b.close()


MASKED_SIZES = (8193, 9217)


def _mask(kind, b):
    if kind == "past_8192":
        return np.arange(b.N) >= ro.KEEP_ENVS
    if kind == "border":
        return ro.BORDER[b.lay].copy()
    return make_mask(kind, b.N)


@pytest.mark.parametrize("N", MASKED_SIZES)
@pytest.mark.parametrize("pipe", list(PIPELINES))
def test_masked_passes_past_8192_envs(pipe, N, monkeypatch):
    b = Batch(pipe, N, monkeypatch)
    try:
        full, _ = b.check_full_pass()
        for kind in MASKS + ("past_8192", "border"):
            m = _mask(kind, b)
            b.fill()
            fr, rpos = b.render(mask=m)
            ctx = (pipe, N, kind, int(m.sum()))
            assert ro.order_fault(rpos, b.key, b.clear, m) is None, (ctx, ro.order_fault(rpos, b.key, b.clear, m))
            d = b.first_difference(fr, full, m, rpos)
            assert d is None, (ctx, "a selected frame differs from the full pass's", d)
            d = b.first_difference(fr, b.sentinel, ~m, rpos)
            assert d is None, (ctx, "an unselected frame lost its sentinel", d)
    finally:
        b.close()


@pytest.mark.parametrize("pipe", ["v3_obj", "v3dr_obj"])
def test_two_maps_past_8192_envs(pipe, monkeypatch):
    N = 8193
    b = Batch(pipe, N, monkeypatch, maps=TWO_MAPS)
    try:
        assert set(np.unique(b.key ^ ro.host_key(ro.X[b.lay], ro.Z[b.lay], ro.A[b.lay]))) == {0, 1237}       # the map term is in the key
        fr, rpos = b.check_full_pass()
        again, rpos2 = b.render()
        assert ro.order_fault(rpos2, b.key, b.clear) is None
        d = b.first_difference(again, fr, None, rpos2)
        assert d is None, (pipe, "the second pass differs", d)
        # the two maps show: a state's two groups render different frames somewhere
        f0, f1 = b.first[0::2], b.first[1::2]
        import torch
        differ = (fr[torch.as_tensor(f0, device=b.dev)] != fr[torch.as_tensor(f1, device=b.dev)]).any(dim=1)
        assert int(differ.sum()) > K // 2, int(differ.sum())
    finally:
        b.close()
