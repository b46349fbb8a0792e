"""GPU: a setter that returns an error leaves the handle as it was (include/dtsim.h).  A dtsim_set_assets rejected for a mesh that names a
missing texture, or for a texture that is not a power of two, keeps the installed textures, meshes and quad records: the next pass takes
the same raster and writes the same bytes, and segment assets that mirror the installed list are still accepted.  A rejected
dtsim_set_maps keeps the maps.  A dtsim_set_assets that succeeds on a handle with maps leaves them to physics only: the render entry
points return DTSIM_E_STATE, on the host and ahead of any launch, until dtsim_set_maps packs the maps against the new assets."""
import ctypes as C

import numpy as np
import pytest

from dtsim import BatchedSimulator, _ffi, batched

pytestmark = pytest.mark.gpu

N, W, H = 8, 160, 120


def _sim():
    sim = BatchedSimulator("small_loop", N, camera_width=W, camera_height=H, domain_rand=False, distortion=False, seed=5,
                           max_steps=100000, action_mode="vel_steer")
    sim.step(np.random.default_rng(0).uniform(0.2, 0.8, (3, N, 2)).astype(np.float32), n_steps=3)
    return sim


def _render(sim, **kw):
    sim.render(**kw)
    return sim.render_pipeline, sim.frames_host().copy()


def _set_assets(sim, textures, meshes=()):
    tarr = (_ffi.Texture * max(len(textures), 1))()
    for i, t in enumerate(textures):
        tarr[i].width, tarr[i].height = t.shape[1], t.shape[0]
        tarr[i].rgba = t.ctypes.data_as(C.POINTER(C.c_uint8))
    marr = (_ffi.Mesh * max(len(meshes), 1))()
    for i, m in enumerate(meshes):
        marr[i].n_tris = len(m["tri_tex"])
        for k in ("verts", "normals", "colors", "uvs"):
            setattr(marr[i], k, m[k].ctypes.data_as(C.POINTER(C.c_float)))
        marr[i].tri_tex = m["tri_tex"].ctypes.data_as(C.POINTER(C.c_int32))
    return sim._lib.dtsim_set_assets(sim._h, tarr, len(textures), marr, len(meshes))


def test_rejected_mesh_keeps_the_assets():
    sim = _sim()
    pipe, frames = _render(sim)
    assert pipe == "k_raster_v3"
    one = lambda n: np.full(n, 0.5, np.float32)
    mesh = dict(verts=one(9), normals=one(9), colors=one(9), uvs=one(6), tri_tex=np.array([len(sim.textures)], np.int32))
    assert _set_assets(sim, sim.textures, [mesh]) == _ffi.E_INVALID
    assert _render(sim)[0] == pipe
    assert np.array_equal(sim.frames_host(), frames)
    sim.close()


def test_rejected_texture_keeps_the_assets():
    sim = _sim()
    pipe, frames = _render(sim)
    seg_pipe, seg_frames = _render(sim, segment=True)
    assert _set_assets(sim, [np.zeros((100, 100, 4), np.uint8)] + sim.textures[1:]) == _ffi.E_INVALID
    sim._install_segment_assets()                          # the installed assets' mirror: raises unless accepted
    assert _render(sim, segment=True)[0] == seg_pipe
    assert np.array_equal(sim.frames_host(), seg_frames)
    assert _render(sim)[0] == pipe
    assert np.array_equal(sim.frames_host(), frames)
    sim.close()


def _product_map(sim):
    return sim.maps[0].to_ffi({mk: i for i, mk in enumerate(sim._mesh_order)}, sim.light_tex)


def _unloaded_tile_texture(sim):
    m = _product_map(sim)
    tex = sim.maps[0].tile_tex.copy()
    tex[np.flatnonzero(tex >= 0)[-1]] = len(sim.textures)
    m.tile_tex = tex.ctypes.data_as(C.POINTER(C.c_int16))
    return [m], tex, _ffi.E_INVALID, "texture %d not loaded" % len(sim.textures)


def _too_many_static_collidables(sim):
    m = _product_map(sim)
    objs = (_ffi.Object * 57)()
    for o in objs:
        o.mesh_id, o.collidable, o.scale = -1, 1, 1.0
    m.n_objects, m.objects = 57, C.cast(objs, C.POINTER(_ffi.Object))
    return [m], objs, _ffi.E_LIMIT, "57 static collidables > 56"


def _blob_over_the_lds_budget(sim):
    m = _product_map(sim)                                  # 8 maps of 32 x 32 undrivable tiles: 8 x 1024 tile words alone are 64 KB
    keep = [np.full(1024, 7, np.uint8), np.zeros(1024, np.uint8), np.zeros(1024, np.int16), np.full(1024, -1, np.int16)]
    m.grid_w = m.grid_h = 32
    m.tile_kind, m.tile_angle = (a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in keep[:2])
    m.tile_curve_cnt = m.tile_angle
    m.tile_tex, m.tile_curve_off = (a.ctypes.data_as(C.POINTER(C.c_int16)) for a in keep[2:])
    m.n_objects = 0
    return [m] * 8, keep, _ffi.E_LIMIT, "exceed the 60 KB LDS staging budget"


@pytest.mark.parametrize("bad", [_unloaded_tile_texture, _too_many_static_collidables, _blob_over_the_lds_budget])
def test_rejected_maps_keep_the_maps(bad):
    sim = _sim()
    pipe, frames = _render(sim)
    assert pipe == "k_raster_v3"
    acts = np.random.default_rng(1).uniform(0.2, 0.8, (2, N, 2)).astype(np.float32)
    fields = (_ffi.FIELD_POS, _ffi.FIELD_ANGLE, _ffi.FIELD_REWARD, _ffi.FIELD_DONE, _ffi.FIELD_TILE, _ffi.FIELD_LANE)
    blob = sim.read(_ffi.FIELD_STATE_BLOB)
    sim.step(acts, n_steps=2)
    want = [sim.read(f) for f in fields]
    sim.write(_ffi.FIELD_STATE_BLOB, blob)
    maps, keep, code, msg = bad(sim)
    assert sim._lib.dtsim_set_maps(sim._h, (_ffi.Map * len(maps))(*maps), len(maps)) == code
    assert msg in sim._lib.dtsim_last_error().decode()
    assert _render(sim)[0] == pipe
    assert np.array_equal(sim.frames_host(), frames)
    sim.step(acts, n_steps=2)
    for f, w in zip(fields, want):
        assert np.array_equal(sim.read(f), w), f
    sim.close()


@pytest.mark.parametrize("map_name", ["small_loop", "loop_pedestrians"])
def test_new_assets_wait_for_the_maps(map_name):
    kw = dict(camera_width=W, camera_height=H, domain_rand=False, distortion=False, seed=5, max_steps=100000, action_mode="vel_steer")
    fresh = BatchedSimulator(map_name, N, **kw)
    fresh_pipe, fresh_frames = _render(fresh)
    sim = BatchedSimulator(map_name, N, **kw)
    acts = np.random.default_rng(0).uniform(0.2, 0.8, (3, N, 2)).astype(np.float32)
    sim.step(acts, n_steps=3)
    sim.render(segment=True)
    sim.render()
    lib, h = sim._lib, sim._h
    assert _set_assets(sim, sim.textures) == _ffi.OK      # the same textures and no meshes: the maps' objects name meshes that are gone
    one = np.zeros(9, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    for call in (lambda: lib.dtsim_render(h), lambda: lib.dtsim_render_ex(h, _ffi.RENDER_SEGMENT), lambda: lib.dtsim_draw_lines(h, one, None, 1),
                 lambda: lib.dtsim_draw_leds(h, one, None, 1)):
        assert call() == _ffi.E_STATE
    assert lib.dtsim_render(h) == _ffi.E_STATE
    msg = lib.dtsim_last_error().decode()
    assert "dtsim_set_assets" in msg and "dtsim_set_maps" in msg
    sim.step(acts, n_steps=3)                             # physics, read and query go on from the map blobs
    pos = sim.read(_ffi.FIELD_POS)
    assert np.isfinite(pos).all() and np.isfinite(sim.read(_ffi.FIELD_REWARD)).all()
    poses = np.stack([pos[:, 0], pos[:, 2], sim.read(_ffi.FIELD_ANGLE)], axis=1)
    pr, want = sim.query(np.arange(N), poses), fresh.query(np.arange(N), poses)
    for k in ("tile_i", "tile_j", "curve_idx", "drivable", "dist", "dot_dir", "angle_deg"):   # the map geometry, not the env's objects
        assert np.array_equal(pr[k], want[k]), k
    sc = batched.load_scene(sim.library, sim.map_names, sim.map_datas)
    tarr, marr, farr, keep = batched.scene_ffi(sc)
    assert lib.dtsim_set_assets(h, tarr, len(sc.textures), marr, len(sc.mesh_order)) == _ffi.OK
    assert lib.dtsim_render(h) == _ffi.E_STATE
    assert lib.dtsim_set_maps(h, farr, len(sc.maps)) == _ffi.OK
    sim.reset(states=fresh.init_states)
    pipe, frames = _render(sim)
    assert pipe == fresh_pipe and np.array_equal(frames, fresh_frames)
    fresh.close()
    sim.close()
