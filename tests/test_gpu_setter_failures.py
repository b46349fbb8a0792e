"""GPU: a setter that returns an error leaves the handle as it was (include/dtsim.h).  A dtsim_set_assets rejected for a mesh that names a
missing texture, or for a texture that is not a power of two, keeps the installed textures, meshes and quad records: the next pass takes
the same raster and writes the same bytes, and segment assets that mirror the installed list are still accepted."""
import ctypes as C

import numpy as np
import pytest

from dtsim import BatchedSimulator, _ffi

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
