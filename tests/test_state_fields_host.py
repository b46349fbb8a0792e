"""The per-env state of csrc/state_fields.h on this CPU: the slab layout behind dtsim_create (the checkpoint format of
DTSIM_FIELD_STATE_BLOB) and the table of public fields behind dtsim_read / dtsim_write / dtsim_field_devptr, compiled with g++ behind a
test-only extern "C" wrapper.  The test holds its own statement of both: ARRAYS, the 47 arrays in slab order, and FIELDS, the array and
plane of every public component.  A host buffer stands in for the slab."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dtsim import _ffi
from dtsim.batched import BatchedSimulator

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gym-duckietown_amd", "csrc")
DYN, OBJ, DELAY = 8, 64, 16                                   # DTSIM_MAX_DYNAMIC, DTSIM_MAX_OBJECTS, DTSIM_MAX_DELAY
assert (DYN, OBJ, DELAY) == (_ffi.MAX_DYNAMIC, _ffi.MAX_OBJECTS, _ffi.MAX_DELAY)

# (name, dtype, planes of [N]) in slab order; every array starts on the next multiple of 256 bytes
ARRAYS = [(n, "f8", 1) for n in ("pos_x", "pos_z", "angle", "q_x", "q_y", "q_c", "q_s", "vel_u", "vel_w")] + [("ring", "f8", DELAY * 2)] + \
    [(n, "f8", 1) for n in ("war", "wal", "wheel_dist", "timestamp", "speed", "reward")] + [("lane", "f8", 4), ("prox", "f8", 1), ("wheels", "f8", 2)] + \
    [(n, "f8", DYN) for n in ("ob_cx", "ob_cz", "ob_sx", "ob_sz")] + [("ob_corners", "f8", DYN * 8)] + \
    [(n, "f8", DYN) for n in ("ob_vel", "ob_wait", "ob_time", "ob_angle", "ob_wiggle", "ob_yrot")] + [("cam", "f4", 6), ("colors", "f4", 16)] + \
    [(n, "i4", 1) for n in ("ring_head", "step_count", "tile_i", "tile_j", "map_id", "episode")] + [(n, "u1", 1) for n in ("done", "done_code", "in_lane")] + \
    [("ob_active", "u1", DYN), ("ob_visible", "u1", OBJ), ("ob_light", "u1", OBJ), ("tl_time", "f8", 1), ("ob_cy", "f8", DYN), ("ob_ext", "f8", DYN * 5)]
SLAB_BYTES = {1: 12544, 33: 82944, 64: 143104, 65: 154880, 4096: 9121792}       # the parent commit's dtsim_state_bytes


def run(name, comps):
    return [(name, c) for c in range(comps)]


# field -> (array, plane) of each public component in [N][...] order; None: no array (reads 0, ignores writes)
F = _ffi
FIELDS = {
    F.FIELD_POS: [("pos_x", 0), None, ("pos_z", 0)], F.FIELD_ANGLE: run("angle", 1), F.FIELD_REWARD: run("reward", 1), F.FIELD_DONE: run("done", 1),
    F.FIELD_DONE_CODE: run("done_code", 1), F.FIELD_STEP_COUNT: run("step_count", 1), F.FIELD_TILE: [("tile_i", 0), ("tile_j", 0)],
    F.FIELD_LANE: run("lane", 4), F.FIELD_IN_LANE: run("in_lane", 1), F.FIELD_PROX: run("prox", 1), F.FIELD_SPEED: run("speed", 1),
    F.FIELD_TIMESTAMP: run("timestamp", 1), F.FIELD_WHEELS: run("wheels", 2), F.FIELD_MAP_ID: run("map_id", 1),
    F.FIELD_OBJ_CENTER: [(a, d) for d in range(DYN) for a in ("ob_cx", "ob_cz")], F.FIELD_OBJ_ACTIVE: run("ob_active", DYN),
    F.FIELD_OBJ_YROT: run("ob_yrot", DYN), F.FIELD_OBJ_PARAMS: [(a, d) for d in range(DYN) for a in ("ob_vel", "ob_wait", "ob_wiggle")],
    F.FIELD_OBJ_VISIBLE: run("ob_visible", OBJ), F.FIELD_EPISODE: run("episode", 1), F.FIELD_OBJ_LIGHT: run("ob_light", OBJ),
    F.FIELD_OBJ_Y: run("ob_cy", DYN), F.FIELD_OBJ_EXTRA: [("ob_ext", k * DYN + d) for d in range(DYN) for k in range(5)],
    F.FIELD_CAMERA: run("cam", 6), F.FIELD_COLORS: run("colors", 16), F.FIELD_WHEEL_DIST: run("wheel_dist", 1),
}
NOT_IN_SLAB = (F.FIELD_RENDER_POS, F.FIELD_RENDER_PIPE)
N_FIELDS = 29
VIEWS = {F.FIELD_ANGLE, F.FIELD_REWARD, F.FIELD_DONE, F.FIELD_DONE_CODE, F.FIELD_STEP_COUNT, F.FIELD_LANE, F.FIELD_IN_LANE, F.FIELD_PROX, F.FIELD_SPEED,
         F.FIELD_TIMESTAMP, F.FIELD_WHEELS, F.FIELD_MAP_ID, F.FIELD_OBJ_ACTIVE, F.FIELD_OBJ_YROT, F.FIELD_OBJ_VISIBLE, F.FIELD_OBJ_LIGHT, F.FIELD_OBJ_Y,
         F.FIELD_EPISODE, F.FIELD_CAMERA, F.FIELD_COLORS, F.FIELD_WHEEL_DIST, F.FIELD_POS, F.FIELD_STATE_BLOB}

WRAPPER = r"""
#include "state_fields.h"
extern "C" {
int sf_n_arrays() { return (int)DT_STATE_N_ARRAYS; }
size_t sf_layout(int N, char* base, long* off) {
  SimArrays A{};
  const size_t bytes = dt_state_layout(A, N, base);
  for (size_t r = 0; r < DT_STATE_N_ARRAYS; ++r) off[r] = base ? dt_state_array(A, DT_STATE_ARRAYS[r].member) - base : -1;
  return A.N == N ? bytes : 0;
}
int sf_field(int id, int* out) {   // elem, comps, writable, view
  const StateField* f = dt_state_field(id);
  if (!f) return 0;
  out[0] = f->elem; out[1] = dt_field_comps(*f); out[2] = f->writable; out[3] = f->view;
  return 1;
}
size_t sf_field_bytes(int id, int N, size_t slab) { const StateField* f = dt_state_field(id); return f ? dt_field_bytes(*f, N, slab) : 0; }
long sf_plane(int id, int c, int N, char* base) {
  SimArrays A{};
  dt_state_layout(A, N, base);
  char* p = dt_field_plane(A, *dt_state_field(id), c);
  return p ? p - base : -1;
}
void sf_xfer(int id, int N, char* base, char* pub, int gather) {
  SimArrays A{};
  dt_state_layout(A, N, base);
  const StateField& f = *dt_state_field(id);
  const int comps = dt_field_comps(f);
  for (int c = 0; c < comps; ++c) {
    char* plane = dt_field_plane(A, f, c);
    if (gather) dt_plane_to_public(pub, plane, N, comps, c, f.elem);
    else if (plane) dt_public_to_plane(plane, pub, N, comps, c, f.elem);
  }
}
}
"""


@pytest.fixture(scope="module")
def sf(tmp_path_factory):
    d = tmp_path_factory.mktemp("state_fields")
    (d / "wrap.cpp").write_text(WRAPPER)
    so = d / "libstate_fields_test.so"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-shared", "-fPIC", "-I", CSRC, str(d / "wrap.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.sf_layout.restype, lib.sf_layout.argtypes = C.c_size_t, [C.c_int, C.c_void_p, C.POINTER(C.c_long)]
    lib.sf_field.argtypes = [C.c_int, C.POINTER(C.c_int)]
    lib.sf_field_bytes.restype, lib.sf_field_bytes.argtypes = C.c_size_t, [C.c_int, C.c_int, C.c_size_t]
    lib.sf_plane.restype, lib.sf_plane.argtypes = C.c_long, [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.sf_xfer.restype, lib.sf_xfer.argtypes = None, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def expected_offsets(N):
    """the 256-rounded running sum of ARRAYS: {name: offset}, and the total"""
    off, out = 0, {}
    for name, dt, planes in ARRAYS:
        out[name] = off
        off += (N * planes * np.dtype(dt).itemsize + 255) // 256 * 256
    return out, off


def field_row(sf, field):
    out = (C.c_int * 4)()
    return tuple(out) if sf.sf_field(field, out) else None


def pattern(field, N):
    """[N][comps] of the field's dtype; the value at (env, c) encodes (field, env, c) -- exactly for the 4 and 8-byte types, and for
    uint8 as far as a byte can: mod 251, never 0xA5 (the untouched slab of the write test)"""
    dt, shp = BatchedSimulator._FIELD_SHAPES[field]
    comps = int(np.prod(shp, dtype=np.int64))
    e, c = np.meshgrid(np.arange(N), np.arange(comps), indexing="ij")
    v = (field + 1) * 65536 + e * 64 + c                     # < 2^24: exact in float32
    if dt == "u1":
        v = v * 7 % 251
        v[v == 0xA5] = 252
    return np.ascontiguousarray(v.astype(dt))


def test_array_table_is_the_literal_list(sf):
    assert sf.sf_n_arrays() == len(ARRAYS) == 47 and len({n for n, _, _ in ARRAYS}) == 47


@pytest.mark.parametrize("N", sorted(SLAB_BYTES))
def test_slab_size_and_offsets(sf, N):
    want, total = expected_offsets(N)
    assert total == SLAB_BYTES[N]
    off = (C.c_long * 47)()
    assert sf.sf_layout(N, None, off) == SLAB_BYTES[N] and set(off) == {-1}         # null base: the size alone
    buf = np.zeros(SLAB_BYTES[N], np.uint8)
    assert sf.sf_layout(N, buf.ctypes.data, off) == SLAB_BYTES[N]
    assert list(off) == [want[n] for n, _, _ in ARRAYS]
    if N == 33:     # the first N at which an f64 array is padded; the three late additions stay at the end
        assert (want["tl_time"], want["ob_cy"], want["ob_ext"]) == (69376, 69888, 72192)
    if N == 64:     # a 256-byte int32 array needs no padding: tile_j follows tile_i directly
        assert want["tile_j"] - want["tile_i"] == 256


def test_sizes_and_flags(sf):
    N = 33
    writable, views = set(), set()
    for field in range(N_FIELDS):
        elem, comps, w, v = field_row(sf, field)
        writable |= {field} if w else set()
        views |= {field} if v else set()
        if field == F.FIELD_STATE_BLOB:
            assert sf.sf_field_bytes(field, N, 82944) == 82944
            continue
        dt, shp = BatchedSimulator._FIELD_SHAPES[field]
        assert elem == np.dtype(dt).itemsize and comps == int(np.prod(shp, dtype=np.int64)), field
        for n in (1, 33, 4096):
            assert sf.sf_field_bytes(field, n, 12345) == np.empty((n,) + shp, dt).nbytes, field
    assert set(BatchedSimulator._FIELD_SHAPES) | {F.FIELD_STATE_BLOB} == set(range(N_FIELDS))
    assert writable == set(range(N_FIELDS)) - set(NOT_IN_SLAB)
    assert views == VIEWS
    assert set(FIELDS) == set(range(N_FIELDS)) - set(NOT_IN_SLAB) - {F.FIELD_STATE_BLOB}
    for bad in (-1, N_FIELDS):
        assert field_row(sf, bad) is None and sf.sf_field_bytes(bad, N, 82944) == 0


@pytest.mark.parametrize("N", [33, 64])
def test_components_come_from_the_planes_of_the_literal_map(sf, N):
    want, total = expected_offsets(N)
    types = {n: dt for n, dt, _ in ARRAYS}
    planes = {n: p for n, _, p in ARRAYS}
    buf = np.zeros(total, np.uint8)
    used = set()
    for field, comps in FIELDS.items():
        assert field_row(sf, field)[1] == len(comps)
        for c, src in enumerate(comps):
            got = sf.sf_plane(field, c, N, buf.ctypes.data)
            if src is None:
                assert got == -1
                continue
            name, plane = src
            assert 0 <= plane < planes[name] and types[name] == BatchedSimulator._FIELD_SHAPES[field][0]
            assert got == want[name] + plane * N * np.dtype(types[name]).itemsize, (field, c)
            assert (name, plane) not in used, "two public components share a plane"
            used.add((name, plane))
    for field in NOT_IN_SLAB:
        assert sf.sf_plane(field, 0, N, buf.ctypes.data) == -1


def test_scatter_touches_the_named_planes_only_and_gather_returns_them(sf):
    N = 33
    want, total = expected_offsets(N)
    for field, comps in FIELDS.items():
        dt = BatchedSimulator._FIELD_SHAPES[field][0]
        size = np.dtype(dt).itemsize
        buf = np.full(total, 0xA5, np.uint8)
        pat = pattern(field, N)
        sf.sf_xfer(field, N, buf.ctypes.data, pat.ctypes.data, 0)
        expect = np.full(total, 0xA5, np.uint8)
        for c, src in enumerate(comps):
            if src is not None:
                o = want[src[0]] + src[1] * N * size
                expect[o:o + N * size] = np.ascontiguousarray(pat[:, c]).view(np.uint8)
        assert np.array_equal(buf, expect), field
        back = np.full_like(pat, 0x5A if dt == "u1" else 77)
        sf.sf_xfer(field, N, buf.ctypes.data, back.ctypes.data, 1)
        if field == F.FIELD_POS:
            assert np.array_equal(back[:, [0, 2]], pat[:, [0, 2]]) and not back[:, 1].any()
        else:
            assert np.array_equal(back, pat), field


PROGRAM = r"""
#include "state_fields.h"
#include <cstdio>
#include <vector>
int main() {
  for (int N : {1, 33}) {
    SimArrays A{};
    std::vector<char> slab(dt_state_layout(A, N, nullptr), 0);
    if (dt_state_layout(A, N, slab.data()) != slab.size()) return 1;
    for (int id = 0; id < DTSIM_FIELD__COUNT; ++id) {
      const StateField& f = *dt_state_field(id);
      const int comps = dt_field_comps(f);
      std::vector<char> pub(dt_field_bytes(f, N, slab.size())), back(pub.size(), 0x5A);
      for (size_t i = 0; i < pub.size(); ++i) pub[i] = (char)(i * 13 + id + 1);
      for (int c = 0; c < comps; ++c) if (char* p = dt_field_plane(A, f, c)) dt_public_to_plane(p, pub.data(), N, comps, c, f.elem);
      for (int c = 0; c < comps; ++c) dt_plane_to_public(back.data(), dt_field_plane(A, f, c), N, comps, c, f.elem);
      for (int c = 0; c < comps; ++c)
        for (int i = 0; i < N; ++i) {
          const size_t o = ((size_t)i * comps + c) * f.elem;
          const bool stored = dt_field_plane(A, f, c) != nullptr;
          for (size_t b = 0; b < f.elem; ++b)
            if (back[o + b] != (stored ? pub[o + b] : 0)) { fprintf(stderr, "N %d field %d component %d env %d\n", N, id, c, i); return 1; }
        }
    }
  }
  return dt_state_field(-1) || dt_state_field(DTSIM_FIELD__COUNT);
}
"""


def test_layout_scatter_and_gather_under_sanitizers(tmp_path):
    """every field laid out, scattered and gathered at N = 1 and 33 in a program of its own built with AddressSanitizer and
    UndefinedBehaviorSanitizer; the slab and the public buffers have exactly their sizes: it exits clean"""
    (tmp_path / "fields.cpp").write_text(PROGRAM)
    exe = tmp_path / "fields"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           str(tmp_path / "fields.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
