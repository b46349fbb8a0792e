"""GPU: every public field of a handle written, read back and checked against every other one; dtsim_field_bytes against
BatchedSimulator._FIELD_SHAPES; which fields offer a device view and where in the slab it lies; the state blob as the checkpoint of all
of them (csrc/state_fields.h; the patterns and the literal tables are those of test_state_fields_host.py).

A handle that has had patterns written into it holds junk map ids and tiles: it is only read and closed, never stepped, reset, queried
or rendered."""
import ctypes as C

import numpy as np
import pytest

import test_state_fields_host as host
from dtsim import BatchedSimulator, _ffi

pytestmark = pytest.mark.gpu

NS = (1, 33, 64)
BLOB, POS = _ffi.FIELD_STATE_BLOB, _ffi.FIELD_POS
SHAPES = BatchedSimulator._FIELD_SHAPES
WRITABLE = sorted(host.FIELDS)                                # every field of the slab's arrays
ALL = sorted(SHAPES)                                          # ... and the two read-only ones of the render pass


def _sim(N):
    return BatchedSimulator("small_loop", N, render=False, domain_rand=False, seed=3)


def _read_all(sim):
    return {f: sim.read(f) for f in ALL}


def _expected(field, pat):
    if field == POS:                                          # y is not stored: it reads 0
        pat = pat.copy()
        pat[:, 1] = 0
    return pat.reshape((pat.shape[0],) + SHAPES[field][1])


@pytest.fixture(scope="module")
def patterned():
    """{N: (handle with host.pattern written to every writable field, {field: what it reads})}"""
    out = {}
    for N in NS:
        sim = _sim(N)
        for f in WRITABLE:
            sim.write(f, host.pattern(f, N))
        out[N] = sim, {f: _expected(f, host.pattern(f, N)) for f in WRITABLE}
    yield out
    for sim, _ in out.values():
        sim.close()


@pytest.mark.parametrize("N", NS)
def test_round_trip_and_isolation(N):
    sim = _sim(N)
    state = _read_all(sim)
    assert np.array_equal(state[_ffi.FIELD_RENDER_POS], np.arange(N))
    for f in WRITABLE:
        pat = host.pattern(f, N)
        sim.write(f, pat)
        state[f] = _expected(f, pat)
        now = _read_all(sim)
        for g in ALL:
            assert now[g].dtype == state[g].dtype and np.array_equal(now[g], state[g]), (f, g)
    sim.close()


def test_sizes_and_errors():
    sim = _sim(33)
    lib, h, N = sim._lib, sim._h, 33
    assert lib.dtsim_state_bytes(h) == host.SLAB_BYTES[N]
    need = {f: np.empty((N,) + shp, dt).nbytes for f, (dt, shp) in SHAPES.items()}
    need[BLOB] = host.SLAB_BYTES[N]
    assert sorted(need) == list(range(host.N_FIELDS))
    buf = np.zeros(host.SLAB_BYTES[N] + 1, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    err = lambda: lib.dtsim_last_error().decode()
    for f, n in need.items():
        assert lib.dtsim_field_bytes(h, f) == n, f
        for call in (lib.dtsim_read, lib.dtsim_write):
            for given in (n - 1, n + 1):
                assert (call(h, f, p, given), err()) == (_ffi.E_INVALID, f"field {f}: {given} bytes given, {n} expected")
    for bad in (-1, host.N_FIELDS):
        assert lib.dtsim_field_bytes(h, bad) == 0
        assert (lib.dtsim_read(h, bad, p, 8), err()) == (_ffi.E_INVALID, f"unknown field {bad}")
        assert (lib.dtsim_write(h, bad, p, 8), err()) == (_ffi.E_INVALID, f"unknown field {bad}")
    assert (lib.dtsim_read(h, POS, None, need[POS]), err()) == (_ffi.E_INVALID, "null argument")
    for f, name in ((_ffi.FIELD_RENDER_POS, "DTSIM_FIELD_RENDER_POS"), (_ffi.FIELD_RENDER_PIPE, "DTSIM_FIELD_RENDER_PIPE")):
        assert (lib.dtsim_write(h, f, p, need[f]), err()) == (_ffi.E_INVALID, name + " is read-only")
    assert np.array_equal(sim.read(_ffi.FIELD_RENDER_POS), np.arange(N, dtype=np.int32))
    assert not buf.any()
    sim.close()


@pytest.mark.parametrize("N", NS)
def test_device_views(patterned, N):
    sim, want = patterned[N]
    lib, h = sim._lib, sim._h
    view = {f: lib.dtsim_field_devptr(h, f) for f in range(-1, host.N_FIELDS + 1)}
    assert {f for f, p in view.items() if p} == host.VIEWS
    blob = sim.read(BLOB)
    assert blob.nbytes == host.SLAB_BYTES[N]
    for f in sorted(host.VIEWS - {BLOB}):
        dt, shp = SHAPES[f]
        pat = want[f].reshape(N, -1)
        comps = 1 if f == POS else pat.shape[1]               # POS: the x plane alone
        off, size = view[f] - view[BLOB], comps * N * np.dtype(dt).itemsize
        assert 0 <= off and off + size <= blob.nbytes, f
        assert np.array_equal(blob[off:off + size].view(dt).reshape(comps, N), pat[:, :comps].T), f


@pytest.mark.parametrize("N", NS)
def test_blob_is_the_checkpoint_of_every_field(patterned, N):
    sim, want = patterned[N]
    other = _sim(N)
    assert other.state_bytes == sim.state_bytes == host.SLAB_BYTES[N]
    other.write(BLOB, sim.read(BLOB))
    for f in WRITABLE:
        assert np.array_equal(other.read(f), want[f]), f
    other.close()
