"""`-m "not gpu"`: the surface of dtsim_camera_maps without a device -- the header declares the struct and both entry points, dtsim/_ffi.py
binds them with the header's argument lists, the ABI version is unchanged, and DuckietownVecEnv(fused_maps=True) raises its documented
ValueErrors before a device or the simulator is touched."""
import ctypes as C
import os
import re

import pytest

from dtsim import _ffi
from dtsim.vecenv import DuckietownVecEnv

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtsim.h")


def test_the_header_declares_the_struct_and_both_entry_points():
    src = open(HEADER).read()
    m = re.search(r"typedef struct dtsim_camera_maps_out \{(.*?)\} dtsim_camera_maps_out;", src, re.S)
    assert m, "dtsim_camera_maps_out"
    fields = re.findall(r"^\s*(void\*|uint8_t\*|float\*) (\w+);", m.group(1), re.M)
    assert fields == [("void*", "depth"), ("uint8_t*", "labels"), ("uint8_t*", "instances"), ("float*", "flow"), ("uint8_t*", "flow_valid")]
    assert re.search(r"^int dtsim_camera_maps\(dtsim_t\* h, const dtsim_camera_maps_out\* out, int oh, int ow, uint32_t flags\);", src, re.M)
    assert re.search(r"^int dtsim_camera_maps_masked\(dtsim_t\* h, const dtsim_camera_maps_out\* out, int oh, int ow, uint32_t flags, "
                     r"const uint8_t\* mask\);", src, re.M)
    assert re.search(r"DTSIM_KERNEL_CAMERA_MAPS = (\d+)", src).group(1) == str(_ffi.KERNEL_CAMERA_MAPS)
    assert int(re.search(r"DTSIM_KERNEL__COUNT = (\d+)", src).group(1)) == _ffi.KERNEL_CAMERA_MAPS + 1


def test_the_abi_version_is_still_12():
    src = open(HEADER).read()
    assert re.search(r"#define DTSIM_ABI_VERSION 12\b", src) and _ffi.ABI_VERSION == 12


def test_ffi_binds_both_entry_points_with_the_structs_layout():
    for name in ("dtsim_camera_maps", "dtsim_camera_maps_masked"):
        assert name in _ffi.EXPORTS
    s = _ffi.CameraMapsOut
    assert [f[0] for f in s._fields_] == ["depth", "labels", "instances", "flow", "flow_valid"]
    assert all(f[1] is C.c_void_p for f in s._fields_) and C.sizeof(s) == 5 * C.sizeof(C.c_void_p)
    lib = _ffi.load()                                            # (loading the library needs no device)
    vp, ci, u32 = C.c_void_p, C.c_int, C.c_uint32
    assert lib.dtsim_camera_maps.argtypes == [vp, C.POINTER(s), ci, ci, u32] and lib.dtsim_camera_maps.restype is ci
    assert lib.dtsim_camera_maps_masked.argtypes == [vp, C.POINTER(s), ci, ci, u32, vp] and lib.dtsim_camera_maps_masked.restype is ci
    # the argument checks that need no handle
    assert lib.dtsim_camera_maps(None, C.byref(s()), 1, 1, 0) == _ffi.E_INVALID


@pytest.mark.parametrize("kw,word", [
    (dict(depth_shape=(60, 80), label_shape=(30, 40)), "one size"),
    (dict(depth_shape=(60, 80), instance_shape=(60, 80), flow_shape=(120, 160)), "one size"),
    (dict(), "at least one"),
    (dict(bev_shape=(32, 32)), "at least one"),
    (dict(flow_shape=(60, 80), camera_rand=True), "camera_rand"),
    (dict(depth_shape=(60, 80), flow_shape=(60, 80), camera_rand=True, camera_rand_maps=True), "camera_rand"),
])
def test_fused_maps_raises_before_a_device_is_touched(kw, word, monkeypatch):
    from dtsim.batched import BatchedSimulator

    def no_simulator(*a, **k):
        raise AssertionError("the simulator was built before the arguments were checked")
    monkeypatch.setattr(BatchedSimulator, "__init__", no_simulator)
    with pytest.raises(ValueError, match=word):
        DuckietownVecEnv("small_loop", 4, fused_maps=True, camera_width=160, camera_height=120, **kw)
