"""`not gpu`: the masked-pass entry points (dtsim_render_masked, dtsim_observe_masked, dtsim_observe_cubic_masked, dtsim_copy_rows) are
declared by include/dtsim.h and exported by the library, and the ABI version did not move (the additions are new functions only)."""
import os
import re

from dtsim import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dtsim_render_masked", "dtsim_observe_masked", "dtsim_observe_cubic_masked", "dtsim_copy_rows")


def test_masked_entry_points_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "dtsim.h")).read()
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _ffi.EXPORTS, name
    lib = _ffi.load()
    for name in NEW:
        assert getattr(lib, name).argtypes, name
    assert _ffi.ABI_VERSION == 12 and lib.dtsim_abi_version() == 12
    assert "#define DTSIM_ABI_VERSION 12" in src


def test_masked_calls_reject_a_null_mask_without_a_device():
    """The argument checks run before anything touches a device: a null handle or mask is DTSIM_E_INVALID."""
    lib = _ffi.load()
    assert lib.dtsim_render_masked(None, 0, None) == _ffi.E_INVALID
    assert lib.dtsim_copy_rows(None, None, None, 16, None) == _ffi.E_INVALID
    assert lib.dtsim_observe_masked(None, None, 1, 1, 0, None, None, None, 0, None, None, 0) == _ffi.E_INVALID
    assert lib.dtsim_observe_cubic_masked(None, None, 1, 1, 0, None, None, None, None, None) == _ffi.E_INVALID
