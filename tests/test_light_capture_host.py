"""`not gpu`: the light_capture mode on the shared camera (DTSIM_F_LIGHT_CAPTURE without DTSIM_F_DOMAIN_RAND, ABI v12) as the host side
declares it -- the header and the Python mirror agree on the ABI version, the render-pipeline field and its values, and BatchedSimulator
accepts the mode (it used to reject it before touching the library)."""
import os
import re

import pytest

from dtsim import BatchedSimulator, _ffi

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dtsim.h")


def test_header_declares_the_pipeline_field_and_abi_v12():
    src = open(HDR).read()
    assert int(re.search(r"#define DTSIM_ABI_VERSION (\d+)", src).group(1)) == _ffi.ABI_VERSION == 12
    assert int(re.search(r"DTSIM_FIELD_RENDER_PIPE = (\d+)", src).group(1)) == _ffi.FIELD_RENDER_PIPE
    assert int(re.search(r"DTSIM_FIELD__COUNT = (\d+)", src).group(1)) == _ffi.FIELD_RENDER_PIPE + 1
    for name, val in [("GENERIC", _ffi.PIPE_GENERIC), ("GENERIC_ENV", _ffi.PIPE_GENERIC_ENV), ("Q", _ffi.PIPE_Q), ("V3", _ffi.PIPE_V3),
                      ("V3DR", _ffi.PIPE_V3DR), ("ENV_LIGHT", _ffi.PIPE_ENV_LIGHT)]:
        assert int(re.search(rf"#define DTSIM_PIPE_{name} (\d+)", src).group(1)) == val, name
    assert _ffi.PIPE_ENV_LIGHT > max(_ffi.PIPE_GENERIC, _ffi.PIPE_GENERIC_ENV, _ffi.PIPE_Q, _ffi.PIPE_V3, _ffi.PIPE_V3DR)


def test_light_capture_is_accepted_without_domain_randomisation():
    """No ValueError: without a GPU the constructor gets as far as the library (which then reports that there is none)."""
    try:
        sim = BatchedSimulator("small_loop", 2, domain_rand=False, light_capture=True, camera_width=64, camera_height=48)
    except ValueError as e:
        pytest.fail(f"light_capture with domain_rand=False rejected: {e}")
    except _ffi.DtsimError as e:                       # no GPU here: dtsim_create refused -- after the keyword checks, for that reason only
        assert e.code == _ffi.E_NOGPU, e
        return
    assert sim.light_capture
    sim.close()


def test_per_env_camera_with_device_resets_is_still_rejected():
    with pytest.raises(ValueError):
        BatchedSimulator("small_loop", 2, domain_rand=False, per_env_camera=True, auto_reset=True, light_capture=True)
