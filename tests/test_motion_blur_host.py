"""`not gpu`: the blend's model (motion_blur_model) against the reference's own expression -- np.average(window, axis=0,
weights=[0.8, 0.15, 0.04, 0.01]), learning/utils/wrappers.py:29 -- on every reachable sum; the division the kernel uses on every numerator and
divisor; the declaration / export of dtsim_blend_frames with an unchanged ABI version; its argument checks without a device; and
DuckietownVecEnv's argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dtsim import DuckietownVecEnv, _ffi
from motion_blur_model import REF_WEIGHTS, blend_f32, blend_u8, device_round, every_sum_window, sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def window():
    """[4, 25501 + 200000] uint8: every sum S in 0 .. 25500 once, then random bytes; with the reference's float64 average of it."""
    w = np.concatenate([every_sum_window(), np.random.default_rng(5).integers(0, 256, (4, 200000), dtype=np.uint8)], axis=1)
    avg = np.average(list(w), axis=0, weights=[0.8, 0.15, 0.04, 0.01])
    assert avg.dtype == np.float64
    return w, avg


def test_the_window_realises_every_sum():
    S, D = sums(list(every_sum_window()), REF_WEIGHTS)
    assert D == 100 and np.array_equal(S, np.arange(25501))


def test_integer_sums_are_the_reference_average(window):
    w, avg = window
    S, D = sums(list(w), REF_WEIGHTS)
    assert np.abs(avg - S / D).max() <= 1e-10


def test_float32_output_is_the_reference_average_in_float32(window):
    w, avg = window
    got = blend_f32(list(w), REF_WEIGHTS)
    assert got.dtype == np.float32 and np.array_equal(got, avg.astype(np.float32))


def test_uint8_output_rounds_the_reference_average_half_up(window):
    w, avg = window
    S, _ = sums(list(w), REF_WEIGHTS)
    got = blend_u8(list(w), REF_WEIGHTS).astype(np.int64)
    tie = S % 100 == 50
    assert int(tie[:25501].sum()) == 255                    # S = 50, 150 .. 25450
    assert np.array_equal(got[~tie], np.floor(avg[~tie] + 0.5).astype(np.int64))
    assert np.array_equal(got[tie], S[tie] // 100 + 1)      # the upper of the two neighbours


def test_the_kernels_division_is_exact_for_every_numerator_and_divisor():
    for D in range(1, 257):
        S = np.arange(255 * D + 1, dtype=np.int64)
        assert np.array_equal(device_round(S, D).astype(np.int64), (2 * S + D) // (2 * D)), D


def test_blend_frames_declared_mirrored_and_exported():
    src = open(os.path.join(ROOT, "include", "dtsim.h")).read()
    assert re.search(r"\bint dtsim_blend_frames\s*\(", src)
    assert int(re.search(r"#define DTSIM_BLEND_MAX\s+(\d+)", src).group(1)) == _ffi.BLEND_MAX == 8
    assert "dtsim_blend_frames" in _ffi.EXPORTS
    lib = _ffi.load()
    assert len(lib.dtsim_blend_frames.argtypes) == 7
    assert _ffi.ABI_VERSION == 12 and lib.dtsim_abi_version() == 12
    assert "#define DTSIM_ABI_VERSION 12" in src


def _call(lib, h, out, frames, weights, n=None, flags=0):
    fp = None if frames is None else (C.c_void_p * max(len(frames), 1))(*frames)
    wp = None if weights is None else (C.c_uint32 * max(len(weights), 1))(*weights)
    return lib.dtsim_blend_frames(h, out, fp, wp, len(weights) if n is None else n, flags, None)


def test_blend_frames_rejects_bad_arguments_without_a_device():
    """Every DTSIM_E_INVALID case is decided before the handle is read or a device touched: `h` is a block of zeros standing for a handle (the
    error text says which check refused), and the pointers are never followed."""
    lib = _ffi.load()
    zeros = C.create_string_buffer(1 << 20)
    h, p = C.cast(zeros, C.c_void_p), 4096
    ok_f, ok_w = [p] * 4, [80, 15, 4, 1]
    for args, why in [
        ((None, p, ok_f, ok_w), b"null argument"),
        ((h, None, ok_f, ok_w), b"null argument"),
        ((h, p, None, ok_w), b"null argument"),
        ((h, p, ok_f, None, 4), b"null argument"),
        ((h, p, [p, p, None, p], ok_w), b"frames[2] is null"),
        ((h, p, [], [], 0), b"n = 0"),
        ((h, p, [p] * 9, [1] * 9), b"n = 9"),
        ((h, p, ok_f, ok_w, -1), b"n = -1"),
        ((h, p, ok_f, [80, 256, 4, 1]), b"weights[1] = 256"),
        ((h, p, ok_f, [0, 0, 0, 0]), b"sum to 0"),
        ((h, p, ok_f, [255, 1, 1, 0]), b"sum to 257"),
        ((h, p, [p] * 8, [255] * 8), b"sum to 2040"),
        ((h, p, ok_f, ok_w, None, _ffi.OBS_CHW), b"unknown flags"),
        ((h, p, ok_f, ok_w, None, _ffi.OBS_F32 | _ffi.OBS_GRAY), b"unknown flags"),
        ((h, p, ok_f, ok_w, None, 1 << 20), b"unknown flags"),
    ]:
        assert _call(lib, *args) == _ffi.E_INVALID, why
        err = lib.dtsim_last_error()
        assert b"dtsim_blend_frames" in err and why in err, (why, err)


@pytest.mark.parametrize("kw", [
    dict(motion_blur=True),                                 # the default action_mode is vel_steer
    dict(motion_blur=True, action_mode="vel_steer"),
    dict(motion_blur=(1, 1), action_mode="vel_steer"),
    dict(motion_blur=True, action_mode="wheels", frame_skip=2),
    dict(motion_blur=True, action_mode="wheels", frame_skip=0),
    dict(motion_blur=(100,), action_mode="wheels"),
    dict(motion_blur=(1,) * 9, action_mode="wheels"),
    dict(motion_blur=(80, 256, 4, 1), action_mode="wheels"),
    dict(motion_blur=(255, 1, 1), action_mode="wheels"),
    dict(motion_blur=(0, 0, 0, 0), action_mode="wheels"),
    dict(motion_blur=(80, -1, 4, 1), action_mode="wheels"),
    dict(motion_blur=(0.8, 0.15, 0.04, 0.01), action_mode="wheels"),
    dict(motion_blur=3, action_mode="wheels"),
])
def test_vecenv_argument_errors_come_before_the_simulator(kw):
    """(device 10 ** 6 does not exist: reaching the device or the simulator would raise something else than ValueError)"""
    with pytest.raises(ValueError, match="motion_blur"):
        DuckietownVecEnv("small_loop", 4, device=10 ** 6, **kw)
