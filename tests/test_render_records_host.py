"""The records one stage of the render pass writes and another reads (csrc/render_records.h) on this CPU, compiled with g++ behind a
test-only extern "C" wrapper: every size, and the offsets the kernels rely on when they read a record as 16-byte pieces or as one scalar
load, held to numbers written here.  The header's own static_asserts hold the sizes at compile time; this holds the fields that were
renamed from `pad` (they carry data) and their neighbours in the same 16-byte piece."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gym-duckietown_amd", "csrc")

SIZES = {"EnvCam": 128, "EnvFast": 64, "EnvQ": 64, "EnvV": 64, "EnvL": 16, "EnvDG": 64, "EnvDR": 80, "EnvDX": 160, "EnvD": 320,
         "PixTab": 16, "SampTab": 32}
OFFSETS = {("EnvD", "x"): 144,
           ("EnvQ", "reach"): 48, ("EnvQ", "env"): 52, ("EnvQ", "tab3"): 56, ("EnvQ", "qpm_bits"): 60,
           ("SampTab", "lr_bits"): 20, ("SampTab", "lf_bits"): 24, ("SampTab", "lit_bits"): 28}

WRAPPER = '#include "render_records.h"\nextern "C" {\n' + "".join(
    f"int rr_sizeof_{t}() {{ return (int)sizeof({t}); }}\n" for t in SIZES) + "".join(
    f"int rr_offsetof_{t}_{f}() {{ return (int)offsetof({t}, {f}); }}\n" for t, f in OFFSETS) + "}\n"


@pytest.fixture(scope="module")
def rr(tmp_path_factory):
    d = tmp_path_factory.mktemp("render_records")
    (d / "wrap.cpp").write_text(WRAPPER)
    so = d / "librender_records_test.so"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC, str(d / "wrap.cpp"), "-o", str(so)])
    return C.CDLL(str(so))


@pytest.mark.parametrize("name", sorted(SIZES))
def test_record_size(rr, name):
    assert getattr(rr, f"rr_sizeof_{name}")() == SIZES[name]


@pytest.mark.parametrize("rec,field", sorted(OFFSETS))
def test_field_offset(rr, rec, field):
    assert getattr(rr, f"rr_offsetof_{rec}_{field}")() == OFFSETS[(rec, field)]
