"""Observation resize, host side: which kernel path of dtsim_observe each shape of the GPU case matrix reaches (so that matrix
provably covers every branch of the selection), the planner of csrc/observe_plan.h held to that restatement, and an independent float64 reference for the OpenCV-cubic restatement that
dtsim_observe_cubic is pinned to (cv2 itself is not installed everywhere the suite runs)."""
import os
import re
import subprocess

import numpy as np
import pytest

from dtsim import resample
from observe_util import (BILINEAR_CASES, CONSTANT_KINDS, CUBIC_CASES, REQUIRED_BRANCHES, content, cubic_headroom, fast_taps,
                          keys_cubic_resize, observe_path)

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-duckietown_amd", "csrc")


@pytest.mark.parametrize("case", sorted(BILINEAR_CASES), ids=lambda c: "%dx%d-%dx%d" % c)
def test_case_reaches_its_path(case):
    assert observe_path(*case) == BILINEAR_CASES[case]


def test_case_matrix_reaches_every_branch():
    paths = [observe_path(*c) for c in BILINEAR_CASES]
    missing = [name for name, hit in REQUIRED_BRANCHES.items() if not any(hit(p) for p in paths)]
    assert not missing, missing


@pytest.mark.parametrize("case", [c for c, p in BILINEAR_CASES.items() if p.startswith("pow2")], ids=lambda c: "%dx%d-%dx%d" % c)
def test_ab_switches_leave_the_pow2_kernel(case):
    """DTSIM_OBSERVE_STAGED keeps the fast taps in k_observe; DTSIM_OBSERVE_GENERIC drops them: the A/B comparisons on the GPU
    compare different code."""
    assert observe_path(*case, staged=True).startswith("k_observe/h=hfast/v=twolane/")
    p = observe_path(*case, generic=True)
    assert "/h=hfast/" not in p and "/v=twolane/" not in p


def test_selection_gates():
    assert observe_path(640, 480, 160, 120).startswith("pow2")
    assert observe_path(642, 480, 160, 120).startswith("k_observe/h=generic")        # not S * ow == W
    assert observe_path(644, 480, 161, 120) == "k_observe/h=hfast/v=table/PER=1/load=pipelined"   # ow * 3 % 4 != 0: no two-lane sum
    assert observe_path(680, 4, 1, 1).endswith("load=pipelined")                    # 8 * ceil(3 W / 4) = 4080 <= 4096
    assert observe_path(684, 4, 1, 1).endswith("load=staged")                       # 4104
    assert observe_path(681, 4, 1, 1).endswith("load=bytes")


# argv: a file of int32 records [W, H, ow, oh, ksize_x, ksize_y, bounds_x, taps_x (a resized width), bounds_y, taps_y (a resized height)],
# staged, generic.  One line per record: kernel hfast hn vfast rows_per_block max_rows_in lds, or "error <code> <message>".
PLAN_PROGRAM = r"""
#include "observe_plan.h"
#include <cstdlib>
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> d;
  for (int32_t v; fread(&v, sizeof v, 1, f) == 1;) d.push_back(v);
  fclose(f);
  const bool staged = atoi(argv[2]) != 0, generic = atoi(argv[3]) != 0;
  for (size_t i = 0; i < d.size();) {
    const int W = d[i], H = d[i + 1], ow = d[i + 2], oh = d[i + 3], ksx = d[i + 4], ksy = d[i + 5];
    i += 6;
    const int32_t *bx = nullptr, *kx = nullptr, *by = nullptr, *ky = nullptr;
    if (ow != W) { bx = &d[i]; i += 2 * (size_t)ow; kx = &d[i]; i += (size_t)ow * ksx; }
    if (oh != H) { by = &d[i]; i += 2 * (size_t)oh; ky = &d[i]; i += (size_t)oh * ksy; }
    ObservePlan p;
    std::string err;
    int rc = dt_observe_pack(p, err, W, H, 4, oh, ow, bx, kx, ksx, by, ky, ksy);
    if (rc == DTSIM_OK) rc = dt_observe_plan(p, err, staged, generic);
    if (rc != DTSIM_OK) { printf("error %d %s\n", rc, err.c_str()); continue; }
    printf("%s %d %d %d %d %d %zu\n", p.kernel == DT_OBS_POW2 ? "pow2" : p.kernel == DT_OBS_STAGED ? "k_observe" : "cubic",
           p.P.hfast, p.P.hn, p.P.vfast, p.P.rows_per_block, p.P.max_rows_in, p.lds);
  }
  return 0;
}
"""
GATE_SHAPES = [(640, 480, 160, 120), (642, 480, 160, 120), (644, 480, 161, 120), (680, 4, 1, 1), (684, 4, 1, 1), (681, 4, 1, 1)]   # test_selection_gates


def test_planner_takes_the_path_of_the_restatement(tmp_path):
    """dt_observe_plan, compiled on its own and given the tables BatchedSimulator.observe passes, chooses the kernel and the fast taps
    observe_path says, under neither switch, DTSIM_OBSERVE_STAGED and DTSIM_OBSERVE_GENERIC (`load=` and `PER=` are decided inside
    k_observe and stay the restatement's alone); its LDS stays within DT_OBS_LDS_KB and its intermediate holds every row block."""
    shapes = list(BILINEAR_CASES) + GATE_SHAPES
    bys = []
    with open(tmp_path / "shapes.bin", "wb") as f:
        for W, H, ow, oh in shapes:
            tabs = (resample.coeffs(W, ow) if ow != W else ()) + (resample.coeffs(H, oh) if oh != H else ())
            np.array([W, H, ow, oh, tabs[1].shape[1] if ow != W else 0, tabs[-1].shape[1] if oh != H else 0], np.int32).tofile(f)
            for t in tabs:
                np.ascontiguousarray(t, dtype=np.int32).tofile(f)
            bys.append(tabs[-2].astype(np.int64) if oh != H else np.stack([np.arange(oh), np.ones(oh, np.int64)], axis=1))
    (tmp_path / "plan.cpp").write_text(PLAN_PROGRAM)
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, str(tmp_path / "plan.cpp"), "-o", str(exe)])
    lds_kb = int(re.search(r"#define DT_OBS_LDS_KB (\d+)", open(os.path.join(CSRC, "observe_plan.h")).read()).group(1))
    for staged, generic in ((False, False), (True, False), (False, True)):
        lines = subprocess.check_output([str(exe), str(tmp_path / "shapes.bin"), str(int(staged)), str(int(generic))], text=True).splitlines()
        assert len(lines) == len(shapes)
        for shape, by, line in zip(shapes, bys, lines):
            what = (shape, staged, generic, line)
            kernel, *nums = line.split()
            assert kernel in ("pow2", "k_observe"), what
            hfast, hn, vfast, rpb, rows_in, lds = (int(v) for v in nums)
            W, H, ow, oh = shape
            path = observe_path(W, H, ow, oh, staged=staged, generic=generic)
            assert path.startswith(kernel + ("<%d,%d>/" % (hn, vfast) if kernel == "pow2" else "/")), what + (path,)
            assert (hfast, hn, vfast) == fast_taps(W, H, ow, oh, generic), what
            if kernel == "k_observe":
                assert (hfast != 0) == ("/h=hfast/" in path) and (vfast != 0) == ("/v=twolane/" in path), what + (path,)
            assert lds <= lds_kb * 1024 and (lds > 0) == (kernel == "k_observe"), what
            assert rpb >= 1, what
            need = max(by[min(o0 + rpb, oh) - 1].sum() - by[o0, 0] for o0 in range(0, oh, rpb))
            assert need <= rows_in <= H, what + (need,)


def test_cubic_cases_reach_both_row_loads_and_borders():
    assert {(W * 3) % 4 == 0 for W, H, ow, oh in CUBIC_CASES} == {True, False}
    assert any(ow > W for W, H, ow, oh in CUBIC_CASES) and any(ow < W for W, H, ow, oh in CUBIC_CASES)
    assert any(W == 1 for W, H, ow, oh in CUBIC_CASES) and any(H == 1 for W, H, ow, oh in CUBIC_CASES)
    for n_in, n_out in [(W, ow) for W, H, ow, oh in CUBIC_CASES] + [(H, oh) for W, H, ow, oh in CUBIC_CASES]:
        first = resample.cubic_coeffs(n_in, n_out)[0]
        assert first.min() >= -3 and first.max() < n_in                  # what dtsim_observe_cubic accepts
    firsts = [(resample.cubic_coeffs(H, oh)[0], H) for W, H, ow, oh in CUBIC_CASES]
    assert sum(f.min() < 0 and f.max() + 3 >= H for f, H in firsts) >= 4        # first < 0 and first + 3 >= H: replicated rows


def _fuzz_sizes(n, seed):
    rng = np.random.default_rng(seed)
    sizes = [(480, 640, 120, 160), (480, 640, 60, 80), (120, 160, 150, 200), (1, 7, 5, 3), (9, 1, 4, 11), (5, 5, 1, 1)]
    for _ in range(n):
        sizes.append((int(rng.integers(1, 70)), int(rng.integers(1, 90)), int(rng.integers(1, 80)), int(rng.integers(1, 100))))
    return sizes


# measured over these sizes: noise 96.1 % exactly equal, the 1-px checkerboards 91.3 - 95.9 %, the headroom pattern 100 % (it
# saturates); never more than 1 level apart
EXACT_FRACTION = {"noise": 0.95, "checker": 0.90, "checker_x": 0.90, "checker_y": 0.90, "headroom": 0.90}


def test_resize_cubic_against_float64_keys_cubic():
    """resample.resize_cubic (11-bit taps, one int32 sum, one rounding) next to a plain float64 Keys cubic with the same geometry:
    tap quantisation alone moves a pixel by less than one level before the final rounding, so the two are within 1 everywhere and
    mostly equal; a wrong A, centre offset or border rule is several levels off."""
    stats = {k: [0, 0] for k in EXACT_FRACTION}
    for i, (H, W, oh, ow) in enumerate(_fuzz_sizes(30, 7)):
        for kind in EXACT_FRACTION:
            f = cubic_headroom(1, H, W, oh, ow)[0] if kind == "headroom" else content(kind, 1, H, W, seed=i)[0]
            got = resample.resize_cubic(f, oh, ow).astype(np.int64)
            want = keys_cubic_resize(f, oh, ow).astype(np.int64)
            d = np.abs(got - want)
            assert d.max() <= 1, (kind, (H, W), (oh, ow), int(d.max()))
            stats[kind][0] += int((d == 0).sum()); stats[kind][1] += d.size
    for kind, (eq, n) in stats.items():
        assert eq / n >= EXACT_FRACTION[kind], (kind, eq / n)


def test_resize_cubic_keeps_constants():
    for i, (H, W, oh, ow) in enumerate(_fuzz_sizes(20, 8)):
        for kind in CONSTANT_KINDS:
            for f in content(kind, 3, H, W, seed=i):
                want = np.broadcast_to(f[:1, :1], (oh, ow, 3))
                assert np.array_equal(resample.resize_cubic(f, oh, ow), want), (kind, (H, W), (oh, ow))
                assert np.array_equal(keys_cubic_resize(f, oh, ow), want), (kind, (H, W), (oh, ow))


def test_float64_reference_is_not_blind():
    """The reference tells a wrong Keys parameter or a half-pixel shift from the real thing by more than one level."""
    f = content("noise", 1, 48, 64)[0]
    ref = resample.resize_cubic(f, 20, 90).astype(np.int64)
    assert np.abs(keys_cubic_resize(f, 20, 90, A=-0.5).astype(np.int64) - ref).max() > 1
    shifted = keys_cubic_resize(np.roll(f, 1, axis=1), 20, 90).astype(np.int64)
    assert np.abs(shifted - ref).max() > 1
