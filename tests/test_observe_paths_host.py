"""Observation resize, host side: which kernel path of dtsim_observe each shape of the GPU case matrix reaches (so that matrix
provably covers every branch of the selection), and an independent float64 reference for the OpenCV-cubic restatement that
dtsim_observe_cubic is pinned to (cv2 itself is not installed everywhere the suite runs)."""
import numpy as np
import pytest

from dtsim import resample
from observe_util import BILINEAR_CASES, CONSTANT_KINDS, CUBIC_CASES, REQUIRED_BRANCHES, content, cubic_headroom, keys_cubic_resize, observe_path


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
