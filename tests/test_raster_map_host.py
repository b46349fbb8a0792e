"""The workgroup map of the quad-record rasters (csrc/raster_map.h) on this CPU, compiled with g++ behind a test-only extern "C" wrapper:
every XCD's list, the launch size, the split into a static prefix and a ticketed suffix, and the claim protocol of k_raster_v3 played
workgroup by workgroup under adversarial arrival orders.  The prefix decode is held to a literal restatement, written here, of the formula
raster_wg had before the map moved into the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gym-duckietown_amd", "csrc")
XCDS, SPLIT = 8, 2
LAST_GROUP, ALL = -1, -2
UNITS = [1, 2, LAST_GROUP, ALL]          # the suffix lengths of the sweep (profiles/raster_ticket_map.txt)
N_TILES = [1, 11, 30, 300]
N_CHUNKS = [1, 2, 7, 8, 9, 17, 64]

WRAPPER = r"""
#include "raster_map.h"
extern "C" {
long rm_grid(int n_tiles, int n_chunks) { return (long)raster_wg_grid((size_t)n_tiles, n_chunks); }
int rm_slots(int n_tiles, int n_chunks) { return raster_list_slots(n_tiles, n_chunks); }
int rm_default_units() { return DT_RASTER_TICKET_UNITS; }
int rm_stride() { return DT_TICKET_STRIDE; }
long rm_ticket_grid(int n_tiles, int n_chunks, int units) { return (long)raster_ticket_grid((size_t)n_tiles, n_chunks, units); }
// per workgroup b of the ticketed launch: tile, chunk, live, static (a thief's slot, past the lists: not live, not static)
void rm_enumerate(int n_tiles, int n_chunks, int units, int* out) {
  const long grid = rm_ticket_grid(n_tiles, n_chunks, units), lists = rm_grid(n_tiles, n_chunks);
  for (long b = 0; b < grid; ++b) {
    const RasterItem it = b < lists ? raster_item(n_tiles, n_chunks, (int)(b & 7), (int)(b >> 3)) : RasterItem{0, 0, false};
    out[4 * b] = it.tile; out[4 * b + 1] = it.chunk; out[4 * b + 2] = it.live;
    out[4 * b + 3] = raster_slot_static(n_tiles, n_chunks, (int)(b & 7), (int)(b >> 3), units);
  }
}
// per XCD: live items, suffix items
void rm_lists(int n_tiles, int n_chunks, int units, int* out) {
  for (int x = 0; x < DT_RASTER_XCDS; ++x) { out[2 * x] = raster_list_len(n_tiles, n_chunks, x); out[2 * x + 1] = raster_ticket_len(n_tiles, n_chunks, x, units); }
}
// the claim protocol of raster_claim_issue / raster_claim_finish (raster_common.h), one claimer after the other in the given order of workgroups:
// the own counter first (a thief draws none there), then a look at the other seven and a draw from each that is not dry, until an item comes;
// per claimer tile (-1: it leaves), chunk, atomic adds used
void rm_claims(int n_tiles, int n_chunks, int units, const int* order, int n, int* out) {
  int counter[DT_RASTER_XCDS] = {0};
  for (int i = 0; i < n; ++i) {
    const int xcd = order[i] & 7;
    const bool thief = (order[i] >> 3) >= raster_list_slots(n_tiles, n_chunks);
    int adds = thief ? 0 : 1;
    RasterItem it = raster_ticket_item(n_tiles, n_chunks, xcd, thief ? 0x7fffffff : counter[xcd]++, units);
    if (!it.live) {
      int seen[DT_RASTER_XCDS];
      for (int a = 1; a < DT_RASTER_XCDS; ++a) seen[a] = counter[raster_claim_xcd(xcd, a)];
      for (int a = 1; a < DT_RASTER_XCDS; ++a) {
        const int x = raster_claim_xcd(xcd, a);
        if (it.live || seen[a] >= raster_ticket_len(n_tiles, n_chunks, x, units)) continue;
        it = raster_ticket_item(n_tiles, n_chunks, x, counter[x]++, units); ++adds;
      }
    }
    out[3 * i] = it.live ? it.tile : -1; out[3 * i + 1] = it.chunk; out[3 * i + 2] = adds;
  }
}
}
"""


@pytest.fixture(scope="module")
def rm(tmp_path_factory):
    d = tmp_path_factory.mktemp("raster_map")
    (d / "wrap.cpp").write_text(WRAPPER)
    so = d / "libraster_map_test.so"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I", CSRC, str(d / "wrap.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.rm_grid.restype = lib.rm_ticket_grid.restype = C.c_long
    ip = C.POINTER(C.c_int)
    lib.rm_enumerate.argtypes = [C.c_int] * 3 + [ip]
    lib.rm_lists.argtypes = [C.c_int] * 3 + [ip]
    lib.rm_claims.argtypes = [C.c_int] * 3 + [ip, C.c_int, ip]
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def enumerate_map(rm, n_tiles, n_chunks, units):
    grid = rm.rm_ticket_grid(n_tiles, n_chunks, units)
    out = np.zeros((grid, 4), np.int32)
    rm.rm_enumerate(n_tiles, n_chunks, units, _ptr(out))
    lists = np.zeros((XCDS, 2), np.int32)
    rm.rm_lists(n_tiles, n_chunks, units, _ptr(lists))
    return out, lists


def claims(rm, n_tiles, n_chunks, units, order):
    order = np.ascontiguousarray(order, np.int32)
    out = np.zeros((len(order), 3), np.int32)
    rm.rm_claims(n_tiles, n_chunks, units, _ptr(order), len(order), _ptr(out))
    return out


def former_decode(n_tiles, n_chunks):
    """raster_wg's non-SUB decode as it stood in render.hip before raster_map.h, for every workgroup of the launch"""
    q_tg = (n_tiles + SPLIT - 1) // SPLIT
    cpx = (n_chunks + 7) // 8
    grid = ((n_tiles + q_tg - 1) // q_tg) * q_tg * cpx * 8
    bx = np.arange(grid)
    xcd, bi = bx & 7, bx >> 3
    per_group = q_tg * cpx
    grp, gi = bi // per_group, bi % per_group
    g_tiles = np.minimum(q_tg, n_tiles - grp * q_tg)
    tile = grp * q_tg + gi % g_tiles
    chunk = xcd * cpx + gi // g_tiles
    live = (gi < g_tiles * cpx) & (chunk < n_chunks)
    return grid, tile, chunk, live


CASES = [(t, c, u) for t in N_TILES for c in N_CHUNKS for u in UNITS]


def test_build_constants(rm):
    assert rm.rm_default_units() in UNITS, "the built suffix length is one of the sweep"
    assert rm.rm_stride() * 4 >= 128, "one counter per 128-byte line"


@pytest.mark.parametrize("n_tiles,n_chunks", [(t, c) for t in N_TILES for c in N_CHUNKS])
def test_grid_and_decode_are_the_former_ones(rm, n_tiles, n_chunks):
    grid, tile, chunk, live = former_decode(n_tiles, n_chunks)
    assert rm.rm_grid(n_tiles, n_chunks) == grid == 8 * rm.rm_slots(n_tiles, n_chunks)
    out, lists = enumerate_map(rm, n_tiles, n_chunks, 0)
    assert len(out) == grid, "no suffix, no thieves: the launch is the former one"
    assert np.array_equal(out[:, 2] != 0, live)
    assert np.array_equal(out[live, 0], tile[live]) and np.array_equal(out[live, 1], chunk[live])
    assert out[:, 3].astype(bool).tolist() == live.tolist(), "no suffix: every live workgroup is static"
    assert lists[:, 1].sum() == 0 and lists[:, 0].sum() == n_tiles * n_chunks
    # today's coverage: every (tile, chunk) exactly once
    key = chunk[live] * n_tiles + tile[live]
    assert np.array_equal(np.sort(key), np.arange(n_tiles * n_chunks))


@pytest.mark.parametrize("n_tiles,n_chunks,units", CASES)
def test_prefix_and_suffix_cover_every_item_once(rm, n_tiles, n_chunks, units):
    grid, tile, chunk, live = former_decode(n_tiles, n_chunks)
    out, lists = enumerate_map(rm, n_tiles, n_chunks, units)
    # the ticketed launch: the former grid, then as many thieves per XCD as the longest suffix (none where everything is suffix)
    assert len(out) == grid + XCDS * (0 if units == ALL else lists[:, 1].max())
    assert not out[grid:, 2].any() and not out[grid:, 3].any(), "a thief's slot is neither live nor static"
    out = out[:grid]
    static = out[:, 3].astype(bool)
    assert not (static & ~live).any(), "a padding workgroup never decodes an item"
    assert np.array_equal(out[static, 0], tile[static]) and np.array_equal(out[static, 1], chunk[static]), "the prefix decode is the former one"
    xcd = np.arange(len(out)) & 7
    keys = [chunk[static] * n_tiles + tile[static]]
    for x in range(XCDS):
        n_live, n_suf = lists[x]
        assert 0 <= n_suf <= n_live and (static & (xcd == x)).sum() == n_live - n_suf
        # the suffix is the END of the list in slot order: its live, non-static slots
        suf = live & ~static & (xcd == x)
        assert suf.sum() == n_suf
        if n_suf:
            assert not static[(xcd == x) & (np.arange(len(out)) > np.flatnonzero(suf)[0])].any(), "nothing static behind the first suffix slot"
        # ticket t is the t-th of them, in slot order (one claimer of XCD x at a time draws 0, 1, 2, ...)
        got = claims(rm, n_tiles, n_chunks, units, np.full(n_suf, x))
        assert np.array_equal(got[:n_suf, 0], tile[suf]) and np.array_equal(got[:n_suf, 1], chunk[suf]) and (got[:n_suf, 2] == 1).all()
        keys.append(chunk[suf] * n_tiles + tile[suf])
        if units == ALL:
            assert n_suf == n_live
        q_tg = (n_tiles + SPLIT - 1) // SPLIT
        last = (n_tiles - 1) // q_tg                         # the last tile group, n_tiles - last * q_tg tiles
        if units in (1, 2):
            assert n_suf == min(n_live, units * (n_tiles - last * q_tg))
        if units == LAST_GROUP:
            assert n_suf == (tile[live & (xcd == x)] // q_tg == last).sum() and (tile[suf] // q_tg == last).all()
    assert np.array_equal(np.sort(np.concatenate(keys)), np.arange(n_tiles * n_chunks))


def arrival_orders(claimers, lists):
    xcd = claimers & 7
    orders = {}
    for x in range(XCDS):                                   # all claimers of one XCD first
        orders[f"xcd{x}_first"] = np.concatenate([claimers[xcd == x], claimers[xcd != x]])
    orders["reverse"] = claimers[::-1]
    empty = lists[xcd, 0] == 0
    orders["empty_lists_first"] = np.concatenate([claimers[empty], claimers[~empty]])
    for seed in range(20):
        orders[f"shuffle{seed}"] = np.random.default_rng(seed).permutation(claimers)
    return orders


@pytest.mark.parametrize("n_tiles,n_chunks,units", CASES)
def test_claim_protocol_claims_every_suffix_item_once(rm, n_tiles, n_chunks, units):
    out, lists = enumerate_map(rm, n_tiles, n_chunks, units)
    static = out[:, 3].astype(bool)
    live = out[:, 2].astype(bool)
    claimers = np.flatnonzero(~static).astype(np.int32)     # suffix slots, padding slots and thieves' slots
    want = np.sort(out[live & ~static, 1].astype(np.int64) * n_tiles + out[live & ~static, 0])
    assert len(want) == lists[:, 1].sum()
    static_keys = out[static, 1].astype(np.int64) * n_tiles + out[static, 0]
    for name, order in arrival_orders(claimers, lists).items():
        got = claims(rm, n_tiles, n_chunks, units, order)
        won = got[:, 0] >= 0
        assert (got[:, 2] >= 0).all() and (got[:, 2] <= XCDS).all(), name
        keys = np.sort(got[won, 1].astype(np.int64) * n_tiles + got[won, 0])
        assert np.array_equal(keys, want), f"{name}: every suffix item exactly once, none unclaimed"
        assert np.array_equal(np.sort(np.concatenate([keys, static_keys])), np.arange(n_tiles * n_chunks)), name
        assert (~won).sum() == len(claimers) - len(want), name
