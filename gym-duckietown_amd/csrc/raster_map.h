// raster_map.h -- the XCD-affine workgroup map of the quad-record rasters (k_raster_q, k_raster_v3, k_raster_v3dr): the launch size, the list
// of (frame tile, env chunk) items each XCD is given, and the split of a list into a static prefix and a ticketed suffix (k_raster_v3 only:
// raster_wg / raster_claim in raster_common.h).  Plain C++ without a HIP header: under hipcc every function is __host__ __device__, and a host
// compiler sees ordinary inline functions, so a host program can include it (tests/test_raster_map_host.py enumerates the lists and plays
// the claim protocol with g++).
//
// Workgroup b runs on XCD b % 8 (round-robin dispatch), and XCD x is given the x-th eighth of the env chunks (all frame tiles of each): with
// the envs in k_env_sort order, one L2 serves the envs of one region of the map for the whole launch.  Within an XCD: groups of
// dt_q_tile_group() frame tiles, all chunks of the slice for one group before the next group, so that a tile's PixTab slice (16 KB) is read
// from HBM once per XCD instead of once per chunk, while the workgroups in flight still belong to few chunks.  The mapping only matters for speed.
// Group size, round 6: HALF the frame (150 tiles at 640 x 480; 10 before) -- with 64 envs per workgroup the tiles of ONE chunk fill an XCD.
// C3 - 4.6 %, C5 - 1.8 %; the whole frame as one group is + 5 ... 12 % (profiles/r06_variants_ab.txt block P).
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define DT_MAP_FN __host__ __device__ inline
#else
#define DT_MAP_FN inline
#endif

#ifndef DT_Q_TILE_SPLIT
#define DT_Q_TILE_SPLIT 2
#endif
#define DT_RASTER_XCDS 8
DT_MAP_FN int dt_q_tile_group(int n_tiles) { return (n_tiles + DT_Q_TILE_SPLIT - 1) / DT_Q_TILE_SPLIT; }
// chunks per XCD slice
DT_MAP_FN int raster_cpx(int n_chunks) { return (n_chunks + DT_RASTER_XCDS - 1) / DT_RASTER_XCDS; }
// launch size: 8 slices of ceil(n_chunks / 8) chunks, frame tiles in groups of dt_q_tile_group() (the last group padded); n_chunks: of all N envs, also
// when the pass is masked (SUB: the workgroups past the live chunks leave at once)
inline size_t raster_wg_grid(size_t n_tiles, int n_chunks) {
  const int q_tg = dt_q_tile_group((int)n_tiles);
  return ((n_tiles + q_tg - 1) / q_tg) * q_tg * ((n_chunks + 7) / 8) * 8;
}

// ---- an XCD's list.  Slot k = blockIdx.x >> 3 of XCD x = blockIdx.x & 7; a slot of the grid's padding (the short last tile group, a slice past
// the last chunk) is not live.
struct RasterItem { int tile, chunk; bool live; };
DT_MAP_FN int raster_list_slots(int n_tiles, int n_chunks) {   // slots of every XCD: raster_wg_grid() / 8
  const int q_tg = dt_q_tile_group(n_tiles);
  return (n_tiles + q_tg - 1) / q_tg * q_tg * raster_cpx(n_chunks);
}
DT_MAP_FN RasterItem raster_item(int n_tiles, int n_chunks, int xcd, int k) {
  const int cpx = raster_cpx(n_chunks);
  const int q_tg = dt_q_tile_group(n_tiles);
  const int per_group = q_tg * cpx;
  const int grp = k / per_group, gi = k % per_group;
  const int g_tiles = q_tg < n_tiles - grp * q_tg ? q_tg : n_tiles - grp * q_tg;   // the last group may be short
  RasterItem it;
  it.tile = grp * q_tg + gi % g_tiles;
  it.chunk = xcd * cpx + gi / g_tiles;
  it.live = gi < g_tiles * cpx && it.chunk < n_chunks;
  return it;
}

// ---- the live items of XCD x, numbered in slot order: raster_list_len() of them, the chunks [x * cpx, x * cpx + raster_list_chunks()).
DT_MAP_FN int raster_list_chunks(int n_chunks, int xcd) {
  const int cpx = raster_cpx(n_chunks), left = n_chunks - xcd * cpx;
  return left < 0 ? 0 : left < cpx ? left : cpx;
}
DT_MAP_FN int raster_list_len(int n_tiles, int n_chunks, int xcd) { return n_tiles * raster_list_chunks(n_chunks, xcd); }
// number of LIVE slot k among the live items of its XCD (every group before the last is full, and a group's live slots come first)
DT_MAP_FN int raster_live_index(int n_tiles, int n_chunks, int xcd, int k) {
  const int q_tg = dt_q_tile_group(n_tiles), per_group = q_tg * raster_cpx(n_chunks);
  return k / per_group * q_tg * raster_list_chunks(n_chunks, xcd) + k % per_group;
}
// live item j of XCD x: raster_item() with the slice's live chunks in place of cpx
DT_MAP_FN RasterItem raster_live_item(int n_tiles, int n_chunks, int xcd, int j) {
  const int q_tg = dt_q_tile_group(n_tiles), per_group = q_tg * raster_list_chunks(n_chunks, xcd);
  const int grp = j / per_group, gi = j % per_group;
  const int g_tiles = q_tg < n_tiles - grp * q_tg ? q_tg : n_tiles - grp * q_tg;
  RasterItem it;
  it.tile = grp * q_tg + gi % g_tiles;
  it.chunk = xcd * raster_cpx(n_chunks) + gi / g_tiles;
  it.live = true;
  return it;
}

// ---- static prefix and ticketed suffix (k_raster_v3).  The last raster_ticket_len() live items of a list are not run by the workgroups whose
// slots they are: every workgroup of such a slot, of a padding slot and of a thief's slot (below) CLAIMS an item instead -- one atomic add on its
// XCD's counter; ticket t < suffix length is suffix item t of that list; a dry list sends it to the other seven counters in rotation from
// xcd + 1 (raster_claim_xcd), at most DT_RASTER_XCDS adds in all; with every list dry it leaves.  An XCD has at least as many claimers as
// suffix items and each begins at its own counter, so every ticket below the suffix length is drawn, whatever the others do: each suffix
// item runs exactly once, and nothing waits for anything.  An item changes XCD only when the XCD that takes it has run dry.
// `units`: the suffix in units of one chunk's tiles of the last tile group (150 items at 640 x 480); 0: no suffix (the static map);
// DT_TICKET_LAST_GROUP: the list's last tile group; DT_TICKET_ALL: the whole list.
#define DT_TICKET_LAST_GROUP (-1)
#define DT_TICKET_ALL (-2)
#ifndef DT_RASTER_TICKET_UNITS
#define DT_RASTER_TICKET_UNITS 1
#endif
#define DT_TICKET_STRIDE 32      // int32 between two XCDs' counters: each on a 128-byte line of its own
DT_MAP_FN int raster_ticket_len(int n_tiles, int n_chunks, int xcd, int units) {
  const int len = raster_list_len(n_tiles, n_chunks, xcd);
  const int q_tg = dt_q_tile_group(n_tiles), g_last = n_tiles - (n_tiles - 1) / q_tg * q_tg;   // tiles of the last group
  if (units == DT_TICKET_ALL) return len;
  if (units == DT_TICKET_LAST_GROUP) return g_last * raster_list_chunks(n_chunks, xcd);
  return units * g_last < len ? units * g_last : len;
}
// true: the workgroup of slot k decodes its item from k (prefix); false: it claims
DT_MAP_FN bool raster_slot_static(int n_tiles, int n_chunks, int xcd, int k, int units) {
  if (k >= raster_list_slots(n_tiles, n_chunks)) return false;   // a thief's slot
  if (!raster_item(n_tiles, n_chunks, xcd, k).live) return false;
  return raster_live_index(n_tiles, n_chunks, xcd, k) < raster_list_len(n_tiles, n_chunks, xcd) - raster_ticket_len(n_tiles, n_chunks, xcd, units);
}
// Thieves: a list has exactly as many claimers as suffix items, so with every slot taken nobody would ever find the own list dry.  The ticketed
// launch therefore appends raster_thieves() slots to every XCD (slots k >= raster_list_slots(): not live, they claim).  They start when all
// of the XCD's own slots have started -- the moment it has room and nothing left of its own -- and take what a late XCD has not begun.
DT_MAP_FN int raster_thieves(int n_tiles, int n_chunks, int units) {
  int most = 0;
  for (int x = 0; x < DT_RASTER_XCDS; ++x) { const int s = raster_ticket_len(n_tiles, n_chunks, x, units); most = s > most ? s : most; }
  return units == DT_TICKET_ALL ? 0 : most;            // (the whole list as suffix is the sweep's contended end: no thieves on top)
}
inline size_t raster_ticket_grid(size_t n_tiles, int n_chunks, int units) { return raster_wg_grid(n_tiles, n_chunks) + (size_t)DT_RASTER_XCDS * raster_thieves((int)n_tiles, n_chunks, units); }
DT_MAP_FN int raster_claim_xcd(int xcd, int attempt) { return (xcd + attempt) & (DT_RASTER_XCDS - 1); }   // the counter of a claimer's attempt 0 .. 7
// ticket t drawn from XCD x's counter: its item, or live = false when that list is dry
DT_MAP_FN RasterItem raster_ticket_item(int n_tiles, int n_chunks, int x, int t, int units) {
  const int s = raster_ticket_len(n_tiles, n_chunks, x, units);
  if (t >= s) return RasterItem{0, 0, false};
  return raster_live_item(n_tiles, n_chunks, x, raster_list_len(n_tiles, n_chunks, x) - s + t);
}
