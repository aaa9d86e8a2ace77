/*
 * lab4d_occgrid.h -- occupancy bit grid and empty-space skipping for the hash field (included by lab4d_hip.h).
 *
 * Not in the reference (nnutils/nerf.py:98 is a TODO; parity unpinned, as for the hash field itself): a bit per cell of a coarse grid
 * over the field's box, refreshed from the field's own density (Mueller et al. 2022, section 5.4 / appendix E), consulted per sample
 * and per ray.  The arithmetic is lab4d_amd/csrc/occgrid_math.hpp, shared with the CPU twin tests/host_harness/occgrid_host.cpp; the
 * kernels equal the twin bit for bit.
 *
 * Rules:
 *   GRID    G cells per axis over aabb = {lo xyz, hi xyz} (device float[6]), 2 <= G <= 256.  x01 = (x - lo) / (hi - lo) per axis.  A point
 *           has a cell iff 0 <= x01 <= 1 on every axis (NaN: none); the cell along an axis is min(G - 1, int(x01 * G)), so a point on an
 *           inner cell face belongs to the higher cell.  Linear index (i * G + j) * G + k, x slowest; cell idx is bit (idx & 31) of
 *           32-bit word (idx >> 5); ceil(G^3 / 32) words, the unused bits of the last word are zero.
 *   UPDATE  ema_new = max(ema_old * decay, d), the product rounded on its own; d = the cell's fresh density, NaN or negative counts as 0;
 *           bit = ema_new > thresh.  A new grid has every bit set and ema = +inf ("nothing known yet"); the first update of a cell whose
 *           ema is +inf replaces it: ema_new = d.
 *   MASK    mask[s] = 1 iff the point has a cell and that cell's bit is set.
 *   SPAN    ray o + t * d, t in [t0, t1]; d need not have unit length, t is in the caller's depth units.  The ray is clipped to the box
 *           with the slab test in x01 space (a zero component of d: that slab is always or never satisfied, depending on o; no infinity
 *           or NaN arithmetic is relied upon; a ray with a non-finite input or t0 > t1 misses), then the cells are walked in order
 *           (Amanatides & Woo), at most 3 * G of them.  t_first = entry parameter of the first occupied cell (>= t0), t_last = exit
 *           parameter of the last occupied cell (<= t1), hit = 1 iff an occupied cell was visited; hit = 0: both equal t0.
 *   TIES    a ray through a cell edge or corner (two or three axes share the smallest exit parameter): one axis is stepped at a time, the
 *           lowest index first (x, y, z); the cell in between is visited with an interval of zero length and counts if occupied.  The
 *           rule compares parameters only: the same for negative and positive directions.
 *
 * All three calls are capturable in a hipGraph (no read-back, no allocation); arguments are checked before the launch.
 */
#ifndef LAB4D_OCCGRID_H
#define LAB4D_OCCGRID_H

/* density (G^3) fp32 -> ema (G^3, in place), bits (ceil(G^3 / 32) words, every word rewritten), n_occupied (device int32[1],
 * overwritten: the number of set bits).  One lane per cell; a wave's 64 decisions are one ballot, n_occupied is a sum of popcounts
 * through integer atomics (order-independent). */
int lab4d_occgrid_update(const float* density, float* ema, uint32_t* bits, int32_t* n_occupied, int G, float decay, float thresh,
                         void* stream);

/* xyz (S, 3) world points -> mask (S) uint8, the input of lab4d_compact. */
int lab4d_occgrid_mask(const float* xyz, const float* aabb, const uint32_t* bits, int G, long S, uint8_t* mask, void* stream);

/* origin, dir (R, 3), t_range (R, 2) = {t0, t1} -> t_span (R, 2) = {t_first, t_last}, hit (R) uint8.  One lane per ray. */
int lab4d_occgrid_ray_span(const float* origin, const float* dir, const float* t_range, const float* aabb, const uint32_t* bits, int G,
                           long R, float* t_span, uint8_t* hit, void* stream);

#endif /* LAB4D_OCCGRID_H */
