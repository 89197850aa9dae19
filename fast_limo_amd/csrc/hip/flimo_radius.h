// fast_limo_amd/csrc/hip/flimo_radius.h -- the ball walk's device parts, shared by flimo_radius.hip (radius search) and
// flimo_cluster.hip (Euclidean clusters): the ball's box of cells, the conservative pruning of a row, the group's lane mask
// and the lane plan (radius_plan).  Private to the two files; include it after `#pragma clang fp contract(off)`.
#pragma once
#include <hip/hip_runtime.h>
#include "flimo_types.h"
#include "flimo_math.h"

namespace flimo {

constexpr int RS_UNROLL = 4;
constexpr int RS_BLOCK = 256;

template <int L>
__device__ __forceinline__ uint32_t group_mask_of(unsigned long long ballot, int lane) {
  if (L == 64) return 0;      // (not used)
  return (uint32_t)(ballot >> (lane & ~(L - 1))) & ((1u << L) - 1u);
}

// the query in cell units, the ball in cell units (inflated), the clipped box of cells
struct RadiusGeo {
  float qcx, qcy, qcz, margin, bnd2;
  int x0, x1, y0, y1, z0, z1;      // inclusive; empty when a first exceeds its last
};
__device__ __forceinline__ int rs_floor_clamped(float v) { return (int)floorf(fminf(fmaxf(v, -1.0e9f), 1.0e9f)); }
__device__ __forceinline__ bool radius_geo(const GridView& G, int maxdim, float gx, float gy, float gz, float radius, RadiusGeo& g) {
  const float fx = (gx - G.ox) * G.inv_cell, fy = (gy - G.oy) * G.inv_cell, fz = (gz - G.oz) * G.inv_cell;
  g.x0 = g.y0 = g.z0 = 0; g.x1 = g.y1 = g.z1 = -1;
  g.qcx = g.qcy = g.qcz = 0.f; g.margin = 0.f; g.bnd2 = 0.f;
  if (!(fx == fx) || !(fy == fy) || !(fz == fz)) return false;      // NaN query: empty
  // (the query's cell and the rounding margin: knn_far_kernel)
  const float flx = floorf(fminf(fmaxf(fx, -1.0e9f), 1.0e9f)), fly = floorf(fminf(fmaxf(fy, -1.0e9f), 1.0e9f)),
              flz = floorf(fminf(fmaxf(fz, -1.0e9f), 1.0e9f));
  const int cx = (int)flx - G.six, cy = (int)fly - G.siy, cz = (int)flz - G.siz;
  const float rx = fminf(fmaxf(fx - flx, 0.f), 1.f), ry = fminf(fmaxf(fy - fly, 0.f), 1.f), rz = fminf(fmaxf(fz - flz, 0.f), 1.f);
  g.qcx = (float)cx + rx; g.qcy = (float)cy + ry; g.qcz = (float)cz + rz;
  g.margin = 1.0e-3f + 4.0e-7f * fmaxf((float)maxdim, fmaxf(fmaxf(fabsf(g.qcx), fabsf(g.qcy)), fabsf(g.qcz)));
  // the radius in cells, inflated: a point with a float32 distance below r^2 lies inside it
  const float rc = (radius * (1.f + 1.0e-5f) + 1.0e-6f) * G.inv_cell;
  g.bnd2 = rc * rc * (1.f + 1.0e-5f);
  const float reach = rc * (1.f + 1.0e-5f) + g.margin + 1.0e-4f;
  g.x0 = max(0, rs_floor_clamped(g.qcx - reach)); g.x1 = min(G.nx - 1, rs_floor_clamped(g.qcx + reach));
  g.y0 = max(0, rs_floor_clamped(g.qcy - reach)); g.y1 = min(G.ny - 1, rs_floor_clamped(g.qcy + reach));
  g.z0 = max(0, rs_floor_clamped(g.qcz - reach)); g.z1 = min(G.nz - 1, rs_floor_clamped(g.qcz + reach));
  return g.x0 <= g.x1 && g.y0 <= g.y1 && g.z0 <= g.z1;
}
// the range of `pts` of row (yy, zz) the ball can reach (rows inside the clipped box only); len = 0: none
__device__ __forceinline__ void radius_row(const GridView& G, const RadiusGeo& g, int yy, int zz, uint32_t& lo, uint32_t& len) {
  lo = 0; len = 0;
  const float a = fmaxf(fmaxf((float)yy - g.qcy, g.qcy - (float)(yy + 1)) - g.margin, 0.f),
              b = fmaxf(fmaxf((float)zz - g.qcz, g.qcz - (float)(zz + 1)) - g.margin, 0.f);
  const float dyz2 = a * a + b * b;
  if (!(dyz2 <= g.bnd2)) return;
  int x0 = g.x0, x1 = g.x1;
  if (g.bnd2 < 1.0e18f) {
    // cells of the row the ball reaches: |x - qcx| <= xr, widened
    const float xr = fl_sqrt(fmaxf(g.bnd2 - dyz2, 0.f)) * (1.f + 1.0e-6f) + g.margin + 1.0e-4f;
    x0 = max(x0, rs_floor_clamped(g.qcx - xr));
    x1 = min(x1, rs_floor_clamped(g.qcx + xr));
  }
  if (x0 > x1) return;
  uint32_t hi;
  grid_row_range(G, G.dir, yy, zz, x0 * G.xs, (x1 + 1) * G.xs, lo, hi);
  len = hi > lo ? hi - lo : 0u;
}

// lanes per query and the kind of walk, from the rows the ball's box spans ((2 ceil(r / cell) + 1)^2, capped by the grid)
inline void radius_plan(const GridView& G, float radius, int& lanes, bool& tiles) {
  const double span = 2.0 * ceil((double)radius / (double)G.cell) + 1.0;
  const double rows = fmin(span, (double)G.ny) * fmin(span, (double)G.nz);
  tiles = rows > 4096.0;
  lanes = rows <= 9.0 ? 8 : (rows <= 25.0 ? 16 : 64);
  if (tiles) lanes = 64;
}

}  // namespace flimo
