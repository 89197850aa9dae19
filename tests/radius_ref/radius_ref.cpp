// tests/radius_ref/radius_ref.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// The reference's radius search (reference include/fast_limo/Objects/Octree.hpp:453-523) restated over the oracle's octree
// (oracle/rl_octree.h: Octant, overlaps :435-450, get_points :217-228), in our own words like the rest of the oracle:
//   public entry   :453-477   nothing when the tree is empty; the squared radius is ONE float product (:467)
//   recursion      :479-523   an octant whose farthest corner lies inside the ball hands over ALL its points without testing
//                             them (:485-503, "the shortcut"); a leaf tests each point with a strict < (:505-515); children
//                             are visited in index order 0..7 when they overlap the ball (:517-522)
// Built by the tests (g++ -O2 -std=c++17 -ffp-contract=off -I oracle) into a temporary directory; small C interface below.
#include <cstdint>
#include <cstring>
#include <vector>
#include "rl_octree.h"

namespace {

struct RadiusRef {
  oracle::Octree tree;
  std::vector<oracle::V3f> pts;      // results of the last search, all queries, CSR
  std::vector<float> sqd;
};

// :485-489: (|query - centroid| + extent) squared, summed (Eigen's 3-coefficient reduction: c0 + (c1 + c2)), below the squared radius
bool farthest_corner_inside(const oracle::Octant* o, const oracle::V3f& q, float sqr_radius) {
  const oracle::V3f a(std::fabs(q.x - o->centroid.x) + o->extent, std::fabs(q.y - o->centroid.y) + o->extent,
                      std::fabs(q.z - o->centroid.z) + o->extent);
  return oracle::sqnorm3(a) < sqr_radius;
}

void search(const oracle::Octree& t, const oracle::Octant* o, const oracle::V3f& q, float sqr_radius, std::vector<oracle::V3f>& pts,
            std::vector<float>& sqd, uint64_t& through_shortcut) {
  if (3 * o->extent * o->extent < sqr_radius && farthest_corner_inside(o, q, sqr_radius)) {      // :491
    std::vector<oracle::V3f> all;
    t.get_points(o, all);
    for (const auto& p : all) {                                                                  // :496-500: no test
      sqd.push_back(oracle::sqnorm3(p - q));
      pts.push_back(p);
    }
    through_shortcut += all.size();
    return;
  }
  if (o->child == nullptr) {                                                                     // :505-515
    for (const auto& p : o->points) {
      const float d = oracle::sqnorm3(p - q);
      if (d < sqr_radius) {
        sqd.push_back(d);
        pts.push_back(p);
      }
    }
    return;
  }
  for (int c = 0; c < 8; c++) {                                                                  // :517-522
    if (o->child[c] == nullptr || !oracle::Octree::overlaps(o->child[c], q, sqr_radius)) continue;
    search(t, o->child[c], q, sqr_radius, pts, sqd, through_shortcut);
  }
}

}  // namespace

extern "C" {
void* rr_create(float min_extent, int downsample) {
  RadiusRef* r = new RadiusRef;
  r->tree.setMinExtent(min_extent);
  r->tree.setDownsample(downsample != 0);
  return r;
}
void rr_destroy(void* h) { delete static_cast<RadiusRef*>(h); }
// Octree::update with one batch of packed xyz
void rr_update(void* h, const float* xyz, uint64_t n) { static_cast<RadiusRef*>(h)->tree.update(xyz, (size_t)n, 3); }
uint64_t rr_size(void* h) { return static_cast<RadiusRef*>(h)->tree.size(); }
// all stored points, traversal order (out: room for rr_size points)
void rr_points(void* h, float* out) {
  RadiusRef* r = static_cast<RadiusRef*>(h);
  std::vector<oracle::V3f> all;
  r->tree.get_points(r->tree.root_, all);
  for (size_t i = 0; i < all.size(); i++) { out[3 * i] = all[i].x; out[3 * i + 1] = all[i].y; out[3 * i + 2] = all[i].z; }
}
// nq queries (packed xyz), one radius: offsets[nq + 1]; returns the total; *through_shortcut = results that were handed over
// without a test.  The results stay in the handle until the next search (rr_results copies them out).
uint64_t rr_radius_search(void* h, const float* q, uint64_t nq, float radius, uint64_t* offsets, uint64_t* through_shortcut) {
  RadiusRef* r = static_cast<RadiusRef*>(h);
  r->pts.clear();
  r->sqd.clear();
  uint64_t sc = 0;
  const float sqr_radius = radius * radius;                                                      // :467
  for (uint64_t i = 0; i < nq; i++) {
    offsets[i] = r->pts.size();
    if (r->tree.root_ == nullptr) continue;                                                      // :459
    search(r->tree, r->tree.root_, oracle::V3f(q[3 * i], q[3 * i + 1], q[3 * i + 2]), sqr_radius, r->pts, r->sqd, sc);
  }
  offsets[nq] = r->pts.size();
  if (through_shortcut) *through_shortcut = sc;
  return r->pts.size();
}
void rr_results(void* h, float* xyz, float* sqd) {
  RadiusRef* r = static_cast<RadiusRef*>(h);
  for (size_t i = 0; i < r->pts.size(); i++) { xyz[3 * i] = r->pts[i].x; xyz[3 * i + 1] = r->pts[i].y; xyz[3 * i + 2] = r->pts[i].z; }
  if (!r->sqd.empty()) std::memcpy(sqd, r->sqd.data(), r->sqd.size() * sizeof(float));
}
}
