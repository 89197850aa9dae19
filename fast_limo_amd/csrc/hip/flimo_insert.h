// fast_limo_amd/csrc/hip/flimo_insert.h
// Host-side statement of WHICH points the map stores.  The k-NN index on the GPU is a uniform
// grid, but the reference decides what is stored through its incremental octree
// (Objects/Octree.hpp:282-432): the first batch is stored completely, later batches are routed to
// octree leaves where a leaf either splits (everything kept), appends, or -- when down-sampling is
// on, the leaf is at minimum extent and already holds more than bucket/8 = 4 points -- drops the
// whole incoming batch for that leaf.  Map contents therefore depend on this lattice, so the
// product mirrors it: an index-based node pool that keeps leaf coordinates (needed to re-split)
// and answers, per incoming point, "stored or dropped".  Effective bucket size is 32 because the
// reference's setter is a no-op (Octree.hpp:155,178-180).
//
// The map itself is maintained by the device-resident book (flimo_gbook.hip), which reproduces the same rule on the
// GPU.  This host statement backs flimo_insert_rule_replay (host-only API used by the CPU tests) and the
// book's initial batch; it is not on the product's data path.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace flimo {

struct InsertBook;
InsertBook* insert_book_create();
void insert_book_destroy(InsertBook* b);
void insert_book_config(InsertBook* b, float min_extent, bool downsample);
void insert_book_clear(InsertBook* b);
size_t insert_book_size(const InsertBook* b);
// A float32 half edge can double fewer than 300 times before it is infinite (from the smallest subnormal, 2^-149, to
// 2^128: 277 times): the root-growth loop of Octree::update never legitimately runs longer.  A batch that would need more
// is refused before anything changes.
constexpr int kMaxRootDoublings = 300;

// xyz: n packed points.  keep[i] := 1 if point i is stored, 0 if dropped (non-finite points are never stored).
// false: the batch was refused (kMaxRootDoublings), book and keep[] flags of no meaning.
bool insert_book_update(InsertBook* b, const float* xyz, size_t n, unsigned char* keep);

// flattened copy of the live tree: c4 = (cx, cy, cz, half) per node, child = 8 links per node (-1 absent),
// cnt = leaf point count or -1 for internal nodes
void insert_book_export(const InsertBook* b, std::vector<float>& c4, std::vector<int>& child, std::vector<int>& cnt, int* root_out);

}  // namespace flimo
