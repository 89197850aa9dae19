// fast_limo_amd/csrc/hip/flimo_kernels.h -- host-callable launchers of the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "flimo_types.h"

namespace flimo {
struct FuseArgs;
struct TieList;
struct BookView;
struct ChainCtl;    // flimo_chain.h: the filter's algebra inside the pass's reducing launch
struct PipeHead;    // flimo_chain.h: the head of a pass queued ahead of its pose (pipelined host loop)
struct ChainHead;   // flimo_chain.h: a launch given one reads its pose constants from the device filter and leaves at once when the chain has ended
// The deskew of a scan's raw points riding on the first pass's k-NN launch (instead of a dispatch of its own): arguments of
// launch_deskew, `on` = 1 when they are valid
struct DeskewArgs {
  const float4* raw; const double* t; const void* frames; int nf; const float* mats; double t_offset;
  float4* out_sorted; float4* out_orig; int on;
  int stage_words;     // > 0: frames + matrices (this many 4-byte words from `frames`) were stored by the HOST into fine-grained device
                       // memory -- no copy launch; the riding pass reads them once per workgroup, past the caches, into shared memory
};

// flimo_kernels.hip
// per pass: k-NN (fast path + worklist widening), then fit + in-block reduction, then the final sum
void launch_knn5(hipStream_t st, int lanes_per_query, const GridView& G, const float4* scan_sorted, int n,
                 const PoseMats& P, int max_ring, void* nbr, int* wl, int* wl_count, unsigned long long* cand,
                 const PrevPass& prev, int tail, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, const struct FuseArgs* fuse = nullptr,
                 const TieList* ties = nullptr, int after_fine = 0, unsigned long long seq = 0ull, const DeskewArgs* deskew = nullptr,
                 const ChainHead* chain = nullptr);
// (chain: the head was stored by an earlier launch on the same stream -- the launch reads it with plain loads and never waits;
//  only launch_match_fused queues a pass ahead of its pose, through a PipeHead)
// fine pre-pass over the second-level grid of crowded regions (see flimo_map.hip); launches that follow it pass after_fine = 1
void launch_knn5_fine(hipStream_t st, const GridView& Gf, const float4* scan_sorted, int n, const PoseMats& P, void* nbr,
                      const PrevPass& prev, const int qlo[3], const int qhi[3], const TieList* ties, unsigned long long seq,
                      const ChainHead* chain = nullptr);
// tail != 0: queries that need more than the 3x3x3 block are finished inside the k-NN launch itself (gates of at most 3
// rings; launch_knn5 clears the flag otherwise) and launch_widen has nothing to do
void launch_widen(hipStream_t st, const GridView& G, const float4* scan_sorted, const PoseMats& P, int max_ring, void* nbr,
                  int* wl, int* wl_count, unsigned long long* cand, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr,
                  const TieList* ties = nullptr, const ChainHead* chain = nullptr);
int fit_blocks(int n);
void set_xcd_stripe(int stripe);   // block -> scan chunk mapping of the per-pass kernels (see xcd_chunk)
// the fit kernel reduces in FIT_GROUPS groups; slot g of its output = 256 sums + the pass number (FIT_SLOT doubles).
// `ticket` arrays hold FIT_GROUPS + 1 counters: one per group and one launch-wide (fit_reduce_publish)
constexpr int FIT_GROUPS = 8;
constexpr int FIT_SLOT = 264;
// fit + in-block MFMA reduction + grid reduction by the last block: out256[0..255] receives the raw
// 16x16 accumulator and out256[256] (as u64) the pass number `seq` (system-scope release), `ticket` and `wl_count` are reset for the next pass
void launch_fit(hipStream_t st, const GridView& G, const float4* scan_sorted, int n, const void* nbr, const PoseMats& P,
                const MatchParams& mp, double* partials, Rec16* recs, RecDbg* dbg, double* out256, unsigned int* ticket,
                int* wl_count, unsigned long long seq);
// fit2: the per-pass fast path (no records, no caps).  Only the FIT_LIVE sums the filter reads leave a block (upper triangle
// of H^T H, H^T h, M; live_idx[k] = index of sum k among the wave's 256 raw MFMA accumulators); the last block of each
// group publishes FIT_LIVE_PAD 16-byte granules {sum, pass number as bits} to out_granules[group] (mapped host memory).
constexpr int FIT_LIVE = 91;
constexpr int FIT_LIVE_PAD = 96;
int fit2_blocks(int n);
void launch_fit2(hipStream_t st, const GridView& G, const float4* scan_sorted, int n, const void* nbr, const PoseMats& P,
                 const MatchParams& mp, const unsigned char* live_idx, double* partials, void* out_granules, unsigned int* ticket,
                 int* wl_count, unsigned long long seq, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, const TieList* ties = nullptr,
                 const ChainHead* chain = nullptr, const ChainCtl* ctl = nullptr, const BookView* book = nullptr);
// The whole measurement pass in ONE launch (k-NN fast path + in-kernel tail + fit + reduction + publish; two lanes per query, gates of
// 2..3 rings): partials needs fused_blocks(n) * FIT_LIVE_PAD doubles; results arrive as launch_fit2's granules.
constexpr int FUSED_SPREAD_SLOTS = 32768;     // scans below this many query slots are spread over more workgroups
int fused_spread(int n);
int fused_blocks(int n);
void launch_match_fused(hipStream_t st, const GridView& G, const float4* scan_sorted, int n, const PoseMats& P, const MatchParams& mp,
                        void* nbr, int* wl, int* wl_count, unsigned long long* cand, const PrevPass& prev,
                        const unsigned char* live_idx, double* partials, void* out_granules, unsigned int* ticket,
                        unsigned long long seq, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, const TieList* ties = nullptr,
                        int after_fine = 0, const DeskewArgs* deskew = nullptr, const ChainHead* chain = nullptr,
                        const ChainCtl* ctl = nullptr, const BookView* book = nullptr, unsigned int wait_epoch = 0u,
                        const PipeHead* pipe = nullptr);      // pipe + wait_epoch (both or neither): the pass is queued ahead of its pose and waits
                                                              // there for the granules of that epoch (chain_enter)
// The reference's choice among exactly tied distances (first met by Octree::knn's recursion): BookView = the device copy of the
// octree (insert book), TieList = the queries a pass flagged.  launch_tie rewrites their neighbour records; launch_knn_tie does the
// same for the output of launch_knn.
struct BookView { const float4* node_c; const int* node_child; const int* node_cnt; int root; unsigned long long* settled; };   // settled (optional): queries whose ties were settled inside a reducing launch
struct TieList { int* list; unsigned int* count; unsigned int cap; unsigned int* count_next; };
void launch_tie(hipStream_t st, const GridView& G, const BookView& B, const float4* scan_sorted, const PoseMats& P, void* nbr,
                const TieList& tl);
void launch_knn_tie(hipStream_t st, const GridView& G, const BookView& B, const float* qxyz, int nq, int k, int32_t* idx, float* sqd,
                    const int32_t* cnt);
// General NUM_MATCH_POINTS (3..8): exact k-NN by the ring search + M x 3 plane fit, records written at the original indices
// (reduce them with launch_cap / launch_reduce).  nbrk: n * nbrk_rec_size() bytes of scratch.  false: k out of range.
size_t nbrk_rec_size();
bool launch_match_k(hipStream_t st, int k, const GridView& G, const float4* scan_sorted, int n, const PoseMats& P,
                    const MatchParams& mp, void* nbrk, Rec16* recs, RecDbg* dbg, const BookView* book = nullptr);   // book: ties the reference's way
size_t nbr_rec_size();
size_t wl_entry_size();   // bytes per worklist entry (query index, world position, 5th-distance hint)
void launch_knn(hipStream_t st, const GridView& G, const float* qxyz, int nq, int k, int max_ring, int32_t* idx,
                float* sqd, int32_t* cnt);
void launch_cap(hipStream_t st, Rec16* recs, int n, int cap);
// MAX_NUM_MATCHES path in one launch: rank valid records in scan order, reduce the first `cap`, publish to slot 0 + pass number
void launch_capreduce(hipStream_t st, const Rec16* recs, int n, int cap, double* out256, int* wl_count, unsigned long long seq);
void launch_reduce(hipStream_t st, const Rec16* recs, int n, int nwaves, double* partials, double* out256);
void launch_mfma_layout(hipStream_t st, double* raw256);
void launch_word_probe(hipStream_t st, const unsigned int* src, void* out_granule, unsigned long long tag);   // the 32-bit word at src (read past the caches) as a granule
void launch_rtt_probe(hipStream_t st, void* out_granule, unsigned long long tag);   // one 16-byte {1.0, tag} granule to mapped host memory
// in/t are in the (Morton-)sorted order with the original index in in[k].w; writes the deskewed point
// to out_sorted[k] (w = original index) and to out_orig[original index]
void launch_deskew(hipStream_t st, const float4* in, const double* t, int n, const void* frames, int nf,
                   const float* mats32, float4* out_sorted, float4* out_orig, double t_offset = 0.0);   // stamp of point k = t[k] + t_offset
void launch_transform(hipStream_t st, const float4* in, int n, const PoseMats& P, float4* out);
// config.debug clouds of the deskew `dk` (n points): deskewed_scan (world frame) and final_raw_scan (moved by P.RT), each at the raw
// point's original index.  false: the staged frames are larger than the kernel takes.
bool launch_deskew_debug(hipStream_t st, const DeskewArgs& dk, int n, const PoseMats& P, float4* out_world, float4* out_final);
size_t dev_frame_size();

// flimo_map.hip
struct MapBuildScratch {
  void* cub_tmp = nullptr;
  size_t cub_tmp_bytes = 0;
  uint32_t* keys_in = nullptr;
  uint32_t* keys_out = nullptr;
  uint32_t* vals_in = nullptr;
  uint32_t* vals_out = nullptr;
  size_t cap_pts = 0;
  unsigned long long *ck_in = nullptr, *ck_out = nullptr;      // 64-bit column keys of the index builds / inserts (flimo_map.hip)
  size_t ck_cap = 0;
  float* bbox = nullptr;   // 6 floats on device (min xyz, max xyz) as ordered ints; armed (empty box) whenever no reduction is running
  // "mail": 64 words of pinned host memory the device writes into (mail_words); the host reads them after synchronising the
  // stream.  Replaces the 4-byte device-to-host copies (each a staged, blocking copy) of counts and boxes.
  uint32_t* mail_host = nullptr;
  uint32_t* mail_dev = nullptr;
  uint32_t mail_seq = 0;
  // the one-launch input filter (filter_raw_scan): per tile {count, launch number} of two sums, then the tile ticket
  unsigned long long* filt_desc = nullptr;
  size_t filt_tiles_cap = 0;
  unsigned int filt_epoch = 0, filt_ticket_base = 0;
  unsigned long long* filt_mail_host = nullptr;   // mapped: four {value, launch number} granules (extreme key, kept count, NaN mark; tied stamps)
  unsigned long long* filt_mail_dev = nullptr;
  // the ordered compaction of a crop (map_crop_compact): per tile {state, count}, then the tile ticket and the kept count
  unsigned long long* crop_desc = nullptr;
  size_t crop_tiles_cap = 0;
  // the range image of a carve (carve_image): [6][res][res] depth bits, then the count word of carve_mask; grown on demand
  unsigned int* carve_img = nullptr;
  size_t carve_img_words = 0;
  // the two counts of a move (seg_move_launch, flimo_segment.hip): points changed, points not finite; zero whenever none is running
  uint32_t* seg_cnt = nullptr;
};
// slots of the mail words
enum MailSlot { MAIL_BOOK = 0 /* 6 */, MAIL_BOOK_END = 8 /* 2 */, MAIL_CROWD = 12, MAIL_BOXCOUNT = 13, MAIL_BBOX = 16 /* 6 */, MAIL_VOXEL = 24 /* 4 */, MAIL_TILES = 28 /* build: tiles, overflow; merge: tiles, overflow */, MAIL_ROWS = 32 /* an insert found the point array or the escape pool full */, MAIL_ESCAPES = 33 /* escape slots a full layout asked for */, MAIL_CROP = 36 /* kept count of a crop */, MAIL_CARVE = 37 /* points a scan sees through */, MAIL_SEG = 38 /* 2: points a move changes, points it leaves not finite */,
                MAIL_TAG = 62 /* number of the last mail_words, written behind its words */, MAIL_WORDS = 64 };
struct MailPart { const void* src; int n; int dst; };
// queues ONE small kernel that copies up to 6 runs of words into the mail slots; `rearm_bbox`: S.bbox is reset to the empty box
// after it has been copied; `zero` / `zero_n`: words set to 0 after the copy (counters for the next round).  No synchronisation.
hipError_t mail_words(hipStream_t st, MapBuildScratch& S, const MailPart* parts, int nparts, bool rearm_bbox = false, void* zero = nullptr,
                      int zero_n = 0);
hipError_t ensure_mail(MapBuildScratch& S);
hipError_t mail_wait(hipStream_t st, MapBuildScratch& S);   // the words of the last mail_words are in S.mail_host (spins on their tag)
// Forgetting (flimo_map_crop_box): the points of in[0 .. n) inside [lo, hi] (inclusive, float32 compares) go to out[0 ..) in their
// order, w = new index -- one launch that reads the map once and writes the kept part once (`blocks` workgroups take tiles by
// ticket); *kept and the kept points' box bb (untouched when nothing is kept) come back through the mail words.  Ends synchronised.
hipError_t map_crop_compact(hipStream_t st, const float4* in, size_t n, const float lo[3], const float hi[3], float4* out, int blocks,
                            MapBuildScratch& S, size_t* kept, float bb[6]);

// Seeing through (flimo_map_seen_through / flimo_map_carve).  cfg: sensor origin (world frame), cube-face resolution, window
// half-width, margins, depth bound.  carve_image: the range image of the scan at pose P (cleared, then one minimum per scan point
// that has a pixel) into S.carve_img; no synchronisation.  carve_mask: d_mask[i] (may be null) = 1 where in[i] is seen through that
// image, *count of them; ends synchronised.  map_carve_compact: map_crop_compact with "not seen through, and inside [lo, hi]
// where both are given" as the kept points.
struct CarveCfg { float s[3]; int res, win; float margin, rel_margin, max_depth; };
hipError_t carve_image(hipStream_t st, const float4* scan, size_t n, const PoseMats& P, const CarveCfg& cfg, MapBuildScratch& S);
hipError_t carve_mask(hipStream_t st, const float4* in, size_t n, const CarveCfg& cfg, MapBuildScratch& S, unsigned char* d_mask, size_t* count);
hipError_t map_carve_compact(hipStream_t st, const float4* in, size_t n, const CarveCfg& cfg, const float* lo, const float* hi, float4* out,
                             int blocks, MapBuildScratch& S, size_t* kept, float bb[6]);

// map_crop_compact with "index outside [first, first + n_mask), or d_mask[index - first] == 0" as the kept points
// (flimo_map_remove_outliers); d_mask: device, [n_mask]
hipError_t map_mask_compact(hipStream_t st, const float4* in, size_t n, const unsigned char* d_mask, size_t first, size_t n_mask, float4* out,
                            int blocks, MapBuildScratch& S, size_t* kept, float bb[6]);

// min/max of n float4 points (NaN-free) -> host bbox[6]
hipError_t map_bbox(hipStream_t st, const float4* pts, size_t n, MapBuildScratch& S, float bbox_host[6]);
// Spatial (Morton) sort of the scan: out[i] = (xyz of in[perm[i]], w = bit pattern of perm[i]).
// Optionally permutes a per-point double array (times) the same way.
hipError_t sort_scan(hipStream_t st, const float4* in, size_t n, float4* out, MapBuildScratch& S,
                     const double* t_in = nullptr, double* t_out = nullptr);
// the same layout without re-ordering (out[i] = (xyz, w = i)): for a sweep a voxel filter re-orders anyway
hipError_t index_scan(hipStream_t st, const float4* in, size_t n, float4* out, const double* t_in, double* t_out);
// The index of a grid (GridView, flimo_types.h) as the host owns it: the pool of tiles (tile 0: all zero), the directory, the
// escape pool and xstart.  map_build_grid sizes and (re)allocates all of it; map_merge_grid takes tiles and escape slots from the
// pools' room and reports when one ran out (index_merge_overflow).
// The escape pool starts at one slot per 16 points of the point buffer's capacity (index_escape_words: 2 bytes per point).  That is
// what a map needs whose crowded columns lie anywhere; the worst case is twice that (16 points in the first column of an x-tile
// take two slots: the segment's own entry and the closing entry of the tile to its left).  A full layout counts the slots it
// asks for and, when the pool was too small, grows it to that count plus a quarter and writes its entries again: it never ends
// with an entry unwritten.  A pool grown that way is kept when the point buffer grows (the larger of the two sizes holds).
constexpr size_t index_escape_words(size_t pts_cap) { return (pts_cap / 16 + 64) * 8; }
struct IndexTables {
  uint2* tiles = nullptr; size_t tiles_cap_entries = 0;
  uint32_t cap_tiles = 0, tiles_used = 0;                 // tiles of the current shape the pool holds / numbers taken at the last build
  TileShape shape{5, 5, 3, 0, 0, 0};                      // the tile shape of the last layout (ts, ty, tz; the extents follow the grid)
  uint16_t* dir = nullptr;                                // GRID_DIR_MAX entries
  uint32_t* need = nullptr;                               // GRID_DIR_MAX words: tiles a batch of new points needs
  uint32_t* counters = nullptr;                           // [0] next free tile number, [1] a merge ran out of tiles, [2] escape slots taken
  uint32_t* ovf = nullptr; size_t ovf_cap = 0;            // words (8 per slot)
  uint32_t* xstart = nullptr; size_t xstart_cap = 0;
  uint32_t* rowcap = nullptr; size_t rowcap_cap = 0;      // [(nz+4)(ny+4)] points that fit from a row's first one to the next row's
  uint32_t* rowoff = nullptr; size_t rowoff_cap = 0;      // build scratch: the rows' first positions
  uint32_t* xstart_alt = nullptr; size_t xstart_alt_cap = 0;      // the second set of the small tables: a grid that grows
  uint32_t* rowcap_alt = nullptr; size_t rowcap_alt_cap = 0;      // (index_regrid) writes it and the two sets change places
  uint16_t* dir_alt = nullptr;
  uint32_t* tail = nullptr;                               // [0] first free position of the point array, [1] an insert found it full, [2] rows moved
};
void index_free(IndexTables& T);
// Sorts `pts_in` by (z, y, fine x column) into the rows of `pts_out` (room for out_cap points) and builds the index (ends with the
// stream waited for once: the pool is sized by the number of tiles the points need).  slack: the rows keep room behind their last
// point (a map that receives inserts) as far as out_cap allows; otherwise they are packed.  pts_cap: capacity of the point buffer
// the index is for (the escape pool's first size; a layout that needs more slots grows the pool and writes its entries again, so
// success means every escape is recorded).  Ends with the stream waited for.
// geo: the grid's geometry (origin, cell, extents, column factor, cell shifts; its table pointers are not looked at).
hipError_t map_build_grid(hipStream_t st, const float4* pts_in, size_t n, float4* pts_out, size_t out_cap, bool slack, IndexTables& T, size_t pts_cap,
                          const GridView& geo, MapBuildScratch& S);
// A grid that grows without a re-sort: N = the new geometry (extents and cell shifts; origin, cell, column factor as O; corner moved
// by whole tiles of O's shape).  hipErrorInvalidValue when the larger grid needs another tile shape (the caller builds afresh).
hipError_t index_regrid(hipStream_t st, IndexTables& T, const GridView& O, GridView& N);
// more room in the pool of tiles before an insert needs it (the tiles move; the caller refreshes its views with index_view)
hipError_t index_grow_pool(hipStream_t st, IndexTables& T, uint32_t cap_tiles_new);
// fills the table pointers and the tile shape of a GridView whose geometry (nx, ny, nz, xs, nxf) is set
void index_view(const IndexTables& T, GridView& G);
// after the stream has been waited for: did a merge since the last build run out of tiles (the index is then incomplete)?
bool index_merge_overflow(const MapBuildScratch& S);
// debug: *diff_dev += the number of (row, column) pairs at which two indices of the same geometry differ
hipError_t index_compare(hipStream_t st, const GridView& A, const GridView& B, unsigned long long* diff_dev);
// Puts the k points appended since the last build into the rows of the cell-sorted array IN PLACE (same geometry): a row whose
// new points fit is merged where it is, a row that outgrows its room moves to the end of the array; the index of the rows that
// received points is rebuilt from those rows.  O(rows + touched rows x row length): no pass over the stored points.  A full array
// or tile pool is reported after the stream has been waited for (index_merge_overflow): the caller lays the map out afresh.
hipError_t map_merge_grid(hipStream_t st, float4* sorted, size_t sorted_cap, const float4* new_pts, size_t k,
                          IndexTables& T, const GridView& geo, MapBuildScratch& S);
// Input filters of a raw sweep (32-byte PointType records already on the device): NaN removal, crop box, every rate-th survivor,
// min distance; order preserved.  out[k] = (xyz, w = k), t_out[k] = stamp without the sweep offset; ext_dev[4] = {extreme ordered
// stamp key (complemented when the sweep is sorted descending), kept count, "a kept stamp is NaN", "two kept stamps are equal"
// (time_order_raw)}; key_out[k] (optional) = ordered stamp key, ascending = the order of the reference's time sort.
hipError_t filter_raw_scan(hipStream_t st, const void* raw32_dev, size_t n, const FilterParams& F, float4* out, double* t_out,
                           unsigned long long* ext_dev, MapBuildScratch& S, unsigned long long* key_out = nullptr, int rec_bytes = 32);
// (rec_bytes 16: records {x, y, z, 32-bit time word} instead of the reference's 32-byte PointType -- time kinds 0 and 1)
// (the three host-side results of the last filter_raw_scan -- extreme key, kept count, NaN mark -- without a copy and a stream wait)
hipError_t filter_raw_scan_result(hipStream_t st, MapBuildScratch& S, const unsigned long long* ext_dev, int timeout_ms, unsigned long long ext3[3]);
hipError_t time_order_raw_tied(hipStream_t st, MapBuildScratch& S, const unsigned long long* ext_dev, int timeout_ms, bool* tied);
// The kept points in the reference's time order (unique when no two stamps are equal; ext_dev[3] = 1 reports equal stamps): stable
// radix sort of the ordered stamp keys filter_raw_scan wrote, pts_out[i] = (xyz of pts[perm_out[i]], w = i), t_out likewise.
hipError_t time_order_raw(hipStream_t st, const float4* pts, const double* t, size_t n, const unsigned long long* keys,
                          unsigned long long* keys_sorted, float4* pts_out, double* t_out, uint32_t* perm_out,
                          unsigned long long* ext_dev, MapBuildScratch& S);
// Second level over crowded regions: box (cell coordinates, inclusive) around the cells holding more than `threshold` points
// (box_host[6] = their number; box_dev: 7 ints of device scratch), and the copy of the map points inside a box of metres
// (w = position in the main sorted map).
hipError_t crowded_list_all(hipStream_t st, const GridView& G, uint32_t threshold, uint32_t* bits,
                            int4* list, uint32_t cap, uint32_t* count_dev, uint32_t* count_host, MapBuildScratch& S);
hipError_t crowded_list_points(hipStream_t st, const float4* pts, size_t k, const GridView& G, uint32_t threshold, uint32_t* bits, int4* list,
                               uint32_t cap, uint32_t* count_dev, uint32_t* count_host, MapBuildScratch& S);
hipError_t crowded_relist(hipStream_t st, const int4* list, uint32_t m, int nx, int ny, int nz, uint32_t* bits, uint32_t* count_dev);
hipError_t map_box_count(hipStream_t st, const GridView& G, const int c0[3], const int c1[3],
                         uint32_t* count_dev, uint32_t* count_host, MapBuildScratch& S);
hipError_t map_box_copy(hipStream_t st, const GridView& G, const int c0[3], const int c1[3], float4* out, MapBuildScratch& S);
hipError_t atan2f_probe(hipStream_t st, const float* yx_host, int n, float* out_host);   // the device's atan2f on n (y, x) pairs
// pcl::VoxelGrid on device points: out gets one centroid per occupied voxel in ascending voxel index
hipError_t voxel_grid(hipStream_t st, const float4* in, size_t n, float leaf, float4* out, size_t* n_out, bool* passthrough,
                      MapBuildScratch& S);
void map_scratch_free(MapBuildScratch& S);

// flimo_radius.hip -- Octree::radiusSearch (Octree.hpp:453-523): the stored points with sqdist3(q, p) < radius * radius, per query.
// Count and fill are ONE walk (same rows, same candidates, same order); lanes per query and the kind of walk (rows of the ball's
// box, or the directory's tiles for a box of many rows) follow from the radius and the grid alone (radius_plan, flimo_radius.h).
// cnt[q] = results of query q; cand (optional): candidates examined per query
hipError_t launch_radius_count(hipStream_t st, const GridView& G, const float* q, int nq, float radius, uint32_t* cnt, unsigned long long* cand);
// offsets[0 .. nq] = exclusive sum of cnt[0 .. nq] (cnt[nq] = 0 set by the caller); tmp == nullptr: tmp_bytes only
hipError_t radius_offsets(hipStream_t st, void* tmp, size_t& tmp_bytes, uint32_t* cnt, unsigned long long* offsets, size_t nq);
// results of query q at offsets[q] ..: insertion index, squared distance, xyz (each optional), or -- keys non-null -- the 64-bit
// keys (distance bits << 32 | insertion index) of the sorted form
hipError_t launch_radius_fill(hipStream_t st, const GridView& G, const float* q, int nq, float radius, const unsigned long long* offsets,
                              int32_t* idx, float* sqd, float* xyz, unsigned long long* keys);
// every segment of the keys ascending (tmp == nullptr: tmp_bytes only), and the keys taken apart (xyz gathered from the map in
// insertion order)
hipError_t radius_sort_segments(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* keys_in, unsigned long long* keys_out,
                                size_t total, size_t nq, const unsigned long long* offsets);
hipError_t launch_radius_unpack(hipStream_t st, const unsigned long long* keys, size_t n, const float4* map_raw, int32_t* idx, float* sqd, float* xyz);

// flimo_cluster.hip -- Euclidean clusters of the stored points (flimo_map_clusters, flimo_c.h): the connected components of
// "sqdist3(p_i, p_j) < tol * tol".  parent, count: [n_map] device words.  init: parent[t] = t, count[t] = 0.  link: the stored
// points first .. first + nq - 1 walk their balls (radius_plan's lanes and walk) and unite with the hits of lower index -- every
// access to parent an agent-scope atomic; run it over the whole map, in chunks.  flatten (a launch of its own): parent[t] = the
// smallest index of t's component, count[that index] = the component's points.  finish: label / size (each may be null) and mask
// of the range [first, first + n), words[4] (zeroed by the caller) += {components, largest (a maximum), selected components} of
// the whole map and the ones of the mask.
hipError_t launch_cluster_init(hipStream_t st, uint32_t* parent, uint32_t* count, size_t n_map);
hipError_t launch_cluster_link(hipStream_t st, const GridView& G, const float4* map_raw, unsigned first, int nq, float tol, uint32_t* parent);
hipError_t launch_cluster_flatten(hipStream_t st, uint32_t* parent, uint32_t* count, size_t n_map);
hipError_t launch_cluster_finish(hipStream_t st, const uint32_t* label_all, const uint32_t* count, size_t n_map, size_t first, size_t n, int min_size,
                                 int max_size, int32_t* label, int32_t* size, unsigned char* mask, uint32_t* words);

// flimo_region.hip -- smooth-surface regions of the stored points (flimo_map_regions, flimo_c.h): the connected components of
// "closer than tol and normals agree" over the SMOOTH points, the predicates of flimo_region.h.  normal: [n_map] rows of
// flimo_map_normals_range (launch_knn_k_normals); parent, count, attach: [n_map] device words.  init: parent[t] = t, count[t] = 0,
// attach[t] = none.  link: the stored points first .. first + nq - 1 walk their balls (radius_plan's lanes and walk); a smooth one
// unites with the smooth hits of lower index whose normal agrees -- every access to parent an agent-scope atomic --, a border one
// (border != 0: it has a normal and is not smooth) records in attach the smooth hit of smallest (distance bits, index) whose normal
// agrees; run it over the whole map, in chunks.  labels (two launches): parent[t] = the label of t -- the smallest index of a smooth
// t's component, the label of attach[t] for a border point, REGION_NONE otherwise --, count[label] = the region's points,
// words[REGION_W_SMOOTH] += the smooth points.  finish:
// label / size / mask (each may be null) of the range [first, first + n), words[REGION_WORDS] (flimo_region.h, zeroed by the caller);
// with keys / vals ([n_map], may be null) the listing's key of every stored point: its label where its region is selected, all ones
// otherwise.  list_labels: label[r] of the listing from the sorted keys and launch_voxel_classify's seg.
hipError_t launch_region_init(hipStream_t st, uint32_t* parent, uint32_t* count, uint32_t* attach, size_t n_map);
hipError_t launch_region_link(hipStream_t st, const GridView& G, const float4* map_raw, const float4* normal, unsigned first, int nq, float tol,
                              float min_cos, float max_curv, int border, uint32_t* parent, uint32_t* attach);
hipError_t launch_region_labels(hipStream_t st, uint32_t* parent, const uint32_t* attach, const float4* normal, float max_curv, uint32_t* count,
                                uint32_t* words, size_t n_map);
hipError_t launch_region_finish(hipStream_t st, const uint32_t* label_all, const uint32_t* count, size_t n_map,
                                size_t first, size_t n, int min_size, int max_size, int32_t* label, int32_t* size, unsigned char* mask,
                                unsigned long long* keys, uint32_t* vals, uint32_t* words);
hipError_t launch_region_list_labels(hipStream_t st, const unsigned long long* keys, const uint32_t* seg, unsigned nr, int32_t* label);

// flimo_knn_k.hip -- Octree::knn (Octree.hpp:526-555) for k up to KNNK_MAX_K with a distance gate: per query the first k stored points
// in the order (float32 squared-distance bits, insertion index) among those with sqdist3(q, p) < max_dist * max_dist (INFINITY: no
// gate).  The running k-best is a list distributed over the lanes that serve the query (knnk_plan lanes, chosen from k); a block
// search near the map, then a best-first walk over the directory's tiles for what it could not prove.  idx / sqd: [nq][k], padded
// with -1 / 0; xyz (optional): [nq][k][3], gathered from map_raw (the map in insertion order); cnt: [nq]; cand (optional): stored
// points each query's walk loaded and tested.  Scratch: work ([nq]) and nwork (one counter): the queries left to the walk over the tiles.
constexpr int KNNK_MAX_K = 64;
int knnk_plan(int k);
hipError_t launch_knn_k(hipStream_t st, const GridView& G, const float4* map_raw, const float* q, int nq, int k, float max_dist, int32_t* idx,
                        float* sqd, float* xyz, int32_t* cnt, unsigned long long* cand, uint2* work, unsigned* nwork);
// The same search, every query finished on the device into the plane normal of its neighbourhood (flimo_map_normals, flimo_c.h):
// mean and covariance of r = p - q in float64, a Jacobi eigen-decomposition, the orientation rule.  q == nullptr: query i is the
// stored point first + i.  normal / cnt: [nq]; centroid [nq][3], cov [nq][6], eig [nq][6]: optional.  Scratch: mom ([nq][9], the
// moments between the searches and the launch that decomposes them), work ([nq]) and nwork (one counter): the queries left to the
// walk over the tiles.
hipError_t launch_knn_k_normals(hipStream_t st, const GridView& G, const float4* map_raw, const float* q, unsigned first, int nq, int k,
                                float max_dist, int min_pts, const float* viewpoint, float4* normal, int32_t* cnt, double* centroid, double* cov,
                                double* eig, double* mom, uint2* work, unsigned* nwork);
// The same search with a list of k + 1 keys for the stored points first .. first + nq - 1 themselves, each ended in its mean
// neighbour distance (flimo_map_outliers, flimo_c.h): the point's own slot dropped, cnt [nq] = the slots left (<= k), mean [nq] =
// kk_slot_sum of the float64 widenings of fl_sqrt(sqd) over them / cnt, NaN for cnt 0.  Scratch: work ([nq]), nwork.
hipError_t launch_outlier_search(hipStream_t st, const GridView& G, const float4* map_raw, unsigned first, int nq, int k, float max_dist,
                                 double* mean, int32_t* cnt, uint2* work, unsigned* nwork);
// The statistics over a range's n slots, T = {i : cnt[i] >= need}, as sums of the shape of flimo_sums.h.  pass 0: out[0] = the bits
// of the float64 sum of mean over T, out[1] = |T|; pass 1: out[0] = the bits of the sum of (mean - mu)^2 over T (out[1] = |T| again).
// part / part_cnt: sum_segments(n) words each; out: two device words.
hipError_t launch_outlier_sum(hipStream_t st, const double* mean, const int32_t* cnt, unsigned n, int need, int pass, double mu, double* part,
                              int32_t* part_cnt, unsigned long long* out);
// mask[i] = cnt[i] < min_pts, or (stat_on and cnt[i] >= need and mean[i] > threshold); counts[0] / counts[1] (device): how many by
// the first / the second rule
hipError_t launch_outlier_mask(hipStream_t st, const double* mean, const int32_t* cnt, unsigned n, int min_pts, int need, bool stat_on,
                               double threshold, unsigned char* mask, unsigned* counts);

// FPFH descriptors of stored points (flimo_map_fpfh, flimo_c.h), after launch_knn_k_normals has left the normals of ALL stored
// points in `normals`.  launch_fpfh_spfh: the search with a list of k keys for the stored points first .. first + nq - 1, each ended
// in the 33 integer counts of its pair features, spfh [map size][33], and the length of its list, len [map size] (rows first ..).
// launch_fpfh_sum: the same search again, each point ended in the weighted sum of its neighbours' rows, every bin one kk_slot_sum,
// each group of 11 scaled to 100: fpfh [nq][33], cnt [nq] (rows 0 ..).  Scratch: work ([nq]), nwork.
hipError_t launch_fpfh_spfh(hipStream_t st, const GridView& G, const float4* map_raw, const float4* normals, unsigned first, int nq, int k,
                            float max_dist, unsigned char* spfh, unsigned char* len, uint2* work, unsigned* nwork);
hipError_t launch_fpfh_sum(hipStream_t st, const GridView& G, const float4* map_raw, const unsigned char* spfh, const unsigned char* len,
                           unsigned first, int nq, int k, float max_dist, float* fpfh, int32_t* cnt, uint2* work, unsigned* nwork);

// ISS keypoints of stored points (flimo_map_keypoints, flimo_c.h).  launch_iss_saliency: launch_knn_k_normals' search and moments
// for the stored points first .. first + nq - 1, each ended by one thread in its saliency -- l0 of flimo_map_normals_range where
// cnt >= max(3, min_pts), l0 > 0, l1 < gamma21 * l2 and l0 < gamma32 * l1 (float64, strict), a quiet NaN otherwise: sal [map size]
// (rows first ..); rcnt (optional) [rn]: cnt of the points inside [rfirst, rfirst + rn).  Scratch: cnt ([nq]), mom ([nq][9]), work
// ([nq]), nwork.  launch_iss_suppress: the search with a list of k keys for the stored points first .. first + nq - 1, each ended
// in mask [nq] (rows 0 ..): salient, and no other point of its list salient with a greater saliency, or an equal one and a lower
// index; *count (device) grows by the ones.  Scratch: work ([nq]), nwork.
hipError_t launch_iss_saliency(hipStream_t st, const GridView& G, const float4* map_raw, unsigned first, int nq, int k, float max_dist, int min_pts,
                               float gamma21, float gamma32, double* sal, unsigned rfirst, unsigned rn, int32_t* rcnt, int32_t* cnt, double* mom,
                               uint2* work, unsigned* nwork);
hipError_t launch_iss_suppress(hipStream_t st, const GridView& G, const float4* map_raw, const double* sal, unsigned first, int nq, int k,
                               float max_dist, unsigned char* mask, unsigned* count, uint2* work, unsigned* nwork);

// The same search with k = 1 for every (pose, point of the resident scan) pair of a chunk of poses (flimo_scan_fitness, flimo_c.h):
// the world point is transform_kernel's, from poses [np][12] (the upper three rows of PoseMats::RT).  sqd [np][n]: the nearest
// stored point's squared distance, -1 for an empty query; idx [np][n] (optional): its insertion index, -1; inliers / sum_sqd [np]:
// the slots that hold a distance and their float64 sum in one fixed shape.  n * np <= 2^31, np <= FIT_MAX_POSES.  Scratch: work
// ([np * n]), nwork.  launch_scan_fitness is its two halves: the two search launches that fill sqd / idx (launch_scan_fit_search, which
// flimo_scan_gicp runs on its own) and the launch that counts and sums them per pose (launch_scan_fit_reduce).
constexpr unsigned FIT_MAX_POSES = 65535;
hipError_t launch_scan_fit_search(hipStream_t st, const GridView& G, const float4* scan, unsigned n, const float* poses, unsigned np, float max_dist,
                                  float* sqd, int32_t* idx, uint2* work, unsigned* nwork);
hipError_t launch_scan_fit_reduce(hipStream_t st, const float* sqd, unsigned n, unsigned np, int32_t* inliers, double* sum_sqd);
hipError_t launch_scan_fitness(hipStream_t st, const GridView& G, const float4* scan, unsigned n, const float* poses, unsigned np, float max_dist,
                               float* sqd, int32_t* idx, uint2* work, unsigned* nwork, int32_t* inliers, double* sum_sqd);

// The normals' search for every (pose, point of the resident scan) pair of a chunk of poses, finished into the pair's
// point-to-plane row {J0..J5, d} and the per-pose sums of the normal equations (flimo_scan_linearize, flimo_c.h).  sums [np][28]:
// the 21 upper-triangle sums of H, the 6 of g, the cost; valid [np].  n * np <= 2^28, np <= FIT_MAX_POSES.
// Scratch per pair: cnt (4 B), mom (72 B), work (8 B), rows (56 B), ok (1 B); per pose and segment of the scan
// (sum_segments(n) of them, flimo_sums.h): part (28 doubles), part_cnt; nwork (one counter).
hipError_t launch_scan_linearize(hipStream_t st, const GridView& G, const float4* map_raw, const float4* scan, unsigned n, const float* poses,
                                 unsigned np, int k, float max_dist, int min_pts, float max_curv, int32_t* cnt, double* mom, uint2* work,
                                 unsigned* nwork, double* rows, unsigned char* ok, double* part, int32_t* part_cnt, double* sums, long long* valid);

// flimo_corr.hip -- pose hypotheses from point correspondences (flimo_corr_poses, flimo_c.h) for a chunk of nh triplets tri [nh][3]
// (every index already checked to lie in [0, m)) over the clouds src / dst [m][3], packed xyz: the solve per hypothesis (status
// [nh], pose [nh][7]; NaN unless OK), then for the OK ones the count of the pairs their float32 matrix brings within max_dist
// (inliers / sum_sqd [nh], 0 for the others; pair_sqd [nh][m], optional: the squared distance, -1 for a non-inlier).  nh * m < 2^31
// when pair_sqd is given.  Scratch: rt ([nh][12]), surv ([nh]), nsurv.
hipError_t launch_corr_poses(hipStream_t st, const float* src, const float* dst, unsigned m, const int32_t* tri, unsigned nh, float edge_sim,
                             float min_edge, float max_dist, int32_t* status, double* pose, float* rt, int32_t* surv, unsigned* nsurv,
                             int32_t* inliers, double* sum_sqd, float* pair_sqd);
// ... and the consistency graph of the correspondences (flimo_corr_graph, flimo_c.h), 0 < m <= FLIMO_CORR_GRAPH_MAX_M.
// launch_corr_adjacency: two launches -- the bit matrix adj [m][(m + 63) / 64], then the rows' popcounts to degree [m] and to c0 [m],
// the start of the core iteration.  launch_corr_core_rounds enqueues `rounds` rounds of the h-index iteration between the two
// buffers c[0] / c[1] (*cur names the one that holds the estimate, before and after); round r leaves flags[r] != 0 iff it changed
// an estimate (flags [rounds] is cleared first).  The estimates are the core numbers once a round changed nothing.
hipError_t launch_corr_adjacency(hipStream_t st, const float* src, const float* dst, unsigned m, float tol, float min_edge, float edge_sim,
                                 uint64_t* adj, int32_t* degree, int32_t* c0);
hipError_t launch_corr_core_rounds(hipStream_t st, const uint64_t* adj, unsigned m, int32_t* c[2], int* cur, unsigned* flags, int rounds);

// flimo_plane.hip -- RANSAC planes of the stored points (flimo_map_planes, flimo_c.h) for a chunk of k triplets tri [k][3] (every
// index already checked to lie in [0, N)) over the N > 0 stored points map_raw: the solve per hypothesis (status [k], plane [k][4];
// NaN unless OK), then for the OK ones the count over ALL stored points in slabs of PLANE_SLAB (flimo_plane.h) and the finish
// (inliers / sum_sq [k], 0 for the others).  Three launches, no wait.  Scratch: rec ([k][2] float4), surv ([k]), nsurv, part_cnt /
// part_sum ([plane_slabs(N)][k]).
hipError_t launch_plane_chunk(hipStream_t st, const float4* map_raw, unsigned N, const int32_t* tri, unsigned k, float dist, float min_edge,
                              float min_sin, const float axis[3], float min_cos, int32_t* status, double* plane, int32_t* inliers,
                              double* sum_sq, float4* rec, int32_t* surv, unsigned* nsurv, int32_t* part_cnt, double* part_sum);
// mask [n] (may be null) of the stored points first .. first + n - 1 against one plane (flimo_map_plane_mask); *count (zeroed by the
// caller) += the ones
hipError_t launch_plane_mask(hipStream_t st, const float4* map_raw, unsigned first, unsigned n, const float normal[3], const float anchor[3],
                             float dist, int side, unsigned char* mask, unsigned* count);

// flimo_voxel.hip -- voxel statistics of the stored points (flimo_map_voxels, flimo_c.h), in stages on one stream; words
// [VOXEL_WORDS] (flimo_voxel.h) is zeroed by the caller, tmp holds voxel_tmp_bytes(n).
//  launch_voxel_sort      keys, the stable sort (keys_out / vals_out: sorted keys and the insertion index of every sorted position),
//                         head flags and their exclusive scan pos; words[VOXEL_W_OUTSIDE] += the outside points.  The caller
//                         reads nv = pos[n - 1] + head[n - 1] and the outside count before the next stage.
//  launch_voxel_classify  seg [nv + 1], ijk [nv][3] (may be null), first [nv], count [nv], words[VOXEL_W_LARGEST]; with lists ([4][nv]; null: no
//                         moments are wanted) the voxels of each lane plan (lengths in words[VOXEL_W_LIST ..]), runs [nv + 1] and
//                         their exclusive scan roff [nv + 1] (roff[nv]: the run slots R the many-runs path needs).
//  launch_voxel_moments   centroid [nv][3] and, with second, cov [nv][6] and rep [nv]; pts is read through gather (null: pts is
//                         in sorted order, launch_voxel_sorted_copy); rs [R][3], rc [R][6], rq [R], rp [R]: the run slots.
//  launch_voxel_points    voxel [nr] / mask [nr] (may be null) of the stored points first .. first + nr - 1 and
//                         words[VOXEL_W_SEL] += the ones; rep is read for VOXEL_KEEP_NEAREST only.
hipError_t voxel_tmp_bytes(size_t n, size_t* bytes);
hipError_t launch_voxel_sort(hipStream_t st, const float4* map_raw, unsigned n, float inv, unsigned long long* keys_in, unsigned long long* keys_out,
                             uint32_t* vals_in, uint32_t* vals_out, uint32_t* head, uint32_t* pos, void* tmp, size_t tmp_bytes, uint32_t* words);
// ... the same behind ready keys (keys_in / vals_in [n], filled by the caller; all ones: the point belongs to no segment)
hipError_t launch_voxel_sort_keys(hipStream_t st, unsigned n, unsigned long long* keys_in, unsigned long long* keys_out, uint32_t* vals_in,
                                  uint32_t* vals_out, uint32_t* head, uint32_t* pos, void* tmp, size_t tmp_bytes);
hipError_t launch_voxel_classify(hipStream_t st, const unsigned long long* keys, const uint32_t* perm, const uint32_t* head, const uint32_t* pos,
                                 unsigned n, unsigned nv, unsigned inside, int plan, uint32_t* seg, int32_t* ijk, int32_t* first, int32_t* count,
                                 uint32_t* runs, uint32_t* roff, uint32_t* lists, void* tmp, size_t tmp_bytes, uint32_t* words);
hipError_t launch_voxel_sorted_copy(hipStream_t st, const float4* map_raw, const uint32_t* perm, unsigned n, float4* out);
hipError_t launch_voxel_moments(hipStream_t st, const float4* pts, const uint32_t* gather, const uint32_t* perm, const uint32_t* seg, unsigned nv,
                                const uint32_t* lists, const unsigned nlist[4], const uint32_t* roff, unsigned R, int second, double* rs,
                                double* rc, double* rq, uint32_t* rp, double* centroid, double* cov, int32_t* rep);
hipError_t launch_voxel_points(hipStream_t st, const unsigned long long* keys, const uint32_t* perm, const uint32_t* head, const uint32_t* pos,
                               const uint32_t* seg, const int32_t* rep, unsigned n, unsigned first, unsigned nr, int keep, unsigned max_pts,
                               int32_t* voxel, unsigned char* mask, uint32_t* words);

// flimo_desc.hip -- nearest descriptors (flimo_desc_match, flimo_c.h).  The resident reference set is two arrays: norm
// [ceil(nr / 32) * 32] (launch_desc_norms with npad = that; NaN for an excluded row and for the padding) and rt
// [ceil(nr / 32)][desc_steps(dim)][64], the rows in the MFMA's A-operand layout (launch_desc_pack).  launch_desc_match answers a
// chunk of nq queries q [nq][dim] against it: the queries' norms (qnorm [nq], scratch), the match over splits of tiles_per_split
// >= 1 reference tiles each (part: scratch, [splits][nq][desc_list_len(k)] keys; splits <= 65535), the merge into idx / dist
// [nq][k] and cnt [nq].  A workgroup of the match takes desc_query_tile(dim) queries.
int desc_steps(int dim);
int desc_query_tile(int dim);
int desc_list_len(int k);
hipError_t launch_desc_norms(hipStream_t st, const float* x, unsigned n, int dim, float* norm, unsigned npad);
hipError_t launch_desc_pack(hipStream_t st, const float* x, unsigned n, int dim, float* rt);
hipError_t launch_desc_match(hipStream_t st, const float* rt, const float* rnorm, unsigned nr, unsigned tiles_per_split, const float* q,
                             float* qnorm, unsigned nq, int dim, int k, unsigned long long* part, int32_t* idx, float* dist, int32_t* cnt);

// flimo_sc.hip -- Scan Context (flimo_scan_context, flimo_sc_db_*, flimo_sc_match; flimo_c.h, flimo_sc.h).
//  launch_sc_descriptor  desc [rings][sectors] and *used (both device) of the scan's n points: the zeroing and one launch.
//  launch_sc_norms       the normalised form of n descriptors raw [n][rings][sectors]: un [n][rings][64], valid [n] (the bits of
//                        the valid columns; 0 for an excluded descriptor).
//  launch_sc_match       a chunk of nq queries in that form against the entries [e_first, e_end) of the database, in splits of
//                        per_split entries (splits <= 65535): part / part_shift [splits][nq][sc_list_len()] scratch, then idx /
//                        dist / shift [nq][k], cnt [nq] and, unless null, profile [nq][k][sectors].  A workgroup takes
//                        sc_query_tile() queries.
struct ScBinCfg;
int sc_query_tile();
int sc_list_len();
hipError_t launch_sc_descriptor(hipStream_t st, const float4* scan, unsigned n, const ScBinCfg& K, float* desc, int* used);
hipError_t launch_sc_norms(hipStream_t st, const float* raw, unsigned n, int rings, int sectors, float* un, unsigned long long* valid);
hipError_t launch_sc_match(hipStream_t st, const float* un, const unsigned long long* valid, unsigned e_first, unsigned e_end, unsigned per_split,
                           const float* qun, const unsigned long long* qvalid, unsigned nq, int rings, int sectors, int k, int min_cols,
                           float max_dist, unsigned long long* part, int* part_shift, int32_t* idx, float* dist, int32_t* shift, int32_t* cnt,
                           float* profile);

// flimo_ndt.hip -- the NDT cell model and the per-pose sums against it (flimo_ndt_build, flimo_scan_ndt; flimo_c.h).
//  launch_ndt_cells   behind launch_voxel_moments: eig [nv][12] (l0 l1 l2, v0, v1, v2 of every voxel of at least min_pts points),
//                     flag [nv + 1] (1: a cell; flag[nv] = 0) and its exclusive scan pos [nv + 1]: pos[nv] is the number of cells.
//                     tmp holds ndt_tmp_bytes(nv).
//  launch_ndt_pack    keys / cnt / eval [nc][3] / cells [nc] (128-byte records, flimo_ndt.h) of the cells, ascending key.
//  launch_scan_ndt    a chunk of np poses (np <= FIT_MAX_POSES, n * np <= 2^28): cell / e [np * n * hood] and m (may be null) per
//                     (pair, neighbour slot); part [np * segments][28], part_cnt [np * segments][2]; sums [np][28], counts [np][2]
//                     (pairs with a live term, live terms).  nc >= 1.
hipError_t ndt_tmp_bytes(size_t nv, size_t* bytes);
hipError_t launch_ndt_cells(hipStream_t st, const int32_t* count, const double* cov, unsigned nv, int min_pts, double* eig, uint32_t* flag,
                            uint32_t* pos, void* tmp, size_t tmp_bytes);
hipError_t launch_ndt_pack(hipStream_t st, const uint32_t* flag, const uint32_t* pos, const int32_t* ijk, const int32_t* count, const double* centroid,
                           const double* eig, unsigned nv, double eig_ratio, unsigned long long* keys, int32_t* cnt, double* eval, void* cells);
hipError_t launch_scan_ndt(hipStream_t st, const float4* scan, unsigned n, const float* poses, unsigned np, int hood, float inv, double d2,
                           const unsigned long long* keys, const void* cells, unsigned nc, int32_t* cell, double* e, double* m, double* part,
                           int32_t* part_cnt, double* sums, long long* counts);

// flimo_gicp.hip -- the GICP covariance model and the per-pose sums against it (flimo_gicp_build, flimo_scan_gicp; flimo_c.h).
//  launch_gicp_pack   behind launch_knn_k_normals: out [n][6] = gicp_regularize (flimo_gicp.h) of cov [n][6], six NaN where there
//                     is none; *count (device) grows by the rows that got one.
//  launch_scan_gicp   a chunk of np poses (np <= FIT_MAX_POSES, n * np <= 2^28): launch_scan_fit_search into sqd / idx [np * n] (idx
//                     is required), then the terms against model [map size][6] and scan_cov [n][6]: pair_m [np * n] (may be null;
//                     NaN for an invalid pair), part [np * segments][28], part_cnt [np * segments]; sums [np][28], valid [np].
hipError_t launch_gicp_pack(hipStream_t st, const double* cov, unsigned n, int rule, double eps, double* out, unsigned* count);
hipError_t launch_scan_gicp(hipStream_t st, const GridView& G, const float4* map_raw, const float4* scan, unsigned n, const float* poses, unsigned np,
                            float max_dist, const double* model, const double* scan_cov, float* sqd, int32_t* idx, uint2* work, unsigned* nwork,
                            double* pair_m, double* part, int32_t* part_cnt, double* sums, long long* valid);

}  // namespace flimo
