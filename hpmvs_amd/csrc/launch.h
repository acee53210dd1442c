// launch.h -- host-callable launchers of the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

#include "conflicts.hpp"
#include "level_walk.hpp"
#include "dev_types.h"
#include "jpeg.hpp"
#include "jpeg_enc.hpp"
#include "octree.hpp"
#include "seed_tree.hpp"

namespace hpmvs {

// CellProcessor::regularize over a versioned leaf table (kernel_regularize.hip, include/hpmvs_amd.h: hpmvs_regularize_batch).
// Kept out of dev_types.h, whose hash is part of the refinement kernel's build id.
constexpr int kRegMaxDepth = 21;   // 3 bits per level below the sentinel bit of a 64-bit path key
struct RegTree {
    float root[4];                     // c_ (3), width_ of the Branch the probes descend from
    int32_t n;                         // nonempty leaves
    int32_t slots;                     // hash slots (power of two, >= 2 n)
    const float* cell_center;          // [n][3] Leaf::c_
    const float* cell_width;           // [n]
    const float* patch_center;         // [n][3] data[0]->center_
    const int32_t* born;               // [n] the leaf exists at queue positions born < q < died
    const int32_t* died;
    unsigned long long* keys;          // [slots] path keys, 0 = free
    int32_t* vals;                     // [slots] leaf index
};
struct RegCells {
    int32_t n, ref_stride;
    const float* center; const float* normal;   // [n][4]
    const int32_t* ref;                          // images_[0] at ref[i * ref_stride]
    const float* width;                          // [n] leaf width_
    const int32_t* position;                     // [n] queue position
    const uint8_t* expanded;                     // [n]
    float* flatness;                             // [n] written for expanded cells only
    int32_t* n_neighbours;                       // [n] -1: not expanded
    int32_t* neighbour;                          // [n][24] or null
};


void launch_half_resize(const uint8_t* src, int w, int h, uint8_t* dst, hipStream_t st);
// level-0 radial undistortion (kernel_undistort.hip): dst [h][w][3] u8, src read only; xy [h][w][2] source points
void launch_undistort(const uint8_t* src, int w, int h, float f, float k1, uint8_t* dst, hipStream_t st);
void launch_undistort_map(int w, int h, float f, float k1, float* xy, hipStream_t st);
void launch_objective(const DevScene& sc, const DevOptions& o, const DevBatch& b, const double* xs, double* f_out,
                      int32_t* ngrabs_out, hipStream_t st);
// the same values from the one-lane-per-grab kernel (kernel_objective_lane.hip)
void launch_objective_lane(const DevScene& sc, const DevOptions& o, const DevBatch& b, const double* xs, double* f_out,
                           int32_t* ngrabs_out, hipStream_t st);
void launch_inccs(const DevScene& sc, const DevOptions& o, const DevBatch& b, int ref_idx, int robust, float* out,
                  hipStream_t st);
// The scene-centre sphere of Scene::initPatches (reference src/hpmvs/Scene.cpp:118-121), passed to seed_init_kernel by value.
// on == 0: no gate.  Kept out of dev_types.h like RegTree above.
struct SeedSphere {
    double c[3];
    double r;
    int32_t on;
};
void launch_seed_init(const DevScene& sc, const DevOptions& o, int start_level, int n, const double* xyz,
                      const int32_t* meas_off, const int32_t* meas_img, const SeedSphere& sphere, const DevBatch& b,
                      hipStream_t st);
void launch_drift_gate(int n, const double* xyz, const DevBatch& b, hipStream_t st);
// CellProcessor::extend / ::branch candidates (mode 0 / 1): parents -> out (n * N patches), and the gates after optimize
int expand_fanout(int mode);
const float* expand_direction_table(int mode);
void launch_expand_init(const DevScene& sc, int mode, int n, const DevBatch& parents, const float* cell_center,
                        const float* cell_width, const uint8_t* skip, const DevBatch& out, hipStream_t st);
void launch_expand_gate(int mode, int n, const DevBatch& parents, const float* cell_center, const float* cell_width,
                        const DevBatch& out, hipStream_t st);
// workspace: optimize_workspace_bytes(n_cus) bytes per in-flight launch; its first 1 KB (work-queue counter)
// must be zero when the kernel starts
size_t optimize_workspace_bytes(int n_cus);
void launch_optimize(const DevScene& sc, const DevOptions& o, const DevBatch& b, int32_t* workspace,
                     int n_cus, hipStream_t st);
// open batch (DevBatch::svc_ctrl set, arrays host-mapped): `wgs` persistent workgroups, workspace of
// optimize_workspace_bytes_for(wgs) bytes with a zeroed first 1 KB
size_t optimize_workspace_bytes_for(int wgs);
size_t optimize_stage_bytes_for(int wgs);  // the slots' staging records (DevBatch::svc_stage)
void launch_optimize_service(const DevScene& sc, const DevOptions& o, const DevBatch& b, int32_t* workspace, int wgs,
                             hipStream_t st);

// depth maps and the acceptance gates over them (kernel_depth.hip)
void launch_depth_fill(float* p, size_t n, hipStream_t st);
void launch_set_depths(const DevScene& sc, const DevDepthView* depths, const DevBatch& b, hipStream_t st);
void launch_depth_gates(const DevScene& sc, const DevDepthView* depths, const DevBatch& b, float margin, int abs_int,
                        int32_t* n_visible, int32_t* n_blocking, int32_t* n_free, hipStream_t st);

// Scene::setDepths(patch, subtract) in call order (keys -> sort -> per-cell replay) and Scene::getLevelSupport
void launch_level_support(const DevScene& sc, const DevBatch& b, int min_level, int32_t* support, hipStream_t st);
void launch_depth_ops_keys(const DevScene& sc, const DevDepthView* depths, const float* pool, const DevBatch& b, unsigned long long* keys,
                           unsigned int* counter, hipStream_t st);
int depth_ops_sort(void* temp, size_t* temp_bytes, const unsigned long long* keys_in, unsigned long long* keys_out, unsigned int count, hipStream_t st);
void launch_depth_ops_apply(const DevScene& sc, const DevDepthView* depths, float* pool, const DevBatch& b, const uint8_t* subtract,
                            const unsigned long long* keys, unsigned int count, hipStream_t st);

// a view's depth maps as jet-coloured images (kernel_depth_vis.hip, depth_vis.hpp, include/hpmvs_amd.h: hpmvs_scene_depth_image).
// level >= 0: that level's map, W x H its cols x rows; level < 0: the combined image over n_levels levels, W x H level 0's.
// vals: [H][W] float; part: 2 * depth_vis_partials(W, H) floats; lut: dvis::make_colormap's bytes on the device; rgb: [H][W][3];
// range: 2 floats, m and M as used.
unsigned depth_vis_partials(int W, int H);
void launch_depth_vis_gather(const DevDepthView& D, int n_levels, int level, int W, int H, float* vals, float* part, hipStream_t st);
void launch_depth_vis_colour(const float* vals, size_t n, const float* part, unsigned n_part, const uint8_t* lut, uint8_t* rgb, float* range,
                             hipStream_t st);

// the patch cloud as DynOctTree::toExtPly's file (kernel_ply.hip, ply_text.hpp, include/hpmvs_amd.h: hpmvs_ply_ext_batch).  Row r of the
// file is patch order[r] (order == nullptr: patch r).  rec: [10][n_rows] digit records, ASCII only; len: [2 n_rows + 1] the rows'
// vertex lengths, then their list lengths, then 0 (the caller zeroes the last entry); err: one word, UINT_MAX before -- 2 row + kind
// of the lowest bad row behind launch_ply_len (kind 0: its order entry is outside [0, n), 1: its n_images outside [0, max_images]).
// offs: the exclusive scan of len (jpeg_enc_scan), offs[2 n_rows] the body's length; body: the file behind its header.  The two
// write launches go only behind a clean error word.
struct PlyRows {
    int32_t n, max_images, n_rows, flags;   // flags: HPMVS_PLY_*
    const float *center, *normal, *scale, *color;
    const int32_t *n_images, *images, *order;
    uint32_t* rec;
    unsigned long long* len;
    unsigned int* err;
};
void launch_ply_len(const PlyRows& A, hipStream_t st);
void launch_ply_vertex(const PlyRows& A, const unsigned long long* offs, uint8_t* body, hipStream_t st);
void launch_ply_list(const PlyRows& A, const unsigned long long* offs, uint8_t* body, hipStream_t st);

// the cells a batch's gates read and setDepths would write (the scheduler's conflict test; layouts at the kernel)
void launch_depth_footprints(const DevScene& sc, const DevDepthView* depths, const DevBatch& b, int32_t* wr, int32_t* fr, int32_t* at,
                             int32_t* vb, hipStream_t st);

// CellProcessor::regularize (kernel_regularize.hip): leaf keys + checks + hash table (hdr[0]: error bits, hdr[1]: deepest leaf, hdr[2]: 22 - shallowest), then
// one launch over the cells
void launch_regularize_leaves(const RegTree& t, int n_cells, int n_views, const int32_t* ref, int ref_stride, const int32_t* n_images,
                              const uint8_t* expanded, int32_t* hdr, hipStream_t st);
void launch_regularize(const DevScene& sc, const RegTree& t, const RegCells& cl, int min_depth, int max_depth, hipStream_t st);

// CellProcessor::filter (kernel_filter.hip): bad[0] |= 1 unless cell_start[0] == 0, non-decreasing, cell_start[n_cells] == n; then
// dist[n] per row and keep[n_cells] per cell (row of the kept patch, -1: empty cell, -2: no winner)
void launch_filter_check(const int32_t* cell_start, int n_cells, int n, int32_t* bad, hipStream_t st);
void launch_filter(const float* center, const float* normal, const int32_t* cell_start, int n_cells, int n, float* dist, int32_t* keep,
                   hipStream_t st);

// the seed octree of Scene::initPatches (kernel_seed_tree.hip, include/hpmvs_amd.h: hpmvs_seed_tree_batch).  blk: the call's
// device record -- bounding box as ordered integers, rows with ok != 0, refusal flag, then the hpmvs_seed_tree_info the host reads
constexpr int kSeedBlkMin = 0, kSeedBlkMax = 3, kSeedBlkRows = 6, kSeedBlkBad = 7, kSeedBlkInfo = 8, kSeedBlkInts = 16;
struct SeedTreeScratch {
    int32_t* blk;                            // [kSeedBlkInts]
    unsigned long long *key_a, *key_b;       // [n] each
    int32_t *row_a, *row_b, *dep, *depth;    // [n] each
    seed::Clamp *pair_a, *pair_b, *pair_c;     // [n] each
    void* temp;                              // seed_tree_temp_bytes(n)
    size_t temp_bytes;
};
struct SeedTreeOut {
    int32_t* rows; int32_t* cell_start; float* cell_center; float* cell_width; int32_t* cell_level; float* patch_center;
};
size_t seed_tree_temp_bytes(int n);
// enqueues steps 1-7 on st; != 0: a rocPRIM call failed.  A root that is not finite sets blk[kSeedBlkBad] and nothing is written.
int launch_seed_tree(const float* center, float* scale, const uint8_t* ok, int n, int maxlevel, const SeedTreeScratch& s,
                     const SeedTreeOut& out, hipStream_t st);

// leaf look-ups in the scheduler's octree (kernel_octree.hip, octree.hpp, include/hpmvs_amd.h: hpmvs_octree_locate_batch).
// launch_octree_build enters the branch keys (value -2) and the nonempty leaves' keys (value: index) into the table keys / vals
// (`slots` entries, keys zeroed by the caller) and then checks it: *verdict collects octree::kBad* bits.  Every output of
// launch_octree_locate is nullable; root = c_ (3), width_.
struct OctreeLocateOut {
    uint8_t* inside; unsigned long long* leaf_key; int32_t* leaf_index; float* leaf_width; float* leaf_center; unsigned long long* target_key;
};
void launch_octree_build(const unsigned long long* branch_key, int nb, const unsigned long long* leaf_key, int nl, unsigned long long* keys,
                         int32_t* vals, uint32_t slots, int32_t* verdict, hipStream_t st);
void launch_octree_locate(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots, int n,
                          const float* points, const float* add_width, const OctreeLocateOut& out, hipStream_t st);

// the look-ups of CellProcessor::extend around the refinement of one expansion call (kernel_extend_tree.hip, include/hpmvs_amd.h:
// hpmvs_extend_tree_batch), against the table launch_octree_build made.  n: candidates (out.n); `width` the level's leaf width.
// The pre kernel goes between launch_expand_init and the refinement (it reads out.center and sets out.n_images of a skipped
// candidate to -20), the post kernel behind launch_expand_gate (it reads out.center / out.ok).  Every output is nullable; what is
// given is written in every entry.
struct ExtendTreeOut {
    uint8_t* skip; uint8_t* pre_inside; unsigned long long* pre_key; uint8_t* border; unsigned long long* post_key;
};
void launch_extend_tree_pre(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots, int n, float width,
                            const DevBatch& out, const ExtendTreeOut& k, hipStream_t st);
void launch_extend_tree_post(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots, int n, float width,
                             const DevBatch& out, const ExtendTreeOut& k, hipStream_t st);

// the same for a forest (kernel_extend_forest.hip, include/hpmvs_amd.h: hpmvs_extend_forest_batch).  trees: [n_trees] on the
// device, every Table pointing at its tree's slot range of one buffer whose keys the caller zeroed; branch_first / leaf_first:
// [n_trees + 1] on the device; n_keys: all keys of the forest.  verdict: [kForestWords], every word set to octree::kForestGood
// by the caller and folded with min -- the table's finding (octree::forest_finding), the first parent whose parent_tree names no
// tree, the lowest tree with a parent and has_level == 0.  The candidate kernels read parent_tree[i / 6] unchecked: launch them
// only behind a good verdict.
using octree::kForestTable; using octree::kForestParent; using octree::kForestLevel; using octree::kForestWords;   // (octree.hpp: the forest's block)
void launch_forest_build(int n_trees, const int32_t* branch_first, const int32_t* leaf_first, const unsigned long long* branch_key,
                         const unsigned long long* leaf_key, int n_keys, const octree::Tree* trees, uint32_t* verdict, hipStream_t st);
void launch_forest_parents(int n_trees, const uint8_t* has_level, int n, const int32_t* parent_tree, uint32_t* verdict, hipStream_t st);
void launch_extend_forest_pre(const octree::Tree* trees, const int32_t* parent_tree, int n, float width, const DevBatch& out,
                              const ExtendTreeOut& k, hipStream_t st);
void launch_extend_forest_post(const octree::Tree* trees, const int32_t* parent_tree, int n, float width, const DevBatch& out,
                               const ExtendTreeOut& k, hipStream_t st);

// one regularize / settle sweep over a forest (kernel_process_forest.hip, include/hpmvs_amd.h: hpmvs_process_forest_batch),
// against the tables launch_forest_build made.  Everything is on the device.  launch_process_cells folds what it finds wrong with
// a row into verdict[kForestParent] as octree::cell_finding (owner: [all leaves], every word octree::kNoOwner before); the other
// launches go only behind a good verdict, in the order they stand here: skip behind launch_level_support, decide behind
// launch_expand_gate (it reads out.ok / out.center), regularize behind decide, gather behind the exclusive scan of op_count.
struct ProcessCells {
    int32_t n, max_images;
    const int32_t* cell_tree; const unsigned long long* cell_key; const float* flatness;   // [n] the call's inputs
    const int32_t* n_images; const int32_t* images;                                        // of the cells' patches
    int32_t* gleaf;              // [n] the cell's leaf among all leaves of the forest
    int32_t* owner;              // [all leaves] the row that owns the leaf
    float* cell_center;          // [n][3] Cell::c_ by the key
    float* cell_width;           // [n]
    uint8_t* removed; uint8_t* split; uint8_t* children; unsigned long long* child_key;   // [n], [n], [n][4], [n][4]
};
void launch_process_cells(int n_trees, const octree::Tree* trees, const int32_t* leaf_first, int n_views, const ProcessCells& c,
                          uint32_t* verdict, hipStream_t st);
void launch_process_skip(const ProcessCells& c, const int32_t* support, uint8_t* skip, hipStream_t st);
void launch_process_decide(const ProcessCells& c, const int32_t* support, const uint8_t* skip, const uint8_t* final_level, const DevBatch& out,
                           int32_t* op_count, hipStream_t st);
// flatness_out may be c.flatness: a cell's lanes have read its entry before its first lane writes it
void launch_regularize_forest(const DevScene& sc, const octree::Tree* trees, const int32_t* leaf_first, const float* leaf_patch_center,
                              const ProcessCells& c, const DevBatch& par, const DevBatch& out, float* flatness_out, int32_t* n_neighbours,
                              unsigned long long* neighbour_key, hipStream_t st);
// exclusive scan of n ints; temp == nullptr: only reports the temporary bytes rocPRIM needs.  != 0: the rocPRIM call failed
int process_scan(void* temp, size_t* temp_bytes, const int32_t* in, int32_t* out, int n, hipStream_t st);
// ops: op_first[n] rows of max_images ids each (wider lists do not occur: out has the cells' max_images), -1 padded
void launch_process_gather(const ProcessCells& c, const int32_t* op_first, const DevBatch& par, const DevBatch& out, const DevBatch& ops,
                           uint8_t* subtract, hipStream_t st);

// a round's border patches (kernel_octree_insert.hip, include/hpmvs_amd.h: hpmvs_octree_route_batch, hpmvs_octree_insert_batch).
// launch_octree_insert reads the table launch_octree_build made and enqueues static kernel, sort and replay on st; != 0: the
// rocPRIM call failed.  Every entry of every output is written (blocker is nullable).  roots: [n_trees][4] c_, width_ on the device.
struct OctreeInsertOut {
    uint8_t* accepted; unsigned long long* leaf_key; int32_t* blocker;
};
struct OctreeInsertScratch {
    unsigned long long *path, *key_a, *key_b, *acc_key;   // [n] each
    uint32_t *val_a, *val_b;                              // [n] each
    int32_t* acc_owner;                                   // [n]
    void* temp;                                           // octree_insert_temp_bytes(n)
    size_t temp_bytes;
};
size_t octree_insert_temp_bytes(int n);   // (size_t)-1: the size query failed
int launch_octree_insert(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots, int n,
                         const float* points, const float* add_width, const OctreeInsertScratch& s, const OctreeInsertOut& out,
                         hipStream_t st);
void launch_octree_route(int n_trees, const float* roots, int n, const float* points, int32_t* tree, hipStream_t st);

// a round's border queue over a forest (kernel_border_forest.hip, include/hpmvs_amd.h: hpmvs_border_forest_batch), against the
// tables launch_forest_build made: static kernel (route, locate, refusal, path), two stable sorts (leaf key, then tree id), replay
// with one wavefront per (tree, leaf key) run, all enqueued on st; != 0: a rocPRIM call failed.  center: [n][4], scale: [n] of the
// patch batch.  Every output is nullable; what is given is written in every entry.  n_trees == 0: trees may be null.
struct BorderForestOut {
    int32_t* tree; uint8_t* accepted; unsigned long long* leaf_key; int32_t* blocker;
};
struct BorderForestScratch {
    unsigned long long *path, *key_a, *key_b, *acc_key;   // [n] each
    uint32_t *val_a, *val_b, *tree_a, *tree_b, *tree_c;   // [n] each
    int32_t* acc_owner;                                   // [n]
    void* temp;                                           // border_forest_temp_bytes(n, n_trees)
    size_t temp_bytes;
};
size_t border_forest_temp_bytes(int n, int n_trees);   // (size_t)-1: a size query failed
int launch_border_forest(int n_trees, const octree::Tree* trees, int n, const float* center, const float* scale,
                         const BorderForestScratch& s, const BorderForestOut& out, hipStream_t st);

// an extend level's conflict graph (kernel_conflicts.hip, conflicts.hpp, include/hpmvs_amd.h: hpmvs_level_conflicts_batch).
// launch_conflicts builds the sorted, unique pairs of the device footprints F and writes the n + 1 offsets of both lists; it is
// host-synchronous (three counts are read back) and takes its device memory from `scratch`, which must outlive the adjacency
// launch.  kConflictsTooMany: more raw pairs than conflicts::kMaxRawPairs, nothing written.  launch_conflicts_adjacency cuts the
// pairs into the two adjacency arrays (flow_adj[n_flow], anti_adj[n_anti]).
constexpr int kConflictsOk = 0, kConflictsHip = 1, kConflictsMemory = 2, kConflictsTooMany = 3;
int launch_conflicts(const conflicts::Footprints& F, const std::function<void*(size_t)>& scratch, uint32_t* flow_off, uint32_t* anti_off,
                     const unsigned long long** pairs_out, uint32_t* n_flow, uint32_t* n_anti, hipStream_t st);
void launch_conflicts_adjacency(const unsigned long long* pairs, uint32_t n_flow, uint32_t n_anti, uint32_t* flow_adj, uint32_t* anti_adj,
                                hipStream_t st);

// an extend level's wave walk (kernel_level_walk.hip, level_walk.hpp, include/hpmvs_amd.h: hpmvs_level_walk_batch).  The entry point
// strings these together with the graph, gate and depth-op launches above; every launch is a kernel of its own on `st`.  walk_scan
// and the two sorts follow depth_ops_sort: temp == nullptr reports the temporary bytes; != 0: the rocPRIM call failed.
// ctl: [0] pending items, [1] the refined candidates among them, [2] decided in this wave, [3] its ops, [4] the subtractions among them.
struct WalkArrays {
    uint8_t *state, *ok;
    int32_t *slot_of, *gv, *gb, *gf;
    const int32_t* n_images;
    int32_t *stage, *counts, *wave;
    uint8_t* accepted;
};
void launch_walk_check(int n, const uint8_t* flags, const int32_t* set, unsigned int* bad, hipStream_t st);
int walk_scan(void* temp, size_t* temp_bytes, const uint32_t* in, uint32_t* out, int n, hipStream_t st);
void launch_walk_mark(int n, const uint8_t* flags, uint32_t* mark, hipStream_t st);
void launch_walk_nodes(int n, const uint8_t* flags, const uint32_t* mark, const uint32_t* scan, int32_t* node_of, int32_t* item_of,
                       uint8_t* node_event, uint8_t* subtract, unsigned int* n_nodes, hipStream_t st);
void launch_walk_gather(const DevBatch& src, const int32_t* rows, int count, const DevBatch& dst, hipStream_t st);
int walk_sort_keys64(void* temp, size_t* temp_bytes, const unsigned long long* key_in, unsigned long long* key, const uint32_t* val_in,
                     uint32_t* val, int count, hipStream_t st);
int walk_sort_keys32(void* temp, size_t* temp_bytes, const uint32_t* key_in, uint32_t* key, const uint32_t* val_in, uint32_t* val, int count,
                     hipStream_t st);
void launch_walk_records(int n, const uint8_t* flags, const unsigned long long* pre, const unsigned long long* post, unsigned long long* key,
                         uint32_t* val, hipStream_t st);
void launch_walk_record_sets(int n, const uint8_t* flags, const int32_t* set, const uint32_t* val, uint32_t* rec_set, uint32_t* pos,
                             hipStream_t st);
void launch_walk_permute(int n, const uint32_t* perm, const unsigned long long* key_in, const uint32_t* val_in, unsigned long long* key,
                         uint32_t* val, hipStream_t st);
void launch_walk_first(const level_walk::Level& L, uint32_t* first_pre, uint32_t* first_post, hipStream_t st);
void launch_walk_init(int n, uint8_t* state, uint8_t* ok, int32_t* counts, uint8_t* accepted, int32_t* wave, hipStream_t st);
void launch_walk_begin(int n, const uint8_t* flags, uint8_t* state, uint8_t* ok, int32_t* rows, int32_t* slot_of, unsigned int* ctl, hipStream_t st);
void launch_walk_round(const level_walk::Level& L, const WalkArrays& A, int w, unsigned int* ctl, hipStream_t st);
void launch_walk_finish(const level_walk::Level& L, const WalkArrays& A, int w, int budget, unsigned int* ctl, hipStream_t st);

// the split into subtrees (kernel_octree_partition.hip, include/hpmvs_amd.h: hpmvs_octree_partition).  launch_octree_partition
// reads the table launch_octree_build made and enqueues the leaf kernel, the sort, the one-wavefront loop and the assignment on
// st; != 0: the rocPRIM call failed.  info: the call's device record, zeroed by the caller -- the hpmvs_octree_partition_info the
// host reads.  root_keys / root_vals: the final roots as a table of their own (key -> list index; root_slots a power of two
// > 2 cap, keys zeroed by the caller).  Every output is nullable; what is given is written in every entry ([cap] the roots').
constexpr int kPartitionTrees = 0, kPartitionOrphans = 1, kPartitionSplits = 2, kPartitionStop = 3, kPartitionHistogram = 4,
              kPartitionInts = 4 + 22;
struct OctreePartitionRoots {
    unsigned long long* root_key; float* root_cell; int32_t* tree_first; int32_t* tree_leaves;
};
struct OctreePartitionKeys {
    int32_t* leaf_tree; unsigned long long* leaf_sub_key; int32_t* branch_tree; unsigned long long* branch_sub_key;
};
struct OctreePartitionScratch {
    int32_t* info;                       // [kPartitionInts]
    unsigned long long *key_a, *key_b;   // [n_leaves] each: the aligned keys, unsorted and sorted
    int32_t *val_a, *val_b;              // [n_leaves] each (val_b stands in for a leaf_order that is not asked for)
    unsigned long long* root_keys;       // [root_slots]
    int32_t* root_vals;                  // [root_slots]
    uint32_t root_slots;
    void* temp;                          // octree_partition_temp_bytes(n_leaves)
    size_t temp_bytes;
};
size_t octree_partition_temp_bytes(int nl);   // (size_t)-1: the size query failed
int launch_octree_partition(const float* root, const unsigned long long* keys, const int32_t* vals, uint32_t slots,
                            const unsigned long long* branch_key, int nb, const unsigned long long* leaf_key, int nl, int min_trees,
                            int min_split_leaves, int cap, const OctreePartitionScratch& s, const OctreePartitionRoots& roots,
                            int32_t* leaf_order, const OctreePartitionKeys& out, hipStream_t st);

// baseline JPEG behind the host's entropy decoder (kernel_jpeg.hip, jpeg.hpp, include/hpmvs_amd.h: hpmvs_jpeg_decode).  q: [3][64]
// quantiser steps in natural order (unused tables zero), coef: the components' [blocks_y][blocks_x][64] int16 one behind the
// other, 16-byte aligned; component c's blocks start at first<c> (first1 = first2 = n_blocks for grayscale).
struct JpegBlocks {
    uint32_t n_blocks, first1, first2;
    int32_t bx0, bx12;  // blocks per row: luma, chroma
};
void launch_jpeg_idct(const uint16_t* q, const int16_t* coef, const JpegBlocks& B, const jpg::Planes& P, uint8_t* planes, hipStream_t st);
// planes -> interleaved u8 RGB [H][W][3]: exactly W x H pixels are written
void launch_jpeg_rgb(const uint8_t* planes, const jpg::Planes& P, uint8_t* rgb, hipStream_t st);

// the scan's Huffman data decoded in parallel (kernel_jpeg_entropy.hip, jpeg.hpp: decode_subseq; include/hpmvs_amd.h:
// hpmvs_jpeg_decode_ex).  bytes: the prescan's unstuffed bytes (16 zero bytes behind), segs / sub_seg: its segments and every
// subsequence's segment, tabs: six jpg::Huff (per component DC, AC) and the 64 zigzag bytes.  Working arrays, one element per
// subsequence: entry, exit, cnt, incl; per workgroup of the sync kernel (kSubsPerGroup subsequences): grp_exit [2][n_groups];
// per 256 subsequences: grp [n_scan_groups].  flags: [0] a pass's slowest workgroup in rounds, [1] the round budget ran out,
// [2] the check refused the chain.
struct JpegEntropy {
    const uint8_t* bytes;
    const jpg::Segment* segs;
    const uint32_t* sub_seg;
    const uint32_t* tabs;
    jpg::ScanInfo si;
    uint32_t subseq_bits, n_subs, n_segs, n_groups, n_scan_groups;
    jpg::SubState *entry, *exit, *grp_exit;
    uint4 *cnt, *incl, *grp;
    uint32_t* flags;
};
// one synchronisation pass (pass 0 decodes from the guesses first); budget: rounds a workgroup may still take
void launch_jpeg_entropy_sync(const JpegEntropy& A, int pass, int budget, hipStream_t st);
// sums, check and write; coef: the zero-filled dense coefficients (JpegBlocks' layout), written only if the check accepts.
// ev (diagnostics, nullable): five events recorded in front of, between and behind the four kernels; -> the first event
// call's error, if any (launch errors: hipGetLastError, as for every launcher here)
hipError_t launch_jpeg_entropy_finish(const JpegEntropy& A, int16_t* coef, hipStream_t st, hipEvent_t* ev = nullptr);

// baseline JPEG encode of interleaved u8 RGB in HBM (kernel_jpeg_encode.hip, jpeg_enc.hpp, include/hpmvs_amd.h: hpmvs_jpeg_encode).
// coef: [n_blocks][64] int16 in zigzag order, MCU scan order (Y00 Y01 Y10 Y11 Cb Cr); tabs: device copy of make_tables'.
void launch_jpeg_enc_coef(const uint8_t* rgb, const jpge::Geom& g, const jpge::EncTables* tabs, int16_t* coef, hipStream_t st);
// lens: [n_blocks + 1] bits of every block's code; the caller zeroes the last entry
void launch_jpeg_enc_lengths(const int16_t* coef, uint32_t n_blocks, const jpge::EncTables* tabs, unsigned long long* lens, hipStream_t st);
// rocPRIM's exclusive sum over n 64-bit entries; temp == nullptr: only reports the temporary bytes it needs.  -> hipError_t
int jpeg_enc_scan(void* temp, size_t* temp_bytes, const unsigned long long* in, unsigned long long* out, size_t n, hipStream_t st);
// offs: the scan of lens; stream: zero-filled, ceil(offs[n_blocks] / 8) bytes rounded up to a multiple of 64
void launch_jpeg_enc_write(const int16_t* coef, uint32_t n_blocks, const jpge::EncTables* tabs, const unsigned long long* offs, uint32_t* stream,
                           hipStream_t st);
// cnt: [n_chunks + 1] 0xFF bytes per 64-byte chunk of the stream; the caller zeroes the last entry
void launch_jpeg_enc_ff(const uint8_t* stream, unsigned long long n_chunks, unsigned long long* cnt, hipStream_t st);
// moved: the scan of cnt; out: n_bytes + moved[n_chunks] bytes, the stream with a 0x00 behind every 0xFF
void launch_jpeg_enc_stuff(const uint8_t* stream, unsigned long long n_chunks, unsigned long long n_bytes, const unsigned long long* moved, uint8_t* out,
                           hipStream_t st);

// refined-patch records of the multi-GPU exchange (include/hpmvs_amd.h: hpmvs_record, 192 bytes)
void launch_pack_records(const DevBatch& b, void* records, hipStream_t st);
void launch_unpack_records(const void* records, int n, const DevBatch& b, hipStream_t st);
// ... and the tails of the lists longer than a record's 64 ids (scratch_counts: one int per 64 patches, total: one device int)
void launch_pack_record_tails(const DevBatch& b, void* tails, int cap, int32_t* scratch_counts, int32_t* total, hipStream_t st);
void launch_unpack_record_tails(const void* tails, int n_tails, int patch_offset, const DevBatch& b, hipStream_t st);
// diagnostics: the BOBYQA state machine on analytic objectives (kernel_selftest.hip); device pointers
void launch_selftest(int n, const int* kind, const double* params, const double* x0, const double* lb, const double* ub,
                     int maxeval, double* xfinal, double* minf, int* rc, int* nevals, int* rescues, double* trace,
                     int trace_cap, double* cold, hipStream_t st);
size_t selftest_cold_doubles(int n);  // doubles of the `cold` scratch (the optimiser states' cold arrays) for n problems

}  // namespace hpmvs
