// mo3d::PatchOptimizer -- the drop-in boundary.  Same class name, namespace, constructor and
// optimize() as the reference (include/hpmvs/PatchOptimizer.h:39-43); copyable and cheap to
// construct (the reference holds one per thread in a std::vector: src/hpmvs/Scene.cpp:94-96,
// src/main.cpp:123-125).  optimize() is a batch of one through the C ABI; optimizeBatch() is the
// additive entry for callers that can hand over many independent patches at once (the seed loop of
// Scene::initPatches, Scene.cpp:114-167).
#ifndef HPMVS_PATCHOPTIMIZER_H
#define HPMVS_PATCHOPTIMIZER_H
#include <cstddef>
#include <cstdint>
#include <unordered_set>
#include <vector>
#include <hpmvs/Patch3d.h>
namespace mo3d {
class HpmvsOptions;
class Scene;
struct OctreeIndex;
struct OctreeForest;
struct BorderForestInsertion;
class PatchOptimizer {
public:
    PatchOptimizer(const mo3d::HpmvsOptions& options, const mo3d::Scene* scene);
    // false = drop this patch (patch untouched), exactly the reference's convention; infrastructure
    // errors (HIP failure, no device) also return false after logging to stderr.
    bool optimize(mo3d::Patch3d& patch);
    // ok[i] = result of optimize(*patches[i]); returns the number of successes
    size_t optimizeBatch(mo3d::Patch3d* const* patches, size_t n, uint8_t* ok);
    // Frontier expansion: the candidate loops of CellProcessor::extend (mode EXTEND, 6 candidates per
    // parent, reference src/hpmvs/CellProcessor.cpp:84-142) and CellProcessor::branch (mode BRANCH, 4
    // candidates, :210-262) for many cells in one GPU call: candidates are constructed exactly as the
    // reference does (*newP = *p, new centre/scale, expanded_ = false, flatness_ = -1), optimized, and
    // the geometric gates applied.  cells[i] = (leaf centre, leaf width) of parents[i]; skip (optional,
    // n*N flags) marks candidates whose target leaf the caller already found occupied (:120-124).
    // candidates receives n*N patches (candidate k of parent i at i*N + k), accepted[i*N + k] != 0 where
    // the candidate passed; the depth tests and the octree insertion stay with the caller.  Returns N.
    enum ExpandMode { EXTEND = 0, BRANCH = 1 };
    struct CellRef { Eigen::Vector3f c; float width; };
    int expandBatch(ExpandMode mode, const mo3d::Patch3d* const* parents, const CellRef* cells, size_t n,
                    const uint8_t* skip, std::vector<mo3d::Patch3d>& candidates, std::vector<uint8_t>& accepted);
    // One priority level of CellProcessor::extend (reference src/hpmvs/CellProcessor.cpp:84-178; main.cpp:146-181 pops the leaves of
    // one priority and runs it on each, one after the other) as a BATCHED frontier with the reference's SEQUENTIAL result: ONE
    // expandBatch for the level, then conflict-free waves of depthGates / walk in the reference's order / setDepths (a candidate is
    // decided unless a map cell it reads or would write, or its leaf, still depends on an undecided earlier candidate -- then it
    // waits for the next wave; hpmvs_amd/frontier.py is the same walk in Python, INTEGRATION.md has the argument).  The walk exists once
    // in the host layer, over a queue of candidates and subtraction events: this is its case without events, filterExtendLevel the one
    // with.  The pyramid levels a read can be on are the scene's cameras' (false beyond HPMVS_MAX_LEVELS).  parents: the
    // leaves' patches in the scheduler's order; width: the leaves' width; `occupied`: the scheduler's occupancy as a set of leaf
    // keys, updated in place (the octree itself stays with the scheduler: `leafKey` maps a point to its leaf, default = the
    // uniform grid floor(p / width)); the scene's depth maps (Scene::resetDepths / setDepths) receive the accepted candidates.
    // stage: 0 accepted and inserted, 20 leaf already taken (no refinement), 1 refinement or the scale / drift gates failed,
    // 23 / 24 / 25 depthTests / viewBlockTest / pixelFreeTests, 26 addConditional found the refined patch's leaf taken.
    struct LevelResult {
        std::vector<mo3d::Patch3d> candidates;   // 6 per parent
        std::vector<int> stage;
        std::vector<int> counts;                 // 3 per candidate: the counts at decision time (-1: not reached)
        std::vector<size_t> accepted;            // candidate indices, the reference's order
        int waves = 0;
        std::vector<size_t> border;              // extendLevelTree: the stage-27 candidates in queue order (the scheduler routes them)
        std::vector<uint64_t> leafKey;           // extendLevelTree: per entry of `accepted` the path key of the leaf it went into
        std::vector<int32_t> tree;               // extendLevelForest: per candidate its tree (empty for the other levels)
    };
    typedef uint64_t (*LeafKeyFn)(const Eigen::Vector3f& p, float width, void* user);
    bool extendLevel(const mo3d::Patch3d* const* parents, size_t n, float width, std::unordered_set<uint64_t>& occupied,
                     float margin, bool absInt, LevelResult& out, bool sequential = true, LeafKeyFn leafKey = nullptr, void* user = nullptr);
    // extendLevel against the scheduler's REAL octree, or a subtree of it (hpmvs_amd.frontier.extend_level_tree: same calls, same
    // results): `parents` are the leaves of ONE node level, all of width `width` -- an exact level width of the tree
    // (tree.levelDepth(width) >= 1, false otherwise).  The walk is extendLevel's; the candidates, their refinement and the keys of
    // both look-ups (CellProcessor.cpp:122-125, 147-154) come from ONE hpmvs_extend_tree_batch.  Stage codes as extendLevel's,
    // where 20 is the pre-gate (inside the root, in a nonempty leaf of any depth or in structure finer than `width`), 26
    // addConditional's refusal, and 27 = BORDER: the candidate passed every gate but left the tree's root.  Border candidates
    // come back in LevelResult::border for the scheduler to route (Scene::octreeRoute / octreeInsert); they are not inserted and
    // write no depths.  The accepted candidates are entered into `tree` (OctreeIndex::insertLeaf at LevelResult::leafKey).
    bool extendLevelTree(const mo3d::Patch3d* const* parents, size_t n, float width, mo3d::OctreeIndex& tree, float margin, bool absInt,
                         LevelResult& out, bool sequential = true);
    // extendLevelTree for ALL subtrees of a partition in one pass (hpmvs_amd.frontier.extend_level_forest: same calls, same results;
    // DESIGN.md §3.15): `parents` are the trees' level queues one after the other -- parentTree[i] names the tree of parent i and must
    // not decrease (false otherwise, as for a tree with a parent of which `width` is no level width; a tree without parents may be
    // rooted anywhere).  The candidates of every tree come from ONE hpmvs_extend_forest_batch and go through the ONE walk, whose
    // result over the concatenated queue is the sequential loop's: extendLevelTree on tree 0, then tree 1, and so on, from the same
    // maps.  LevelResult::tree names every candidate's tree, leafKey is the key in that tree, where the accepted candidate is
    // entered.  Border candidates (27: outside their OWN tree's root) are delivered by the scheduler between levels, never between
    // the subtrees of one level.
    bool extendLevelForest(const mo3d::Patch3d* const* parents, const int32_t* parentTree, size_t n, float width, mo3d::OctreeForest& forest,
                           float margin, bool absInt, LevelResult& out, bool sequential = true);
    // One priority level of CellProcessor::branch (reference src/hpmvs/CellProcessor.cpp:210-307) over the patches of the level's
    // leaves, in the scheduler's order: level-support gate (:221-224), the four diagonal children with Cell::contains before and
    // after optimize (:233-258) as ONE expandBatch, then the depth maps in the reference's order -- per split leaf its patch taken
    // back (:276-279), its children entered (:296) -- as ONE ordered Scene::setDepths call.  finalLevel[i]: nodeLevel(leaf i) >=
    // PATCH_FINAL_MINLEVEL (the scheduler's knowledge): such a leaf keeps its patch when no child survived (:265-266).  The tree
    // operations (split, the children's leaves, the queue) stay with the caller; the result says what to do with every leaf.
    struct BranchResult {
        std::vector<mo3d::Patch3d> candidates;   // 4 per leaf
        std::vector<uint8_t> child;              // 4 per leaf: goes into the new leaves
        std::vector<int> support;                // Scene::getLevelSupport of the leaf's patch
        std::vector<uint8_t> split;              // per leaf: split (its patch's depths are out of the maps, the children's in)
    };
    bool branchLevel(const mo3d::Patch3d* const* parents, const CellRef* cells, size_t n, const uint8_t* finalLevel, BranchResult& out);
    // Priorities L*10+1 / +2 of CellProcessor::processCell (reference src/hpmvs/CellProcessor.cpp:369-420) as batched device calls, the
    // C++ form of hpmvs_amd.frontier.regularize_level / settle_level / process_level (same calls, same results).  The octree stays the
    // scheduler's: it passes a versioned snapshot of its nonempty leaves (include/hpmvs_amd.h, hpmvs_leaf_table): leaf j exists at queue
    // positions born[j] < q < died[j].
    struct LeafTable {
        Eigen::Vector3f rootCenter;          // Cell::c_ of the Branch the CellProcessor walks (a subtree's root when the model is split)
        float rootWidth = 0.0f;
        std::vector<float> center, width, patch;   // 3 / 1 / 3 floats per leaf: Leaf::c_, width_, data[0]->center_
        std::vector<int32_t> born, died;           // 1 per leaf (-1 / INT32_MAX: present for the whole sweep)
        size_t size() const { return width.size(); }
    };
    // CellProcessor::regularize (:309-367) for cells[i] at queue position position[i] against `table`: writes flatness_ (an unexpanded
    // cell keeps it) and sets priorityReduction_ = 0 (:399).  cellWidth[i]: its leaf's width_.  nNeighbours (optional): the distinct
    // nonempty leaves found, -1 for an unexpanded cell.
    bool regularizeLevel(mo3d::Patch3d* const* cells, size_t n, const float* cellWidth, const int32_t* position, const LeafTable& table,
                         std::vector<int>* nNeighbours = nullptr);
    // processCell's decision for expanded leaves with flatness_ >= 0 (:409-419), in the scheduler's order: flatness_ > 2.4 removes the
    // patch (its depths taken back), anything else branches the leaf (branchLevel's rule).  Removals and branches share ONE ordered
    // Scene::setDepths call.  childOctant[4 i + k]: the octant (Branch::at's index) of leaf i that child k goes into, -1 if none.
    struct SettleResult {
        std::vector<mo3d::Patch3d> candidates;   // 4 per leaf
        std::vector<uint8_t> child;              // 4 per leaf
        std::vector<int> childOctant;            // 4 per leaf
        std::vector<int> support;
        std::vector<uint8_t> removed, split;
    };
    bool settleLevel(const mo3d::Patch3d* const* parents, const CellRef* cells, size_t n, const uint8_t* finalLevel, SettleResult& out);
    // One sweep of mixed cells in queue order (position = index): settleLevel on the cells with flatness_ >= 0, their removals and splits
    // as died / born entries of the table, then regularizeLevel on the cells with flatness_ < 0 against it.  Every cell must be expanded
    // and own its leaf (cellLeaf[i]: index into `table`, distinct).  out.table: the sweep's versioned table (split children appended).
    struct ProcessResult {
        std::vector<size_t> settled;             // the cells settleLevel decided, in order
        SettleResult settle;                     // row j for cell settled[j]
        LeafTable table;
        std::vector<int> childLeaf;              // 4 per settled cell: the table index of the child's leaf (-1: none)
        std::vector<int> nNeighbours;            // per cell; -2 for settled cells
    };
    bool processLevel(mo3d::Patch3d* const* cells, const int32_t* cellLeaf, size_t n, const uint8_t* finalLevel, const LeafTable& table,
                      ProcessResult& out);
    // processLevel for ALL subtrees of a partition as ONE hpmvs_process_forest_batch (hpmvs_amd.frontier.process_level_forest: same
    // call, same results): cells[i] is data[0] of the nonempty leaf cellKey[i] of forest.trees[cellTree[i]], the
    // trees' queues one after the other (cellTree must not decrease, false otherwise).  The tree travels as its key sets -- no
    // leaf table, no cell centres; patchCenter holds data[0]->center_ of every nonempty leaf, 3 floats each, in the order
    // OctreeForest::flatten lists the leaves.  Thin marshalling: the sweep's decisions, regularize against the tree as it stands
    // at every cell's turn and the ordered depth-map replay all happen in the one device call.  Written back: flatness_ and
    // priorityReduction_ = 0 of the regularized cells (CellProcessor.cpp:399); images_ cleared for removed patches (:411) and for
    // the old patch of a split leaf (:279-280).  The forest is NOT changed: OctreeIndex::applySweep applies a tree's share.
    struct ForestProcessResult {
        std::vector<mo3d::Patch3d> candidates;   // 4 per cell (those of a regularized, removed or exhausted cell are not built)
        std::vector<int> support;                // per cell
        std::vector<uint8_t> removed, split;     // per cell
        std::vector<uint8_t> child;              // 4 per cell
        std::vector<uint64_t> childKey;          // 4 per cell: the key in the cell's tree of the leaf the child goes into, 0: none
        std::vector<int> nNeighbours;            // per cell; -2 for settled cells
    };
    bool processLevelForest(mo3d::Patch3d* const* cells, const int32_t* cellTree, const uint64_t* cellKey, size_t n, const uint8_t* finalLevel,
                            const mo3d::OctreeForest& forest, const std::vector<float>& patchCenter, ForestProcessResult& out);
    // A round's border queue delivered to ALL subtrees as ONE hpmvs_border_forest_batch (hpmvs_amd.frontier.deliver_border_forest:
    // same call, same results; reference CellProcessor.cpp:487-540): Scene::octreeBorderForest with setDepths, then
    // for the accepted patches, in queue order, flatness_ = 0 (:514: no regularization on border cells) and
    // OctreeIndex::insertLeaf of their key into their own tree.  The scheduler's queue and its priorities stay the caller's.
    bool deliverBorderForest(mo3d::Patch3d* const* border, size_t n, mo3d::OctreeForest& forest, mo3d::BorderForestInsertion& out);
    // Priority L*10 of processCell for cells holding several patches (reference src/hpmvs/CellProcessor.cpp:369-392, filter :43-82), the
    // C++ form of hpmvs_amd.frontier.filter_level / filter_extend_level (same calls, same results).  patches: the cells' patches in data
    // order, the cells in the scheduler's order; cell c holds patches[cellStart[c]] .. patches[cellStart[c + 1] - 1] (cellStart has
    // nCells + 1 entries, starts at 0 and does not decrease).  keep[c]: the index of the patch filter keeps (-1: empty cell); removed[i]:
    // patch i lost (its depths are out of the maps and its images_ cleared, as the reference does; the tree stays the caller's).
    struct FilterResult {
        std::vector<int> keep;
        std::vector<float> dist;                 // per patch: the reference's mean signed plane distance (0 in single-patch cells)
        std::vector<uint8_t> removed;
    };
    // filter for every cell as ONE hpmvs_filter_batch, then the losers' depths taken back in ONE ordered Scene::setDepths(..., subtract).
    // false (nothing changed) for malformed offsets or a cell with no winner (the reference would keep a null pointer).
    bool filterLevel(mo3d::Patch3d* const* patches, const size_t* cellStart, size_t nCells, FilterResult& out);
    // filter cell i, then CellProcessor::extend on its kept patch, for every cell in queue order: ONE filter call, then the walk of
    // extendLevel over the kept patches with the losers in its queue and its conflict graph as subtraction events, each right before its
    // cell's candidates.  `level` is laid out as extendLevel's, the kept patches being the parents.  false before any map update for
    // malformed offsets, an empty cell, a cell with no winner or a kept patch that is already expanded (processCell does not extend it).
    bool filterExtendLevel(mo3d::Patch3d* const* patches, const size_t* cellStart, size_t nCells, float width,
                           std::unordered_set<uint64_t>& occupied, float margin, bool absInt, FilterResult& filter, LevelResult& level,
                           LeafKeyFn leafKey = nullptr, void* user = nullptr);
    // filterExtendLevel against the real octree: the same walk with extendLevelTree's keys, the filters' losers as events.
    bool filterExtendLevelTree(mo3d::Patch3d* const* patches, const size_t* cellStart, size_t nCells, float width, mo3d::OctreeIndex& tree,
                               float margin, bool absInt, FilterResult& filter, LevelResult& level);
    // filterExtendLevelTree for all subtrees in one pass: cell c is a leaf of forest.trees[cellTree[c]], cellTree non-decreasing.
    bool filterExtendLevelForest(mo3d::Patch3d* const* patches, const size_t* cellStart, const int32_t* cellTree, size_t nCells, float width,
                                 mo3d::OctreeForest& forest, float margin, bool absInt, FilterResult& filter, LevelResult& level);
    // The candidate steps of such a level alone, as ONE hpmvs_extend_tree_batch (include/hpmvs_amd.h; the C++ form of
    // hpmvs_amd.api.extend_tree_batch): expandBatch(EXTEND) with cells = (0, width) and the skip flags decided on the device by
    // the tree, plus the keys of both look-ups, 6 n entries each.  preKey means something only where preInside is set: a centre
    // outside the root matches no leaf.  Returns 6; on failure `accepted` is all zero and `candidates` empty.
    struct TreeKeys {
        std::vector<uint8_t> skip, preInside, border;
        std::vector<uint64_t> preKey, postKey;
    };
    int expandTreeBatch(const mo3d::Patch3d* const* parents, size_t n, float width, const mo3d::OctreeIndex& tree,
                        std::vector<mo3d::Patch3d>& candidates, std::vector<uint8_t>& accepted, TreeKeys& keys);
    // The same for a forest, as ONE hpmvs_extend_forest_batch: parentTree[i] names the tree of parent i, in any order; the keys
    // are relative to the candidate's own tree.
    int expandForestBatch(const mo3d::Patch3d* const* parents, const int32_t* parentTree, size_t n, float width, const mo3d::OctreeForest& forest,
                          std::vector<mo3d::Patch3d>& candidates, std::vector<uint8_t>& accepted, TreeKeys& keys);
    // diagnostics of the last optimize()/optimizeBatch() call that the reference computes and drops
    // (final mean robust INCC f*, PatchOptimizer.cpp:365,376): one entry per patch
    const std::vector<double>& lastObjective() const { return lastF_; }
    const std::vector<int>& lastEvaluations() const { return lastEvals_; }
    // The batch entries keep their structure-of-arrays copies in pinned host memory that the GPU uses in place, reused from
    // call to call through a per-thread cache.  Bytes the CALLING thread holds for reuse right now, and the cap beyond which
    // returned blocks go back to the system (default 512 MB, $HPMVS_PIN_CACHE_MB; setPinnedCacheCap changes it for the
    // calling thread and trims at once).
    static size_t pinnedCacheBytes();
    static size_t pinnedCacheCap();
    static void setPinnedCacheCap(size_t bytes);
private:
    // expandBatch's body for both device entries: hpmvs_expand_batch (tree == nullptr), or hpmvs_extend_tree_batch at `width`
    // against `tree` (mode EXTEND; cells and skip unused, keys filled), or hpmvs_extend_forest_batch against `forest` with parentTree
    int expandCall(ExpandMode mode, const mo3d::Patch3d* const* parents, const CellRef* cells, size_t n, const uint8_t* skip,
                   const mo3d::OctreeIndex* tree, float width, TreeKeys* keys, std::vector<mo3d::Patch3d>& candidates,
                   std::vector<uint8_t>& accepted, const mo3d::OctreeForest* forest = nullptr, const int32_t* parentTree = nullptr);
    const mo3d::HpmvsOptions* options_p;
    const mo3d::Scene* scene_p;
    std::vector<double> lastF_;
    std::vector<int> lastEvals_;
    int preferFullRows_ = 0;   // small calls that go straight to rows as wide as a list can get (a dense scene: optimizeBatch)
};
}  // namespace mo3d
#endif
