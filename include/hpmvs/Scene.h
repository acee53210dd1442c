// mo3d::Scene -- the part of the reference's Scene the refinement path reads (reference
// include/hpmvs/Scene.h:69-71: cameras_, images_, covis_; cached by PatchOptimizer at
// src/hpmvs/PatchOptimizer.cpp:38-41).  The octree object and the scheduler stay with the host application (seedTree builds
// the initial tree's leaf tables); the
// depth maps (reference Scene.h:74-76) live in HBM next to the pyramids, with batch forms of setDepths and of the
// three acceptance tests the expansion gates its candidates on.  The scene must be complete before the first PatchOptimizer is constructed and is
// immutable afterwards, exactly as in the reference; at that point it is uploaded to HBM once and
// shared by every optimizer instance.
#ifndef HPMVS_SCENE_H_
#define HPMVS_SCENE_H_
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include <hpmvs/Camera.h>
#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/Image.h>
#include <hpmvs/NVMReader.h>
#include <hpmvs/Patch3d.h>
struct hpmvs_scene;
namespace mo3d {
// A DynOctTree as path keys (include/hpmvs_amd.h: hpmvs_octree_index): the root cell, every Branch below it, the nonempty leaves.
struct OctreeIndex {
    float rootCenter[3];
    float rootWidth;
    std::vector<uint64_t> branchKeys;
    std::vector<uint64_t> leafKeys;
    // Enter a patch into the EMPTY leaf `key` (what addConditional's splits leave behind): the key is appended to leafKeys and
    // every proper prefix below the root that is not a branch yet to branchKeys, deepest first.  Append only: the vectors keep
    // their order.  PatchOptimizer::extendLevelTree enters a level's accepted candidates with it.
    void insertLeaf(uint64_t key) {
        if (branchSet_.size() != branchKeys.size()) branchSet_ = std::unordered_set<uint64_t>(branchKeys.begin(), branchKeys.end());
        leafKeys.push_back(key);
        for (uint64_t k = key >> 3; k > 1; k >>= 3)
            if (branchSet_.insert(k).second) branchKeys.push_back(k);
    }
    // The depth d >= 1 whose cells have width_ == width (rootWidth halved d times, each time in double and narrowed to float, as
    // Cell(parent, idx) does; at most 21 levels), -1 when there is none: the widths extendLevelTree takes.
    int levelDepth(float width) const {
        float w = rootWidth;
        int d = 0;
        while (w > width && d < 21) { w = (float)((double)w / 2.0); d++; }
        return (w == width && d >= 1) ? d : -1;
    }
    // One regularize / settle sweep's removals and splits of THIS tree (PatchOptimizer::processLevelForest, whose arrays these
    // are, restricted to the cells of this tree and in queue order), with the meaning of DynOctTree::remove / Leaf::split:
    //   removed[i]   the leaf cellKey[i] is emptied; when its parent Branch is then empty all through, the parent becomes ONE
    //                empty leaf (remove_internal collapses one level only, doctree.h:422-450; the root stays a Branch)
    //   split[i]     the leaf becomes a Branch; child k (child[4 i + k]) goes into the leaf childKey[4 i + k], the FIRST child
    //                of a leaf being its data[0]
    // The vectors keep the order of what survives; new branches and leaves are appended in the order they were made.
    // leafFrom (optional): per entry of the new leafKeys its index in the old ones, or -(1 + 4 i + k) for a leaf born from
    // child k of cell i -- what the caller needs to carry its per-leaf data (data[0]->center_) over.  One pass over the keys
    // and the cells, whatever the number of removals.  False, and nothing changed, when a removed or split cell's key is no
    // nonempty leaf of the tree.
    bool applySweep(const uint64_t* cellKey, const uint8_t* removed, const uint8_t* split, const uint8_t* child, const uint64_t* childKey,
                    size_t n, std::vector<int32_t>* leafFrom = nullptr) {
        std::unordered_set<uint64_t> B(branchKeys.begin(), branchKeys.end()), L(leafKeys.begin(), leafKeys.end());
        for (size_t i = 0; i < n; i++)
            if ((removed[i] || split[i]) && !L.count(cellKey[i])) return false;
        std::unordered_map<uint64_t, int32_t> below;   // Branch -> nonempty leaves below it
        for (uint64_t key : leafKeys)
            for (uint64_t k = key >> 3; k > 1; k >>= 3) below[k]++;
        std::vector<uint64_t> newBranches, newLeaves, stack;
        std::vector<int32_t> newFrom;
        for (size_t i = 0; i < n; i++) {
            const uint64_t key = cellKey[i];
            if (!removed[i] && !split[i]) continue;
            L.erase(key);
            for (uint64_t k = key >> 3; k > 1; k >>= 3) below[k]--;
            if (removed[i]) {
                const uint64_t par = key >> 3;
                if (par == 1 || below[par] != 0) continue;
                stack.assign(1, par);   // the parent and every Branch below it go: one empty leaf is left
                while (!stack.empty()) {
                    const uint64_t b = stack.back();
                    stack.pop_back();
                    B.erase(b);
                    below.erase(b);
                    for (uint64_t c = 0; c < 8; c++)
                        if (B.count((b << 3) | c)) stack.push_back((b << 3) | c);
                }
                continue;
            }
            if (B.insert(key).second) newBranches.push_back(key);
            for (int k = 0; k < 4; k++) {
                const uint64_t ck = childKey[4 * i + k];
                if (!child[4 * i + k] || !L.insert(ck).second) continue;
                for (uint64_t a = ck >> 3; a > 1; a >>= 3) below[a]++;
                newLeaves.push_back(ck);
                newFrom.push_back(-(int32_t)(1 + 4 * i + k));
            }
        }
        std::vector<uint64_t> bk, lk;
        for (uint64_t k : branchKeys) if (B.count(k)) bk.push_back(k);
        for (uint64_t k : newBranches) if (B.count(k)) bk.push_back(k);
        if (leafFrom) leafFrom->clear();
        for (size_t j = 0; j < leafKeys.size(); j++)
            if (L.count(leafKeys[j])) { lk.push_back(leafKeys[j]); if (leafFrom) leafFrom->push_back((int32_t)j); }
        lk.insert(lk.end(), newLeaves.begin(), newLeaves.end());
        if (leafFrom) leafFrom->insert(leafFrom->end(), newFrom.begin(), newFrom.end());
        branchKeys.swap(bk);
        leafKeys.swap(lk);
        branchSet_.swap(B);
        return true;
    }
    std::unordered_set<uint64_t> branchSet_;   // insertLeaf's view of branchKeys; rebuilt when branchKeys was changed by hand
};
// The subtrees of one partition as the forest calls take them (include/hpmvs_amd.h: hpmvs_octree_forest): every tree's keys are
// relative to its own root.  PatchOptimizer::extendLevelForest / filterExtendLevelForest run a level over all of them at once.
struct OctreeForest {
    std::vector<OctreeIndex> trees;
    // The C structure's arrays: the roots, the offsets and the keys one tree after the other.  `flat` keeps them alive.
    struct Flat {
        std::vector<float> root;                     // [n_trees][4] c_, width_
        std::vector<int32_t> branchFirst, leafFirst; // [n_trees + 1]
        std::vector<uint64_t> branchKey, leafKey;
    };
    void flatten(Flat& flat) const {
        flat = Flat();
        flat.branchFirst.push_back(0);
        flat.leafFirst.push_back(0);
        for (const OctreeIndex& t : trees) {
            flat.root.insert(flat.root.end(), t.rootCenter, t.rootCenter + 3);
            flat.root.push_back(t.rootWidth);
            flat.branchKey.insert(flat.branchKey.end(), t.branchKeys.begin(), t.branchKeys.end());
            flat.leafKey.insert(flat.leafKey.end(), t.leafKeys.begin(), t.leafKeys.end());
            flat.branchFirst.push_back((int32_t)flat.branchKey.size());
            flat.leafFirst.push_back((int32_t)flat.leafKey.size());
        }
    }
};
// What hpmvs_border_forest_batch returns for a round's border queue (Scene::octreeBorderForest, PatchOptimizer::deliverBorderForest).
struct BorderForestInsertion {
    std::vector<int32_t> tree;         // [n] -1: no root contains the patch (it is dropped)
    std::vector<uint8_t> accepted;     // [n]
    std::vector<uint64_t> leafKey;     // [n] in the row's own tree
    std::vector<int32_t> blocker;      // [n] an index into the queue
};
// The split of a DynOctTree into subtrees (include/hpmvs_amd.h: hpmvs_octree_partition); the roots' vectors hold nTrees entries.
struct OctreePartition {
    int nTrees, nOrphans, nSplits, stop;   // stop 0: the root alone; 1: the list reached minTrees; 2: the largest subtree is too small
    std::vector<int32_t> histogram;        // [22] cellHistogram: nonempty leaves by depth below the root
    std::vector<uint64_t> rootKey;         // the subtree roots in the reference's list order
    std::vector<float> rootCell;           // [nTrees][4] c_, width_
    std::vector<int32_t> treeFirst, treeLeaves;   // subtree k's leaves: leafOrder[treeFirst[k] .. treeFirst[k] + treeLeaves[k] - 1]
    std::vector<int32_t> leafOrder;        // [leaves] indices into OctreeIndex::leafKeys in Leaf_iterator order
    std::vector<int32_t> leafTree;         // [leaves] -1: an orphan
    std::vector<uint64_t> leafSubKey;      // [leaves] the key re-based on the subtree's root, 0 for an orphan
    std::vector<int32_t> branchTree;       // [branches] -1: a root or a branch above the roots
    std::vector<uint64_t> branchSubKey;    // [branches]
};

class Scene {
public:
    Scene();
    virtual ~Scene();
    // Scene::addCameras (src/hpmvs/Scene.cpp:42-88) minus the depth maps: Image::load + Camera::init
    bool addCameras(const NVM_Model& model, const HpmvsOptions& options);
    // Scene::extractCoVisiblilty (src/hpmvs/Scene.cpp:241-298), including its positional-index quirk
    bool extractCoVisiblilty(const NVM_Model& model, const HpmvsOptions& options);
    // The seed loop of Scene::initPatches (src/hpmvs/Scene.cpp:112-178) as ONE batched GPU call: seed
    // construction, optimize(), drift gate.  Survivors are appended to `out` in point order; inserting
    // them into the octree / depth maps (Scene.cpp:183-199) is seedTree below.
    // With options.FILTER_SCENE_CENTER (--only_sphere) the points outside getSceneCenter's sphere are skipped first, on the
    // device, as Scene.cpp:105-121 does; without a valid centre nothing is gated.
    bool initPatches(const NVM_Model& model, const HpmvsOptions& options, std::vector<Ppatch3d>& out) const;
    // The same loop behind a sphere of the caller's own (a region of interest): points with |xyz - center| > radius are
    // skipped first, whatever FILTER_SCENE_CENTER says.  stage: the per-point stage codes of hpmvs_init_patches_sphere_batch
    // (include/hpmvs_amd.h; 13 = outside the sphere), one per model point.
    bool initPatches(const NVM_Model& model, const HpmvsOptions& options, std::vector<Ppatch3d>& out,
                     const Eigen::Vector3d& center, double radius, std::vector<int>* stage = nullptr) const;
    // Scene::getSceneCenter (src/hpmvs/Scene.cpp:210-239) over hpmvs_scene_center: the point closest to every camera's optical
    // axis and the largest distance from it to a camera centre.  False without a valid centre (no camera; also one camera or
    // parallel axes, where the reference aborts or returns its QR's leftovers).  Host code, float64; equal to the reference's
    // to solver accuracy, not bit for bit (include/hpmvs_amd.h).
    bool getSceneCenter(Eigen::Vector3d& center, double& radius) const;
    // The second half of Scene::initPatches (src/hpmvs/Scene.cpp:183-199) as ONE batched GPU call (hpmvs_seed_tree_batch):
    // getBoundingBox, the root Branch, scale_3dx_ = max(scale_3dx_, width / (1 << PATCH_INIT_MAXLEVEL + 1)) written to every
    // patch, the octree the sequential patchTree_.add loop builds -- as the leaf tables the level calls read, not as pointers --
    // and, with setDepths, Scene::setDepths(p, false) of every patch (resetDepths first).  Insertion order is the vector's.
    // The octree object itself stays with the host application, which can build any pointer form it needs from the tables.
    struct SeedTree {
        float rootCenter[3], rootWidth, scaleFloor;
        std::vector<int32_t> rows;         // patch indices leaf by leaf (Leaf_iterator order), data order within a leaf
        std::vector<int32_t> cellStart;    // [leaves + 1] leaf l holds rows[cellStart[l] .. cellStart[l + 1] - 1]
        std::vector<float> cellCenter;     // [leaves][3] Leaf::c_
        std::vector<float> cellWidth;      // [leaves]
        std::vector<int32_t> cellLevel;    // [leaves] nodeLevel
        std::vector<float> patchCenter;    // [leaves][3] data[0]->center_
        size_t leaves() const { return cellWidth.size(); }
    };
    bool seedTree(std::vector<Ppatch3d>& patches, const HpmvsOptions& options, SeedTree& out, bool setDepths = true) const;
    // ---- depth maps (src/hpmvs/Scene.cpp:74-80) and the acceptance tests over them, batched on the device.
    // resetDepths: allocate / clear (MAX_DEPTH = 1000).  setDepths: Scene::setDepths(patch) (Scene.cpp:351-381) for
    // every patch.  depthGates: per patch the counts of Scene::depthTests, viewBlockTest and pixelFreeTests
    // (Scene.cpp:518-644) that CellProcessor compares with MIN_IMAGES_PER_PATCH (CellProcessor.cpp:134-142);
    // absInt selects C's abs(int) for the unqualified abs() at Scene.cpp:571 (default: the <cmath> overload).
    bool resetDepths() const;
    bool setDepths(const Patch3d* const* patches, size_t n) const;
    // Scene::setDepths(patch, subtract) for a list of calls IN ORDER (src/hpmvs/Scene.cpp:351-381): subtract[i] != 0 takes patch i's
    // depths back (a cell that still holds exactly its depth becomes MAX_DEPTH again, :373-374 -- CellProcessor::branch does that
    // for the patch of a leaf it splits, CellProcessor.cpp:276-279).  That does not commute with the minimum of an ordinary call,
    // so the list is applied cell by cell in call order on the device: the maps are those of the sequential loop.
    bool setDepths(const Patch3d* const* patches, size_t n, const uint8_t* subtract) const;
    // Scene::getLevelSupport(patch, minLevel) (src/hpmvs/Scene.cpp:334-343) for every patch
    bool levelSupport(const Patch3d* const* patches, size_t n, int minLevel, std::vector<int>& support) const;
    bool depthGates(const Patch3d* const* patches, size_t n, float margin, std::vector<int>& nVisible,
                    std::vector<int>& nBlocking, std::vector<int>& nFree, bool absInt = false) const;
    // The map cells those tests READ and the cells setDepths would WRITE, per patch, as packed keys -- what a scheduler needs to
    // run one priority level in conflict-free waves and still end with the reference's sequential result
    // (PatchOptimizer::extendLevel).  reads[i]: every cell depthTests / viewBlockTest reach through getFullDepth (3x3 level-0
    // pixels, every pyramid level) and pixelFreeTests' cell; writes[i]: the cell per attached image.  nLevels: pyramid levels.
    bool depthFootprints(const Patch3d* const* patches, size_t n, std::vector<std::vector<uint64_t> >& reads,
                         std::vector<std::vector<uint64_t> >& writes, int nLevels = 6) const;
    // The conflict graph of one level over those cells, made on the device (ONE hpmvs_level_conflicts_batch: no footprint reaches
    // the host): `patches` are the level's nodes in queue order, isEvent[i] != 0 marks a subtraction event (writes, no reads;
    // nullptr: all candidates).  flow[i]: the nodes j < i that write a cell i reads (an event i: the candidates that write a cell
    // it writes); anti[i]: the candidates j < i that read a cell i writes, and for a candidate i the events j < i that write one.
    // CSR, every list ascending without duplicates; the pyramid levels are the scene's cameras'.
    struct LevelGraph {
        std::vector<uint32_t> flowOff, flowAdj, antiOff, antiAdj;
    };
    bool levelConflicts(const Patch3d* const* patches, size_t n, const uint8_t* isEvent, LevelGraph& graph) const;
    // The wave walk of one extend level as ONE batched GPU call (hpmvs_level_walk_batch, include/hpmvs_amd.h):
    // items are the level's queue in the reference's order (an event's patch, a candidate's patch), flags the HPMVS_WALK_* bits,
    // set (nullptr: one set) the tree each candidate's keys belong to, preKey / postKey its leaf before and after refinement.
    // out.stage must hold the n preset stages.  Returns 0, 1 when the device refuses the level (HPMVS_ERR_STATE: no map was
    // written, walk on the host), -1 for any other failure (reported).  PatchOptimizer's levels use it with HPMVS_DEVICE_WALK=1.
    struct LevelWalk {
        std::vector<int32_t> stage, counts, wave;   // [n] in / out, [n][3], [n] the 1-based wave that decided the item
        std::vector<uint8_t> accepted;              // [n]
        int waves = 0;
    };
    int levelWalk(const Patch3d* const* items, size_t n, const HpmvsOptions& options, const uint8_t* flags, const int32_t* set,
                  const uint64_t* preKey, const uint64_t* postKey, float margin, bool absInt, LevelWalk& out) const;
    // The scheduler's octree as CellProcessor::extend consults it (CellProcessor.cpp:122-125, 147-154), for a list of points as
    // ONE batched GPU call (hpmvs_octree_locate_batch): root->at(p), getRoot()->contains(p) and the leaf
    // DynOctTree::addConditional(p, addWidth) would put p in.  OctreeIndex names the tree by path keys (sentinel bit, 3 bits per
    // level z y x, root = 1): every Branch below the root and the nonempty leaves; addWidth empty: no target keys.  False (and
    // hpmvs_last_error) when the keys are no tree.  The batched level on top of the same look-ups is
    // PatchOptimizer::extendLevelTree / filterExtendLevelTree (ONE hpmvs_extend_tree_batch per level).
    struct OctreeLocation {
        std::vector<uint8_t> inside;       // [n] root.contains(p)
        std::vector<uint64_t> leafKey;     // [n] path key of the located leaf
        std::vector<int32_t> leafIndex;    // [n] index into OctreeIndex::leafKeys, -1: an empty leaf
        std::vector<float> leafWidth;      // [n]
        std::vector<float> leafCenter;     // [n][3]
        std::vector<uint64_t> targetKey;   // [n] 0: addConditional refuses
    };
    bool octreeLocate(const OctreeIndex& tree, const std::vector<float>& points /*[n][3]*/, const std::vector<float>& addWidth /*[n] or empty*/,
                      OctreeLocation& out) const;
    // A round's border patches (CellProcessor.cpp:487-540), each as ONE batched GPU call.  octreeRoute: for every point the index
    // of the first root in list order (roots [t][4]: c_, width_) that contains it, -1 when none does (distributeBorderCell).
    // octreeInsert: DynOctTree::addConditional(points[i], addWidth[i]) for i = 0 .. n - 1 IN THAT ORDER, every patch seeing the
    // leaves of the earlier ones (processBorderCellQueue's loop; addWidth = scale_3dx_ * 2.0 there).  The tree is not changed:
    // the caller enters the accepted keys.  Results as hpmvs_octree_insert_batch's (include/hpmvs_amd.h).
    struct OctreeInsertion {
        std::vector<uint8_t> accepted;     // [n] addConditional's return
        std::vector<uint64_t> leafKey;     // [n] *outleaf: the leaf the patch went into, or the one that refused it
        std::vector<int32_t> blocker;      // [n] the earlier patch behind a refusal; -1: accepted, or refused by the tree itself
    };
    bool octreeInsert(const OctreeIndex& tree, const std::vector<float>& points /*[n][3]*/, const std::vector<float>& addWidth /*[n]*/,
                      OctreeInsertion& out) const;
    bool octreeRoute(const std::vector<float>& roots /*[t][4]*/, const std::vector<float>& points /*[n][3]*/, std::vector<int32_t>& out) const;
    // Both of them for a whole round's border queue and ALL subtrees as ONE batched GPU call (hpmvs_border_forest_batch):
    // patches[i] is handed to the first tree of the forest whose root contains center_, inserted in queue order among the rows of
    // its tree with addConditional(center_, scale_3dx_ * 2.0), and with setDepths the accepted ones write their depths.  Thin
    // marshalling through OctreeForest::flatten; the forest and the patches are not changed.  Results as the call's
    // (include/hpmvs_amd.h): leafKey is relative to the row's own tree, blocker an index into this queue.
    bool octreeBorderForest(const OctreeForest& forest, const Patch3d* const* patches, size_t n, bool setDepths,
                            BorderForestInsertion& out) const;
    // getSubTrees(scene.patchTree_, subTrees, FLAGS_subtrees) of the reference's main (src/main.cpp:50-96) and
    // DynOctTree::cellHistogram as ONE batched GPU call (hpmvs_octree_partition): the subtree roots in the reference's list order
    // (the order octreeRoute takes), every key's subtree and its key re-based on that root, and the Leaf_iterator order that
    // initFromTree seeds each CellProcessor's queue in.  minSplitLeaves is the reference's constant 100.  Nonempty leaves in no
    // subtree (nOrphans) are reference behaviour: they stay in the tree, nothing extends them.  False (and
    // hpmvs_last_error) when the keys are no tree, minTrees > HPMVS_MAX_SUBTREES or minSplitLeaves < 1.
    bool octreePartition(const OctreeIndex& tree, int minTrees, OctreePartition& out, int minSplitLeaves = 100) const;
    // Scene::saveAsNVM (src/hpmvs/Scene.cpp:646-713): the scene as a VisualSFM dataset in the frame the output is expressed in.
    // <folder>/imgs/<i>.jpg is view i's undistorted level 0, encoded where it lies in HBM (hpmvs_scene_get_level_jpeg at CImg's
    // quality 100: libjpeg's file byte for byte); <folder>/project.nvm holds per view f = kMat_[0](0,0), the de-homogenised
    // centre, r = 0 and the quaternion <wxyz> of the matrix whose rows are the normalised axes, and per patch one point with
    // its colour, its centre and one measurement per attached image at the camera's level-0 projection of the centre; an empty
    // model follows, as in the reference.  The reference walks its patchTree_; here the patches are handed in, as they are to
    // writeExtPly.  The quaternion is normalised in double behind the conversion (the reference leaves the float axes' 1e-7).
    // False, with the reason on stderr, when a folder or file cannot be written or a view cannot be encoded.
    bool saveAsNVM(const char* folder, const std::vector<Ppatch3d>& patches) const;
    // Scene::visualizeDepths (src/hpmvs/Scene.cpp:434-516): the depth maps as jet-coloured JPEG files with an overview.html
    // table around them, the reference's markup and column order.  Per view i: <i>_col.jpg, pyramid level 1's pixels;
    // <i>_all.jpg, the getFullDepth map over all levels ("Combined"); <i>_<l>.jpg for l < cameras_[0].getLevels(), level l's map.
    // Every image is normalised, coloured (CImg's normalize(0, 255) and jet_LUT256(), byte for byte) and encoded at quality 100
    // where the maps lie in HBM (hpmvs_scene_depth_jpeg, hpmvs_scene_get_level_jpeg): no cell and no pixel visits the host.
    // The one difference: an image under 8 pixels on a side (the encoder's lower bound) has no file, and its table cell holds
    // the text <cols>x<rows> instead of an <img>.  The folder is created when it is missing.  False when the maps do not exist
    // (resetDepths), a device call fails (hpmvs_last_error names the reason, also on stderr) or a file cannot be written
    // (the reason on stderr, as saveAsNVM reports it).
    bool visualizeDepths(const char* folder) const;
    // scene.patchTree_.toExtPly(name, ...) (include/hpmvs/doctree.h:526-622, the file main writes after every tenth priority and as
    // patches-final.ply) with the reference's own defaults, ASCII: the header, per patch x y z [nx ny nz] red green blue
    // [scalar_scale], then per patch its image list.  Float-to-text conversion, the lines' placement and their writing run on the
    // scene's device (hpmvs_ply_ext_batch); the file equals writeExtPly's (PlyWriter.h) byte for byte for colours in [0, 256).  A
    // colour outside is clamped to 0 .. 255 and a NaN gives 0: the reference's ASCII path prints (int) color_ there (300, -3),
    // its binary path and writeExtPly convert with an undefined (unsigned char).  The image lists travel as one dense
    // patches x longest-list array: one long list widens every row.  The reference walks its patchTree_; here the patches are handed in, as they are to saveAsNVM, in the order they
    // are to be written.  False, with the reason on stderr as saveAsNVM reports it, when the device call fails or the file cannot be written.
    bool toExtPly(const char* name, const std::vector<Ppatch3d>& patches, bool binary = false, bool normal = true, bool scale = true,
                  bool visibility = true) const;
    std::map<std::string, int> dict_;
    std::vector<Camera> cameras_;
    std::vector<Image> images_;
    std::vector<std::vector<int> > covis_;
    // HBM-resident copy, created on first use (thread-safe), device = HPMVS_DEVICE env or 0
    hpmvs_scene* deviceScene() const;
    int device() const { return device_; }
    void setDevice(int d) { device_ = d; }
    // Combines concurrent single-patch PatchOptimizer::optimize() calls of several host threads (the reference's
    // callers: one optimizer per OpenMP thread, Scene.cpp:94-96,166-167, CellProcessor.cpp:129,256) into batched
    // device launches; opaque, owned by the scene
    void* combiner() const;
private:
    // the one implementation under both initPatches: sphere = cx cy cz r, or null for no gate
    bool initPatchesGated(const NVM_Model& model, const HpmvsOptions& options, std::vector<Ppatch3d>& out, const double* sphere,
                          std::vector<int>* stage) const;
    mutable hpmvs_scene* dev_;
    mutable void* combiner_ = nullptr;
    mutable std::mutex mu_;
    int device_;
    int maxLevel_;
};
}  // namespace mo3d
#endif
