/*
 * hpmvs_amd.h -- C ABI of the MI355X-native HPMVS patch-refinement path.
 *
 * This is the drop-in boundary for the ONE hot path of alexlocher/hpmvs:
 * mo3d::PatchOptimizer::optimize(Patch3d&) and everything below it
 * (reference src/hpmvs/PatchOptimizer.cpp:78-103).  Plain pointers and sizes only;
 * no C++/torch types.  The C++ mirror of the reference interface
 * (include/hpmvs/PatchOptimizer.h, Patch3d.h, ...) is a thin layer over these calls.
 *
 * Every entry point returns HPMVS_OK or a negative error; hpmvs_last_error() gives text.
 * Per-patch failure ("drop this patch", the reference's `return false`) is NOT an error:
 * it is reported in hpmvs_patch_batch::ok.
 *
 * Reference interfaces replaced (file:line relative to the reference root):
 *   hpmvs_scene_*            <- the const Scene view PatchOptimizer caches at construction,
 *                               src/hpmvs/PatchOptimizer.cpp:38-41 (cameras_, images_, covis_;
 *                               include/hpmvs/Scene.h:69-71), filled by Scene::addCameras
 *                               (src/hpmvs/Scene.cpp:42-88: Image::load pyramid, Camera::init)
 *                               and Scene::extractCoVisiblilty (Scene.cpp:241-298).
 *   hpmvs_optimize_batch     <- PatchOptimizer::optimize, PatchOptimizer.cpp:78-103, over a batch
 *                               (the OpenMP seed loop of Scene::initPatches, Scene.cpp:114-167).
 *   hpmvs_objective_batch    <- PatchOptimizer::static_objective_fn / objective_fn,
 *                               PatchOptimizer.cpp:286-320 (what NLopt calls back).
 *   hpmvs_inccs_batch        <- PatchOptimizer::setINCCs, PatchOptimizer.cpp:448-474.
 *   hpmvs_build_pyramid      <- Image::load's pyramid, src/hpmvs/Image.cpp:55-63
 *                               (CImg get_resize_halfXY, thirdLibs/cimg/CImg.h:21189-21203).
 *   hpmvs_undistort,         <- Image::undistort, src/hpmvs/Image.cpp:68-146 (run by Image::load for
 *   hpmvs_scene_set_view_distorted  k1 != 0, :50-53), before the pyramid.
 *   hpmvs_jpeg_decode,       <- Image::load's CImg / libjpeg read of the view, src/hpmvs/Image.cpp:46
 *   hpmvs_scene_set_view_jpeg   (thirdLibs/cimg/CImg.h:36920-36934).
 *   hpmvs_jpeg_encode,       <- the views Scene::saveAsNVM writes, src/hpmvs/Scene.cpp:646-713, through CImg's save_jpeg
 *   hpmvs_scene_get_level_jpeg  and libjpeg at quality 100 (thirdLibs/cimg/CImg.h:40748-40838).
 *   hpmvs_scene_depth_image, <- the images Scene::visualizeDepths saves, src/hpmvs/Scene.cpp:434-516, through CImg's
 *   hpmvs_scene_depth_jpeg      normalize, map and jet_LUT256 (thirdLibs/cimg/CImg.h:18423-18435, 19034-19078, 19331-19341).
 *   hpmvs_init_patches_batch <- the seed loop of Scene::initPatches, src/hpmvs/Scene.cpp:112-178.
 *   hpmvs_init_patches_sphere_batch <- the same loop with the scene-centre gate of --only_sphere
 *                               (options.FILTER_SCENE_CENTER), src/hpmvs/Scene.cpp:105-121.
 *   hpmvs_scene_center       <- Scene::getSceneCenter, src/hpmvs/Scene.cpp:210-239 (TriangulateMidpoint,
 *                               include/hpmvs/Triangulation.hpp:28-53).
 *   hpmvs_expand_batch       <- the candidate loops of CellProcessor::extend / ::branch,
 *                               src/hpmvs/CellProcessor.cpp:84-142 and :210-262.
 *   hpmvs_regularize_batch   <- CellProcessor::regularize, src/hpmvs/CellProcessor.cpp:309-367.
 *   hpmvs_filter_batch       <- CellProcessor::filter, src/hpmvs/CellProcessor.cpp:43-82.
 *   hpmvs_seed_tree_batch    <- the second half of Scene::initPatches, src/hpmvs/Scene.cpp:183-199
 *                               (getBoundingBox, swapRoot, the scale floor, patchTree_.add, setDepths).
 *   hpmvs_octree_locate_batch <- the tree look-ups of CellProcessor::extend, src/hpmvs/CellProcessor.cpp:122-125, 147-154.
 *   hpmvs_extend_tree_batch   <- CellProcessor::extend's candidate loop with both tree look-ups, src/hpmvs/CellProcessor.cpp:84-154.
 *   hpmvs_extend_forest_batch <- the same for all subtrees of getSubTrees' list at once (one processQueue level each, src/main.cpp).
 *   hpmvs_process_forest_batch <- the regularize / settle sweep (priorities L*10+1 / +2) over all subtrees at once, in queue order.
 *   hpmvs_octree_route_batch, <- CellProcessor::distributeBorderCell and ::processBorderCellQueue,
 *   hpmvs_octree_insert_batch    src/hpmvs/CellProcessor.cpp:487-540 (the root search and the addConditional loop).
 *   hpmvs_border_forest_batch <- both of them for a whole round's border queue over all subtrees at once, with the accepted
 *                                patches' setDepths (CellProcessor.cpp:487-540): the third forest call of a tree level.
 *   hpmvs_octree_partition    <- getSubTrees, src/main.cpp:50-96, and DynOctTree::cellHistogram, doctree.h:493-511.
 *   hpmvs_camera_from_nvm    <- Camera::init, src/hpmvs/Camera.cpp:34-81.
 */
#ifndef HPMVS_AMD_H
#define HPMVS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPMVS_OK 0
#define HPMVS_ERR_HIP (-1)     /* a HIP runtime call failed */
#define HPMVS_ERR_ARG (-2)     /* bad argument */
#define HPMVS_ERR_STATE (-3)   /* scene not committed / already committed */
#define HPMVS_ERR_NODEVICE (-4) /* no gfx950 device visible: there is NO CPU fallback */
#define HPMVS_ERR_UNSUPPORTED (-5) /* a well-formed input of a kind that is not handled (JPEG: see hpmvs_jpeg_decode, hpmvs_jpeg_encode) */

#define HPMVS_MAX_LEVELS 8
#define HPMVS_MAX_IMAGES 256 /* images attached to one patch (reference: unbounded vector<int>); overflow => stage 100.  Lists of up to
                              HPMVS_FAST_IMAGES ids run in the batch kernel; a patch whose list outgrows that at any point of the
                              pipeline is redone by the wide kernel behind it (same launch, same results, one patch per wavefront) */
#define HPMVS_FAST_IMAGES 64
#define HPMVS_RECORD_IMAGES 64 /* ids an hpmvs_record carries */

typedef struct hpmvs_scene hpmvs_scene; /* opaque; owns the HBM-resident pyramids and tables */

/* include/hpmvs/HpmvsOptions.h:29-58, the fields the path reads */
typedef struct {
    int32_t MAXLEVEL;             /* 5 */
    int32_t MINLEVEL;             /* 0 */
    float MAX_ANGLE;              /* 60 deg in rad */
    float MIN_ANGLE;              /* 10 deg in rad */
    int32_t MAX_IMAGES_PER_PATCH; /* 6 (dead in the reference) */
    int32_t MIN_IMAGES_PER_PATCH; /* 3 */
    float NCC_ALPHA_1;            /* 0.4 */
    float NCC_ALPHA_2;            /* 0.5 */
} hpmvs_options;

/* What the path reads of mo3d::Camera (include/hpmvs/Camera.h:87-105).  Level l's projection is
 * diag(2^-l, 2^-l, 1) * P0 exactly (src/hpmvs/Camera.cpp:55-63 halves rows 0,1 per level), so only
 * level 0 is passed. */
typedef struct {
    float P0[12];    /* projection_[0], row-major 3x4 */
    float center[4]; /* center_ (w = 1) */
    float xaxis[3];  /* xAxis_ */
    float yaxis[3];  /* yAxis_ */
    float zaxis[3];  /* zAxis_ */
    float fsum;      /* kMat_[0](0,0) + kMat_[0](1,1) */
    int32_t n_levels; /* projection_.size() = MAXLEVEL + 1 */
} hpmvs_camera;

/* A batch of Patch3d records (include/hpmvs/Patch3d.h:33-83) in structure-of-arrays form.
 * All pointers are host pointers unless `on_device` is set in the call, in which case all are
 * device pointers on the scene's GPU.  Inputs are updated in place only for patches with ok=1
 * (reference: patch untouched on failure, PatchOptimizer.cpp:86-87). */
typedef struct {
    int32_t n;           /* number of patches */
    int32_t max_images;  /* row stride of `images` (<= HPMVS_MAX_IMAGES) */
    float *center;       /* [n][4] center_ (w = 1)            in/out */
    float *normal;       /* [n][4] normal_ (w = 0)            in/out */
    float *scale;        /* [n]    scale_3dx_                 in (returned unchanged) */
    int32_t *n_images;   /* [n]    images_.size()             in/out */
    int32_t *images;     /* [n][max_images] images_, [0] = reference image   in/out */
    uint8_t *ok;         /* [n]    return value of optimize() out */
    float *color;        /* [n][3] color_ (valid when ok)     out */
    float *ncc;          /* [n]    ncc_ (constant 1.4f as in the reference, PatchOptimizer.cpp:95) out */
    /* diagnostics the reference computes and discards (may be NULL) */
    double *fmin;        /* [n]    final mean robust INCC (NLopt minf) */
    double *x;           /* [n][3] final optimiser variables (depth, angle1, angle2) */
    int32_t *result;     /* [n]    nlopt_result code of the BOBYQA run */
    int32_t *nevals;     /* [n]    objective evaluations */
    int32_t *stage;      /* [n]    0 = ok, else index of the pipeline stage that returned false (1..9);
                          *        100 = attached-image list overflow, 101 = an image id outside the scene */
    int32_t *ngrabs;     /* [n]    sampleTexture calls that passed the gates (588 B of image each) */
} hpmvs_patch_batch;

/* ---- library ---------------------------------------------------------------------------- */
const char *hpmvs_last_error(void);
int hpmvs_device_count(void);
/* Identifies the build of this library: a hash of its sources taken by the Makefile.  Measurement records
 * (profiles/pmc_traffic.json) carry it, so that counters are never reported beside another kernel's time. */
const char *hpmvs_build_id(void);
void hpmvs_default_options(hpmvs_options *o);

/* Host-side Camera::init (reference src/hpmvs/Camera.cpp:34-81): NVM camera (focal length,
 * rotation quaternion wxyz world->camera in double, centre; include/hpmvs/NVMReader.h:44-50) and the
 * level-0 image size -> the float32 tables above.  Pure host code, usable without a GPU. */
int hpmvs_camera_from_nvm(double f, const double q_wxyz[4], const double c[3], int width, int height,
                          int max_level, hpmvs_camera *out);

/* Host-side Scene::getSceneCenter (reference src/hpmvs/Scene.cpp:210-239): the sphere --only_sphere
 * (options.FILTER_SCENE_CENTER) keeps NVM points in.  Pure host code in float64, usable without a GPU.
 *   d_i = (double)zaxis normalised, o_i = (double)center[0..2] / (double)center[3];
 *   A = sum_i (I - d_h d_h^T), b = sum_i (I - d_h d_h^T) (o_i, 1) as 4x4 / 4, in camera order (TriangulateMidpoint,
 *   include/hpmvs/Triangulation.hpp:35-45); A x = b; center = x[0..2] / x[3]; radius = max_i |center - o_i| (the reference's
 *   live line takes the maximum, Scene.cpp:233, not the median).
 * The system is solved by Householder QR with column pivoting, the method of the reference's Eigen::ColPivHouseholderQR but
 * not Eigen's code: the centre equals the reference's to solver accuracy -- about 64 * 2^-52 * |A^-1| (|A| |x| + |b|),
 * 4e-13 for three cameras 30 from the origin -- not bit for bit.  An NVM point within that distance of the sphere's surface
 * can therefore fall on the other side than in a particular Eigen build.
 * *valid = 1 and HPMVS_OK when center[3] and *radius are set.  *valid = 0, still HPMVS_OK, with zeros in both, for
 *   n == 0 (the reference returns false),
 *   n == 1 (a departure: the reference aborts there, CHECK_GE(origins.size(), 2)),
 *   a numerically rank-deficient system: a diagonal entry of R with |R_kk| <= 64 * 2^-52 * |R_00|, which is all optical
 *   axes parallel to about 1e-7 rad (the reference returns whatever its QR yields), or a result that is not finite.
 * HPMVS_ERR_ARG for NULL pointers or n < 0. */
int hpmvs_scene_center(const hpmvs_camera *cams, int n, double center[3], double *radius, int *valid);

/* ---- scene (HBM-resident, immutable after commit; shared read-only by all callers) ------- */
int hpmvs_scene_create(int n_views, int device, hpmvs_scene **out);
/* Level-0 interleaved u8 RGB (row-major, 3*(y*W+x)+c: reference Image.h:93-105).  The pyramid is
 * built on the GPU by the half-resize kernel.  rgb_on_device != 0: `rgb_l0` is a device pointer. */
int hpmvs_scene_set_view(hpmvs_scene *s, int view, int width, int height, const uint8_t *rgb_l0,
                         int rgb_on_device, const hpmvs_camera *cam);
int hpmvs_scene_set_covis(hpmvs_scene *s, int view, const int32_t *ids, int n);
int hpmvs_scene_commit(hpmvs_scene *s);
int hpmvs_scene_destroy(hpmvs_scene *s);
/* copy one pyramid level back to the host (tests: bit-exact pyramid parity) */
int hpmvs_scene_get_level(const hpmvs_scene *s, int view, int level, uint8_t *host_out, size_t cap,
                          int *w, int *h);
size_t hpmvs_scene_bytes(const hpmvs_scene *s);

/* stand-alone pyramid kernel: src (w x h, device or host) -> dst (w/2 x h/2).  A `device` that is no index of a visible
 * device is HPMVS_ERR_ARG "build_pyramid: bad device index", as for every entry that takes one (it used to be
 * HPMVS_ERR_HIP with the text of the failed hipSetDevice). */
int hpmvs_build_pyramid(int device, const uint8_t *src, int w, int h, uint8_t *dst, int on_device);

/* ---- radial undistortion (VisualSFM's one-parameter model: NVM camera field r) ------------- */
/* Image::undistort of the reference: every output pixel samples the raw level 0 at the point m that satisfies
 * m (1 + k1 |m|^2) = p in coordinates normalised by f around (w/2, h/2), bilinearly as CImg does, truncated to u8.
 * `f` and `k1` are the float values the reference keeps (Image::f_, Image::k1_).  Pixels whose source point falls
 * outside (1, w-1) x (1, h-1) -- the reference leaves them as uninitialised memory -- are 0 here.
 * All three entries: HPMVS_ERR_ARG unless k1 is finite and f is finite and > 0; HPMVS_ERR_NODEVICE without a device. */
/* src -> dst, both w x h interleaved u8 RGB (device pointers when on_device != 0, else host); the two buffers must not
 * overlap.  k1 == 0 returns src byte for byte (the reference never resamples such a view). */
int hpmvs_undistort(int device, const uint8_t *src, int w, int h, float f, float k1, uint8_t *dst, int on_device);
/* diagnostics: xy [h][w][2] (host) = the float source point each output pixel samples, NaN included */
int hpmvs_undistort_map(int device, int w, int h, float f, float k1, float *xy);
/* hpmvs_scene_set_view for a raw view: level 0 is undistorted on the GPU, then the pyramid is built from it.  A host
 * rgb_raw is copied to the device first; a device one (rgb_on_device != 0) is read in place.  k1 == 0 is exactly
 * hpmvs_scene_set_view. */
int hpmvs_scene_set_view_distorted(hpmvs_scene *s, int view, int width, int height, const uint8_t *rgb_raw,
                                   int rgb_on_device, const hpmvs_camera *cam, float f, float k1);

/* ---- baseline JPEG views (what VisualSFM's NVM files name) ---------------------------------- */
/* Image::load of the reference reads a view through CImg and libjpeg with the library's defaults (JDCT_ISLOW, fancy
 * upsampling, the integer YCbCr tables); these entries give the same pixels byte for byte.  The host parses the markers
 * and decodes the entropy data of the one scan into int16 coefficients, on the calling thread (callers parallelise over
 * views, as the reference's loop over cameras does); dequantisation, the 8x8 IDCT, chroma interpolation and the colour
 * conversion run on the GPU (kernel_jpeg.hip).
 * Decoded: 8-bit baseline or extended-sequential Huffman files (SOF0, SOF1) with 8-bit quantisation tables, one component
 *   (grayscale, written as R = G = B) or three as YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, all components in
 *   one scan, with or without restart intervals, 8 to 65535 pixels on a side and fewer than 4 Gi samples in all.
 * HPMVS_ERR_UNSUPPORTED: progressive, arithmetic-coded, lossless or hierarchical frames; 12-bit samples; four components;
 *   data libjpeg would take for RGB-coded (Adobe APP14 with transform 0, or component ids 'R','G','B', without JFIF); other
 *   sampling factors; more than one scan; 16-bit quantisation tables; an image under 8 pixels on a side.
 * HPMVS_ERR_ARG: anything malformed, and a truncated file (libjpeg would pad it with grey and warn; here it is refused).
 * hpmvs_last_error names the reason.  The file bytes are always host memory; every read of them is bounds checked. */
/* Pure host code, usable without a GPU.  It walks the whole file, entropy data included, and so returns what the decoder
 * would.  h_samp, v_samp: the luma sampling factors (1,1 / 2,1 / 2,2; 1,1 for grayscale). */
int hpmvs_jpeg_info(const uint8_t *bytes, size_t n, int *width, int *height, int *components, int *h_samp, int *v_samp);
/* rgb: width x height interleaved u8 RGB, 3*(y*W+x)+c, host memory or (rgb_on_device != 0) device memory on `device`;
 * exactly 3*W*H bytes are written.  HPMVS_ERR_ARG for NULL pointers and for cap < 3*W*H; arguments and the file are
 * checked before the device is looked for (HPMVS_ERR_NODEVICE).  Working buffers (2 bytes of coefficients and 1 byte of
 * sample planes per sample) live for the call only. */
int hpmvs_jpeg_decode(int device, const uint8_t *bytes, size_t n, uint8_t *rgb, size_t cap, int rgb_on_device);
/* diagnostics (tools/jpeg_scale.py): hpmvs_jpeg_decode to a device buffer, with the time of its stages in ms[4]: host parse
 * and entropy decode (wall clock, this thread), coefficient upload, IDCT kernel, RGB kernel (HIP events) */
int hpmvs_jpeg_decode_timed(int device, const uint8_t *bytes, size_t n, uint8_t *rgb_device, size_t cap, float *ms);
/* diagnostics (tools/jpeg_entropy_scale.py): the same with the scan decoded on the device and no fallback (HPMVS_ERR_STATE
 * as hpmvs_jpeg_decode_ex with _DEVICE), stages in ms[12]: [0] host prescan (wall clock); by HIP events [1] uploads of the
 * scan and its tables with the fills, [2] jpeg_entropy_sync_kernel summed over its passes, [3] the passes with the read-backs
 * between them, [4] jpeg_entropy_scan_local_kernel, [5] _scan_groups, [6] _check, [7] _write, [8] quantiser upload, [9] IDCT
 * kernel, [10] RGB kernel; [11] the synchronisation rounds taken */
/* diagnostics: what decoded the scan in the calling thread's last successful JPEG decode through any entry above --
 * *used HPMVS_JPEG_ENTROPY_HOST or _DEVICE, *rounds (nullable) the device's synchronisation rounds.  It shows what
 * hpmvs_jpeg_decode and hpmvs_scene_set_view_jpeg, which report nothing, made of HPMVS_JPEG_ENTROPY and of the _AUTO
 * threshold.  HPMVS_ERR_STATE before the thread's first such decode. */
int hpmvs_jpeg_last_decode(int *used, int *rounds);
int hpmvs_jpeg_entropy_timed(int device, const uint8_t *bytes, size_t n, uint8_t *rgb_device, size_t cap, float *ms);
/* hpmvs_scene_set_view for a view given as JPEG file bytes: level 0 is decoded in HBM (the pixels never visit the host),
 * undistorted there when k1 != 0 (as hpmvs_scene_set_view_distorted does, and with its rules for f and k1, which hold for
 * k1 == 0 too), and the pyramid is built from it.  Width and height are the file's (hpmvs_jpeg_info).  Calls for different
 * views of one scene are as independent of each other as those of hpmvs_scene_set_view; nothing is kept between calls. */
int hpmvs_scene_set_view_jpeg(hpmvs_scene *s, int view, const uint8_t *bytes, size_t n, const hpmvs_camera *cam, float f,
                              float k1);
/* Where the scan's Huffman data is decoded.  _HOST: the bit-serial walk on the calling thread, as hpmvs_jpeg_info does it.
 * _DEVICE: on the GPU (kernel_jpeg_entropy.hip): the host removes the byte stuffing and finds the restart markers, the scan's
 * bytes go up instead of the coefficients, and subsequences of the scan are decoded in parallel until each starts where the
 * one before it ended; a check kernel accepts that chain only if it is the sequential decode and one the host walk accepts.
 * An accepted chain gives the host walk's coefficients bit for bit.  Anything else -- a chain the check refuses, more
 * synchronisation rounds than the cap, FF FF fill bytes in the scan, restart markers or an end of scan that the prescan does
 * not vouch for, working buffers the device cannot allocate -- is left to the host walk, whose code, message and pixels are then the call's: no refusal, message or pixel
 * depends on this choice.  _AUTO: the device for scans of HPMVS_JPEG_AUTO_MIN_SCAN_BYTES and more, the host below.
 * hpmvs_jpeg_decode and hpmvs_scene_set_view_jpeg are the _ex entries with what the environment variable
 * HPMVS_JPEG_ENTROPY=host|device|auto names (read once per process; unset or anything else: auto); its `device` still leaves
 * to the host walk what the device does not take.
 * The _ex entries called with _DEVICE themselves do NOT fall back: where the host walk would have to run they return
 * HPMVS_ERR_STATE with the reason in hpmvs_last_error (a file whose headers are refused keeps its own code).
 * *used (nullable): HPMVS_JPEG_ENTROPY_HOST or _DEVICE, what decoded the scan.  HPMVS_ERR_ARG for another `entropy` value. */
enum { HPMVS_JPEG_ENTROPY_AUTO = 0, HPMVS_JPEG_ENTROPY_HOST = 1, HPMVS_JPEG_ENTROPY_DEVICE = 2 };
#define HPMVS_JPEG_AUTO_MIN_SCAN_BYTES 445155 /* measured: profiles/jpeg_entropy_scale.json, DESIGN.md 3.13 */
int hpmvs_jpeg_decode_ex(int device, const uint8_t *bytes, size_t n, uint8_t *rgb, size_t cap, int rgb_on_device, int entropy,
                         int *used);
int hpmvs_scene_set_view_jpeg_ex(hpmvs_scene *s, int view, const uint8_t *bytes, size_t n, const hpmvs_camera *cam, float f,
                                 float k1, int entropy, int *used);
/* The dense coefficients behind the entropy decode, to host memory: per component [blocks_y][blocks_x][64] int16 in natural
 * order, the components one behind the other, blocks padded to whole MCUs (cap: int16 elements available at coef).
 * subseq_bits: the subsequence size of the device decode, 0 for the shipped one (512), else a multiple of 32 from 64 up --
 * a test hook that puts subsequence boundaries at every position of a small file.  The cap on synchronisation rounds
 * shrinks as the size grows (740 * 512 / subseq_bits, rounded down): above 378 880 bits it is 0, and only a scan whose
 * segments are one subsequence each is decoded on the device.  *rounds (nullable): synchronisation
 * rounds the device decode took (0 on the host).  HPMVS_ERR_ARG before any write for a bad entropy or subseq_bits value
 * and a short cap; _DEVICE as above. */
int hpmvs_jpeg_coefficients(int device, const uint8_t *bytes, size_t n, int entropy, int subseq_bits, int16_t *coef, size_t cap,
                            int *used, int *rounds);

/* ---- baseline JPEG files written from pixels in HBM ----------------------------------------- */
/* Scene::saveAsNVM of the reference writes every undistorted view through CImg's save_jpeg: jpeg_set_defaults, then
 * jpeg_set_quality(q, TRUE), on RGB rows -- YCbCr 4:2:0, JDCT_ISLOW, the Annex K Huffman tables, no restart markers, no
 * optimised coding.  These entries write the file libjpeg writes for that, byte for byte (pinned to Pillow over
 * libjpeg-turbo: tests/golden/g8_jpeg_enc.npz).  Colour conversion, edge replication, downsampling, the forward DCT, the
 * quantiser, the Huffman coding and the byte stuffing run on the GPU (kernel_jpeg_encode.hip); the host receives the stuffed
 * entropy data and its length and puts the 623-byte header in front and EOI behind.
 * HPMVS_ERR_ARG: a NULL pointer, quality outside 1 .. 100, a side above 65535, cap smaller than the file (nothing is
 *   written to `out`; *n still names the file's length, so a second call can bring the right buffer).
 * HPMVS_ERR_UNSUPPORTED: a side under 8 pixels -- the lower bound of hpmvs_jpeg_decode, so that everything written here
 *   can be read back here.  Arguments are checked before the device is looked for (HPMVS_ERR_NODEVICE).
 * Calls are independent and keep nothing between them; working buffers live for the call only. */
/* An upper bound of the file for a width x height image at any quality: every block's code at its longest (under 208
 * bytes), every byte of it stuffed.  Noise at quality 100 gives files larger than the raw pixels.  0 for sides outside
 * 1 .. 65535. */
size_t hpmvs_jpeg_encode_bound(int width, int height);
/* rgb: width x height interleaved u8 RGB, 3*(y*W+x)+c, host memory or (rgb_on_device != 0) device memory on `device`;
 * out: host memory of cap bytes; *n: the bytes written. */
int hpmvs_jpeg_encode(int device, const uint8_t *rgb, int width, int height, int quality, uint8_t *out, size_t cap, size_t *n,
                      int rgb_on_device);
/* A pyramid level of a scene's view encoded where it lies: no pixel visits the host.  Level 0 of a view with k1 != 0 holds
 * the undistorted pixels, the frame every patch and camera of the output is expressed in.  out == NULL: *n = the bound for
 * the level's size and nothing else happens (as hpmvs_scene_get_level reports sizes).  HPMVS_ERR_ARG for a bad view or
 * level; a level under 8 pixels on a side is HPMVS_ERR_UNSUPPORTED.  Works before and after hpmvs_scene_commit. */
int hpmvs_scene_get_level_jpeg(const hpmvs_scene *s, int view, int level, int quality, uint8_t *out, size_t cap, size_t *n);
/* diagnostics (tools/jpeg_encode_scale.py): hpmvs_jpeg_encode of a device buffer with the time of its stages in ms[8], by
 * HIP events: [0] the first working buffer and the tables' upload, [1] jpeg_enc_coef_kernel, [2] jpeg_enc_length_kernel, the
 * scan of the lengths and the total's read-back, [3] the second working buffer and its fills, [4] jpeg_enc_write_kernel,
 * [5] jpeg_enc_ff_kernel, the scan of the counts and the total's read-back, [6] jpeg_enc_stuff_kernel, [7] the entropy
 * data's copy to the host. */
int hpmvs_jpeg_encode_timed(int device, const uint8_t *rgb_device, int width, int height, int quality, uint8_t *out, size_t cap,
                            size_t *n, float *ms);

/* ---- depth maps as jet-coloured images ------------------------------------------------------- */
/* Scene::visualizeDepths of the reference (src/hpmvs/Scene.cpp:434-516) renders every depth map, and per view the
 * getFullDepth map over all levels ("Combined"), as an image: a cell equal to MAX_DEPTH becomes 0, CImg's normalize(0, 255)
 * maps the image's least value m and largest value M to 0 and 255 in float32 (m == M: every pixel 0; m == 0 and M == 255:
 * left as it is), the truncated result indexes CImg's 256-entry jet_LUT256().  These entries give that image byte for
 * byte (tests/golden/g9_depth_vis.npz) from the maps where they lie in HBM (hpmvs_scene_depth_reset): no cell and no pixel
 * visits the host (kernel_depth_vis.hip).  The image of a level is cols wide and rows high, pixel (x, y) the map's element
 * (y, x): the transpose of the column-major memory order.  The combined image has level 0's size; its pixel (x, y) is the
 * least cell over the levels at (x >> l, y >> l), up to the first level where that cell lies outside the map.
 * A cell that is no finite number counts as empty (the reference's result for one is undefined); negative finite cells are
 * ordinary values.  The maps are only read.  Calls are ordered behind pending map writes as hpmvs_scene_depth_get_level is,
 * keep nothing between them and may run concurrently.
 * level: 0 .. n_levels - 1 or HPMVS_DEPTH_COMBINED.  HPMVS_ERR_STATE without depth maps and HPMVS_ERR_ARG for a bad view /
 * level, as the depth-map entries report them; arguments are checked before the device is touched. */
#define HPMVS_DEPTH_COMBINED (-1)
/* host only: the 256 RGB entries of the colormap, entry i at lut[3*i .. 3*i+2] */
int hpmvs_depth_colormap(uint8_t lut[768]);
/* rgb: width x height interleaved u8 RGB, 3*(y*W+x)+c, host memory or (rgb_on_device != 0) device memory on the scene's
 * device, of cap >= 3*W*H bytes (else HPMVS_ERR_ARG); rgb == NULL: a size query, only *width and *height are set (both
 * nullable).  range (nullable): m and M as used. */
int hpmvs_scene_depth_image(const hpmvs_scene *s, int view, int level, uint8_t *rgb, size_t cap, int rgb_on_device, int *width,
                            int *height, float range[2]);
/* That image as the baseline JPEG file hpmvs_jpeg_encode writes for it, with hpmvs_scene_get_level_jpeg's conventions:
 * out == NULL: *n = the bound; cap smaller than the file: HPMVS_ERR_ARG, nothing written, *n the length needed; a map under
 * 8 cells on a side: HPMVS_ERR_UNSUPPORTED. */
int hpmvs_scene_depth_jpeg(const hpmvs_scene *s, int view, int level, int quality, uint8_t *out, size_t cap, size_t *n);

/* ---- the hot path ------------------------------------------------------------------------- */
/* Full optimize() for every patch of the batch.  `stream` is a hipStream_t (NULL = default
 * stream); with on_device != 0 the call only enqueues work on `stream`. */
int hpmvs_optimize_batch(const hpmvs_scene *s, const hpmvs_options *o, hpmvs_patch_batch *b,
                         int on_device, void *stream);

/* The seed-initialisation loop of Scene::initPatches (reference src/hpmvs/Scene.cpp:112-178) as one
 * call: for every NVM point build the seed patch on the GPU (centre = xyz, attached images = the
 * point's measurements that project inside the START_LEVEL image with a 2 px margin, normal towards the
 * first attached camera, scale = getScale(centre, START_LEVEL)), run optimize() on the whole batch,
 * and apply the post-gate |centre - xyz| <= 2 * scale (Scene.cpp:171).
 *   xyz[n][3] (float64), meas_off[n+1], meas_img[meas_off[n]] : NVM_Point::xyz / measurements[].imgIndex
 * `b` receives the seed patches (refined where ok[i] = 1).  stage[i] additionally uses
 *   10 = fewer than MIN_IMAGES_PER_PATCH measurements (Scene.cpp:127), 11 = fewer than 2 visible images
 *   (Scene.cpp:153), 12 = failed the drift gate (Scene.cpp:171).
 * Host or device pointers as for hpmvs_optimize_batch. */
int hpmvs_init_patches_batch(const hpmvs_scene *s, const hpmvs_options *o, int start_level, int n_points,
                             const double *xyz, const int32_t *meas_off, const int32_t *meas_img,
                             hpmvs_patch_batch *b, int on_device, void *stream);
/* The same loop behind the scene-centre gate of --only_sphere (reference src/hpmvs/Scene.cpp:118-121): a point with
 * |xyz - (cx, cy, cz)| > r is skipped before every other test,
 *   stage 13 = outside the scene sphere; it wins over 10, 11 and 100, which the reference tests afterwards.
 * The distance is float64 on the float64 xyz, sqrt((dx*dx + dy*dy) + dz*dz) without contraction, and the comparison is
 * `dist > r`: a point on the sphere is kept, a NaN coordinate is not gated (it goes on as in hpmvs_init_patches_batch), an
 * infinite one is gated.  Given (centre, radius) the gate is exact; hpmvs_scene_center's values equal the reference's to solver
 * accuracy only (see there).  A gated row comes back like every row rejected before optimize(): ok 0, n_images 0, centre
 * (float)xyz with w = 1, normal 0, scale 0; it costs what a stage-10 row costs.
 * sphere[4] = cx cy cz r is ALWAYS a host pointer, whatever on_device says.  NULL: no gate, which is
 * hpmvs_init_patches_batch itself (one implementation).  r = +inf gates nothing.  HPMVS_ERR_ARG for a centre that is not
 * finite and for a NaN or negative radius. */
int hpmvs_init_patches_sphere_batch(const hpmvs_scene *s, const hpmvs_options *o, int start_level, int n_points,
                                    const double *xyz, const int32_t *meas_off, const int32_t *meas_img,
                                    const double sphere[4], hpmvs_patch_batch *b, int on_device, void *stream);

/* Frontier expansion: the candidate loops of CellProcessor::extend (reference
 * src/hpmvs/CellProcessor.cpp:84-178) and CellProcessor::branch (:210-262) for a whole frontier of
 * octree cells in one call -- candidate construction, optimize() and the geometric acceptance gates.
 *   mode HPMVS_EXPAND_EXTEND : 6 candidates per parent on a hexagon of radius cell_width around the parent
 *        centre in the parent's tangent plane (x axis from the reference camera), scale = 0.9 * width / 2;
 *        accepted if optimize() succeeds, width/2 < 2*scale < width (:131-132) and the centre moved less
 *        than 1.5 * width from the PARENT centre (:133).
 *   mode HPMVS_EXPAND_BRANCH : 4 candidates at radius width/4 on the diagonals, scale = 0.45 * width / 2;
 *        only candidates inside the parent's cell are optimized (:247) and they must still be inside it
 *        afterwards (:257).
 * parents: n patches (center, normal, n_images, images are read; images[.][0] is the reference image);
 * cell_center[n][3], cell_width[n]: the octree leaf of each parent (Cell::c_, Cell::width_);
 * skip (optional, n*N bytes): nonzero = the caller already knows the candidate is not wanted (extend: the
 *   target leaf is occupied or finer, :120-124) -> it is built but not optimized;
 * out: batch of n*N patches, candidate k of parent i at index i*N + k, max_images = parents->max_images.
 *   ok = accepted; stage = 0, the optimize() stage 1..9/100, 20 = skipped / outside the cell before optimize,
 *   21 = scale gate, 22 = drift gate (extend) or left the cell (branch).  A candidate that fails keeps its
 *   constructed centre/scale (optimize() leaves failed patches untouched).
 * The depth / view-block / free-pixel tests (:135-142) and the octree insertion read and write scene state
 * that is order dependent in the reference; they stay with the caller.  Host or device pointers as for
 * hpmvs_optimize_batch. */
#define HPMVS_EXPAND_EXTEND 0
#define HPMVS_EXPAND_BRANCH 1
int hpmvs_expand_batch(const hpmvs_scene *s, const hpmvs_options *o, int mode, const hpmvs_patch_batch *parents,
                       const float *cell_center, const float *cell_width, const uint8_t *skip,
                       hpmvs_patch_batch *out, int on_device, void *stream);
/* the (cos, sin) pairs of the candidate directions the kernels use: dxdy[2*N], N = 6 (extend) or 4 (branch);
 * returns N.  (std::cos/std::sin of the float angle 2*pi/N*i [+ pi/4], CellProcessor.cpp:107-109, 233-235.) */
int hpmvs_expand_directions(int mode, float *dxdy);

/* objective_fn at optimiser variables x[n][3] for each patch's current image list, with
 * refCenter_/refRay_/axes taken from the patch as optimizePatch does.  f_out[n]. */
int hpmvs_objective_batch(const hpmvs_scene *s, const hpmvs_options *o, const hpmvs_patch_batch *b,
                          const double *x, double *f_out, int32_t *ngrabs_out, int on_device,
                          void *stream);

/* setINCCs(ref_idx, robust) for each patch: out[n][max_images] */
int hpmvs_inccs_batch(const hpmvs_scene *s, const hpmvs_options *o, const hpmvs_patch_batch *b,
                      int ref_idx, int robust, float *out, int on_device, void *stream);

/* ---- depth maps and the acceptance gates of the expansion (second half) ----------------------------------
 * The reference accepts a refined candidate only if it agrees with the depth maps written by the patches accepted
 * so far (src/hpmvs/CellProcessor.cpp:134-142, 198-200):
 *     Scene::depthTests(p, margin)    >= MIN_IMAGES_PER_PATCH      src/hpmvs/Scene.cpp:518-524, 531-580
 *     Scene::viewBlockTest(p, margin) <  MIN_IMAGES_PER_PATCH      src/hpmvs/Scene.cpp:607-642 (every view of the scene)
 *     Scene::pixelFreeTests(p)        >= MIN_IMAGES_PER_PATCH - 1 and > 0.75 * #images    src/hpmvs/Scene.cpp:582-605
 * and records an accepted patch with Scene::setDepths (src/hpmvs/Scene.cpp:351-381).  The maps live in HBM in the
 * reference's own layout -- per view and pyramid level an Eigen::MatrixXf(rows, cols), column-major, filled with
 * MAX_DEPTH = 1000, rows / cols = level size / DEPTH_SUBSAMPLE (src/hpmvs/Scene.cpp:33,74-80) -- so the unchanged
 * scheduler copies its matrices in and out as they are (matrix.data(), rows(), cols()).
 *   hpmvs_scene_depth_reset      allocate (first call) and fill every map with MAX_DEPTH
 *   hpmvs_scene_depth_set_level / _get_level   one map <-> host (get with data == NULL: shape query)
 *   hpmvs_set_depths_batch       setDepths(patch, subtract = false) for every patch of the batch with ok[i] != 0
 *                                (all patches when ok is NULL): a float minimum per cell, order-independent
 *   hpmvs_depth_gates_batch      the three counts per patch, read-only; the caller applies the thresholds.
 *                                abs_int selects the reading of the unqualified `abs(diff)` at Scene.cpp:571: 0 = the
 *                                <cmath> overload (fabsf), 1 = C's abs(int), which truncates the difference first --
 *                                which one a reference binary has depends on the headers its toolchain exports. */
int hpmvs_scene_depth_reset(hpmvs_scene *s);
int hpmvs_scene_depth_set_level(hpmvs_scene *s, int view, int level, const float *data, int rows, int cols);
int hpmvs_scene_depth_get_level(const hpmvs_scene *s, int view, int level, float *data, size_t capacity, int *rows, int *cols);
int hpmvs_set_depths_batch(hpmvs_scene *s, const hpmvs_patch_batch *b, int on_device, void *stream);
int hpmvs_depth_gates_batch(const hpmvs_scene *s, const hpmvs_patch_batch *b, float margin, int abs_int,
                            int32_t *n_visible, int32_t *n_blocking, int32_t *n_free, int on_device, void *stream);
/* Scene::setDepths(patch_i, subtract[i]) for i = 0 .. n - 1 with ok[i] != 0, IN THAT ORDER (src/hpmvs/Scene.cpp:351-381).
 * subtract[i] != 0 takes patch i's depths back: a cell that still holds exactly that patch's depth becomes MAX_DEPTH again
 * (:373-374) -- what CellProcessor::branch does for the patch of a leaf it splits before it enters the children's depths
 * (src/hpmvs/CellProcessor.cpp:276-279, 296).  Unlike the minimum of subtract = 0 that depends on the order of the calls that
 * reach a cell, so the batch is applied cell by cell in call order (sorted keys, one thread replays a cell's calls): the maps
 * are those of the sequential loop.  subtract == NULL: hpmvs_set_depths_batch.  n * max_images < 2^28 per call.  The call is
 * host-synchronous also with on_device = 1 (the number of keys is read back before the sort; its temporaries are freed on return).
 * hpmvs_level_support_batch: Scene::getLevelSupport(patch, min_level) (src/hpmvs/Scene.cpp:334-343), branch's first gate. */
int hpmvs_depth_ops_batch(hpmvs_scene *s, const hpmvs_patch_batch *b, const uint8_t *subtract, int on_device, void *stream);
int hpmvs_level_support_batch(const hpmvs_scene *s, const hpmvs_patch_batch *b, int min_level, int32_t *support, int on_device, void *stream);
/* The cells those calls touch, as integers: what a scheduler needs to run one priority level's candidates in conflict-free
 * waves and still end with the reference's SEQUENTIAL result (CellProcessor.cpp:130-142 reads maps that earlier candidates
 * of the same level have written, Scene.cpp:351-381; hpmvs_amd/frontier.py is that scheduler, INTEGRATION.md has the recipe).
 * Any output may be NULL.  Computed with the same device code as the gates / setDepths, so the cells are exact.
 *   writes     [n][max_images][4]  attached image k: view, level, x, y of the cell setDepths offers its depth to (view -1: none)
 *   frees      [n][max_images][4]  attached image k: view, level, x, y of the cell pixelFreeTest reads (view -1: none)
 *   attached   [n][max_images][3]  attached image k: view, ix0, iy0 -- depthTests reads getFullDepth of the 3x3 level-0 pixel
 *                                  block from (ix0, iy0): cell ((int)(px / 2.0) >> l, (int)(py / 2.0) >> l) of every level l
 *   view_block [n][n_views][3]     every view v: 1 if viewBlockTest examines it, ix0, iy0 of its 3x3 block (read the same way) */
int hpmvs_depth_footprints_batch(const hpmvs_scene *s, const hpmvs_patch_batch *b, int32_t *writes, int32_t *frees,
                                 int32_t *attached, int32_t *view_block, int on_device, void *stream);
/* The conflict graph of one extend level, made on the device from those footprints: what the wave walk of a level needs and
 * nothing else (hpmvs_amd/csrc/conflicts.hpp states the cells and has the host restatement).  Nodes are the
 * batch's patches in queue order; is_event[i] != 0 marks a subtraction event (writes, NO reads; NULL: all candidates).
 *   flow[i], i a candidate: nodes j < i of either kind that write a cell i reads
 *   flow[i], i an event:    candidates j < i that write a cell i writes
 *   anti[i], i a candidate: candidates j < i that read a cell i writes, and events j < i that write a cell i writes
 *   anti[i], i an event:    candidates j < i that read a cell i writes
 * A read block from (ix0, iy0) covers the cells x0 >> (1 + l) .. x1 >> (1 + l), x1 = ix0 + 2, x0 = max(ix0, 0), of every level
 * l < n_levels (likewise y; none when x1 < 0 or y1 < 0); a pixelFreeTests read is its one cell.  Ignored: entries with view < 0 or
 * view >= n_views, writes / frees on a level outside [0, n_levels), cells or blocks beyond 2^24 (no map has them).  No edge
 * between two events, no node its own neighbour.
 * Output: CSR, *_off[n + 1] and *_adj, every list ascending without duplicates -- one byte string per input.  The offsets and the
 * totals *n_flow / *n_anti (HOST words in both forms) are always written; the adjacency arrays only when cap_flow >= *n_flow and
 * cap_anti >= *n_anti (entries), else HPMVS_ERR_ARG with "capacity" in hpmvs_last_error and the totals valid: allocate and call
 * again (an adjacency array may be NULL with capacity 0).  n == 0, nodes without images and is_event == NULL are valid.
 * HPMVS_ERR_ARG before any write for n_levels outside 1 .. HPMVS_MAX_LEVELS, max_images outside 1 .. HPMVS_MAX_IMAGES, n_views
 * outside 1 .. 8191, n * max_images >= 2^28 and null arrays; HPMVS_ERR_STATE before any output when more than 2^30 (reader, writer)
 * pairs meet before duplicates are dropped (every node on one cell; counted by key-range bounds, a node's own writes included, so
 * such an input is refused without a walk over its pairs).  Host-synchronous also with on_device = 1 (three counts are
 * read back on the way; the scratch is freed on return).
 * hpmvs_level_conflicts_batch runs the footprint kernel into scratch of its own -- no footprint leaves the device -- with
 * n_levels = the deepest pyramid of the scene's cameras.  hpmvs_conflicts_from_footprints takes footprint arrays in the layouts
 * above (host or device pointers; n_images[n]: the entries of a row that count) and needs no scene. */
int hpmvs_level_conflicts_batch(const hpmvs_scene *s, const hpmvs_patch_batch *b, const uint8_t *is_event, uint32_t *flow_off,
                                uint32_t *flow_adj, size_t cap_flow, uint32_t *anti_off, uint32_t *anti_adj, size_t cap_anti,
                                uint32_t *n_flow, uint32_t *n_anti, int on_device, void *stream);
int hpmvs_conflicts_from_footprints(int device, int n, int max_images, int n_views, int n_levels, const int32_t *n_images,
                                    const int32_t *writes, const int32_t *frees, const int32_t *attached, const int32_t *view_block,
                                    const uint8_t *is_event, uint32_t *flow_off, uint32_t *flow_adj, size_t cap_flow,
                                    uint32_t *anti_off, uint32_t *anti_adj, size_t cap_anti, uint32_t *n_flow, uint32_t *n_anti,
                                    int on_device, void *stream);
/* The WAVE WALK of one extend level -- what strings the candidates, the graph, the gates and the ordered depth update into the
 * result of CellProcessor::extend run over the level's leaves one after the other -- as ONE call, entirely on the device
 * (hpmvs_amd/csrc/level_walk.hpp states the rule and has the host restatement; INTEGRATION.md has the recipe).
 * `items`: the level's queue, n rows in the reference's order -- a subtraction event's patch (the patches CellProcessor::filter
 * removed from a cell, right before that cell's candidates), a candidate's refined patch; the rows of candidates that were not
 * refined are not read.  flags[i]: HPMVS_WALK_EVENT, or for a candidate any of HPMVS_WALK_REFINED (it was refined: stage 0 of the
 * candidate call, and not skipped), _BORDER (refined and outside its tree's root), _HAS_PRE (pre_key[i] is a leaf: the pre_inside of
 * the candidate calls; the grid always), _PRE_TAKEN / _POST_TAKEN (that leaf is nonempty, or refused, when the level starts).
 * set[i] (NULL: one set): the tree the keys of candidate i belong to -- keys are equal only within one set; >= 0.  pre_key /
 * post_key: the leaf of the candidate before and after refinement (post_key is read for a refined candidate that is not border).
 * stage (in / out): preset to each candidate's refinement result, an accepted candidate's becomes 0, a rejected one's 20 (its
 * leaf was taken), 23 / 24 / 25 (depthTests / viewBlockTest / pixelFreeTests), 26 (the refined patch's leaf was taken) or 27
 * (border: every gate passed, handed to the scheduler); an event's is not written.  counts [n][3]: the three counts at decision
 * time, -1 where never counted.  accepted[i]: 1 for an accepted candidate, whose depths are in the maps on return, as the
 * subtractions of every event are.  wave[i]: the wave (1-based) that decided item i; *n_waves (a HOST word in both forms): their
 * number -- the items still deferred after wave w are those with wave[i] > w.
 * Inside: the conflict graph over the events and the refined candidates by the device code of hpmvs_level_conflicts_batch; the
 * candidates' key records, sorted once; then per wave the gates over the pending refined candidates against the maps as they stand,
 * resolve ROUNDS -- an item decides once no earlier item it shares a map cell or a leaf key with, and that can still change its
 * outcome, is undecided; the last few of a wave are decided by one wavefront in order -- and one ordered depth update (the kernels of
 * hpmvs_set_depths_batch when the wave holds additions only, else those of hpmvs_depth_ops_batch).  Rounds and waves are kernel
 * launches; the host reads a count after each and takes no decision.
 * HPMVS_ERR_ARG before any output byte or map cell is written: null arrays, max_images outside 1 .. HPMVS_MAX_IMAGES, a flag byte
 * that cannot occur (an event that is refined or border, a bit that is none of the above), a negative set, and whatever
 * hpmvs_level_conflicts_batch refuses.  HPMVS_ERR_STATE before any map write: a scene without depth maps (or with 2^32 cells or
 * more), the graph's 2^30-pair refusal -- the caller then walks on the host.  n == 0, only events and only unrefined candidates are
 * valid.  Host-synchronous in both pointer forms.  hpmvs_last_level_walk: the rounds of the last call on this scene, the most
 * rounds of one wave and the in-order passes (any may be NULL). */
#define HPMVS_WALK_EVENT 1
#define HPMVS_WALK_REFINED 2
#define HPMVS_WALK_BORDER 4
#define HPMVS_WALK_HAS_PRE 8
#define HPMVS_WALK_PRE_TAKEN 16
#define HPMVS_WALK_POST_TAKEN 32
int hpmvs_level_walk_batch(hpmvs_scene *s, const hpmvs_options *o, const hpmvs_patch_batch *items, const uint8_t *flags,
                           const int32_t *set, const uint64_t *pre_key, const uint64_t *post_key, float margin, int abs_int,
                           int32_t *stage, int32_t *counts, uint8_t *accepted, int32_t *wave, int32_t *n_waves, int on_device,
                           void *stream);
int hpmvs_last_level_walk(const hpmvs_scene *s, int32_t *rounds, int32_t *most_rounds, int32_t *in_order_passes);

/* ---- CellProcessor::regularize for a priority level (src/hpmvs/CellProcessor.cpp:309-367, processCell :369-420) ----------------
 * The octree stays the scheduler's.  For each call it passes a VERSIONED snapshot of the nonempty leaves: a leaf is part of the
 * tree at queue positions born < q < died (leaves present when the sweep starts: born = -1, died = INT32_MAX; a leaf the sweep
 * removes or splits at position s: died = s; a leaf that split creates: born = s).  root_* is the Branch the CellProcessor walks
 * (a subtree's root when the model is split).  Every leaf's path is re-derived from the root with the reference's recurrences
 * (Cell(parent, idx), doctree.cpp:30-36; Branch::at, doctree.h:250-255); a leaf whose recomputed centre is not bit-equal to
 * cell_center, or that lies deeper than HPMVS_MAX_TREE_DEPTH levels, makes the call fail with HPMVS_ERR_ARG before any output
 * is written. */
#define HPMVS_MAX_TREE_DEPTH 21
#define HPMVS_REGULARIZE_PROBES 24
typedef struct {
    int32_t n;                  /* nonempty leaves */
    float root_center[3];       /* Cell::c_ of the root Branch */
    float root_width;           /* its width_ */
    const float *cell_center;   /* [n][3] Leaf::c_ */
    const float *cell_width;    /* [n]    Leaf::width_ */
    const float *patch_center;  /* [n][3] data[0]->center_ (x, y, z) */
    const int32_t *born;        /* [n] */
    const int32_t *died;        /* [n] */
} hpmvs_leaf_table;
/* regularize(cell) for every cell of `cells` (center, normal, n_images, images[.][0] are read): cell_width[n] = its leaf's width_,
 * position[n] = its queue position q, expanded[n] = expanded_.  flatness[n] is in/out: an unexpanded cell keeps its value
 * (regularize returns at once) and gets n_neighbours = -1; otherwise flatness = 2.6 (no neighbour leaf), 2.5 (fewer than 4) or
 * the RMS plane distance / width, and n_neighbours = the distinct nonempty leaves the 24 probes found at q (the cell's own leaf
 * counts when a probe lands in it).  neighbour_leaf (nullable): [n][24] those leaves' table indices in first-probe order
 * (yy outer, xx inner), -1 padded.  The RMS sum runs in that order; the reference sums in std::set<Leaf*> (heap-address)
 * order, so flatness may differ from a given reference run by the rounding of at most 23 float additions.
 * HPMVS_ERR_ARG also for an expanded cell whose reference image is not a view of the scene.  Host or device pointers (leaf
 * table included) as for hpmvs_optimize_batch; the call is host-synchronous once (leaf checks) and then only enqueues when
 * on_device != 0. */
int hpmvs_regularize_batch(const hpmvs_scene *s, const hpmvs_patch_batch *cells, const float *cell_width, const int32_t *position,
                           const uint8_t *expanded, const hpmvs_leaf_table *leaves, float *flatness, int32_t *n_neighbours,
                           int32_t *neighbour_leaf, int on_device, void *stream);

/* ---- CellProcessor::filter for a priority level (src/hpmvs/CellProcessor.cpp:43-82, processCell :377-378) ------------------------
 * The rows of `patches` (center and normal are read) are the cells' patches in data order, the cells in the scheduler's order:
 * cell c holds rows cell_start[c] .. cell_start[c + 1] - 1.  For a cell of k >= 2 patches, dist[r] is the reference's float for
 * row r: (sum over the other rows jj, in order, of normalized(normal_r) . (center_jj - center_r)) / (float)(k - 1), signed; 0
 * for the rows of single-patch cells.  keep[c] is the row of the patch filter keeps -- the lowest row reaching the minimum among
 * the cell's distances < FLT_MAX (NaN and +inf never win) --, the cell's row for a single patch, -1 for an empty cell and -2
 * for a cell with no distance below FLT_MAX (the reference would keep a null pointer there).  The other rows of a cell are
 * its losers: the caller takes their depths back (hpmvs_depth_ops_batch, subtract = 1, in queue order) and clears their image
 * lists.  HPMVS_ERR_ARG before any output is written when a count is negative, cell_start[0] != 0, the offsets decrease or
 * cell_start[n_cells] != patches->n (with device pointers the offsets are checked by a small kernel whose verdict the call
 * reads back first).  Host or device pointers as for hpmvs_optimize_batch; host-synchronous once, then only enqueues when
 * on_device != 0. */
int hpmvs_filter_batch(const hpmvs_scene *s, const hpmvs_patch_batch *patches, const int32_t *cell_start, int n_cells, float *dist,
                       int32_t *keep, int on_device, void *stream);

/* ---- the seed octree: the second half of Scene::initPatches (src/hpmvs/Scene.cpp:183-199) -------------------------------------
 * For the rows of `b` with ok[i] != 0 (every row when ok is NULL), in row order -- the survivors of hpmvs_init_patches_batch --:
 * getBoundingBox (doctree.h:732-756: max starts at FLT_MIN, a NaN coordinate never enters), the root Branch((min + max) / 2,
 * max(dist)), scale = max(scale, width / (1 << PATCH_INIT_MAXLEVEL + 1)) written back to b->scale, and the octree the sequential
 * loop patchTree_.add(p, scale) leaves behind, as the tables the level calls read:
 *   rows         [n]      the n_rows rows, leaf by leaf in Leaf_iterator order, in data order (= row order) within a leaf
 *   cell_start   [n + 1]  leaf l holds rows[cell_start[l] .. cell_start[l + 1] - 1]; cell_start[n_leaves] = n_rows
 *   cell_center  [n][3]   Leaf::c_, by the reference's Cell(parent, idx) descent (hpmvs_regularize_batch accepts it bit for bit)
 *   cell_width   [n]      Leaf::width_
 *   cell_level   [n]      the leaf's depth below the root (nodeLevel), >= 1: the root is a Branch
 *   patch_center [n][3]   data[0]->center_ (nullable)
 * Entries from n_rows / n_leaves on come back 0.  The tree is computed in closed form (add only ever splits: DESIGN.md §3.10) and
 * equals the sequential insertion's leaf for leaf; insertion order is row order (the reference's is whatever order its OpenMP
 * threads reach the critical section in).  set_depths != 0 then runs setDepths(p, false) for the same rows (needs
 * hpmvs_scene_depth_reset, and the batch's normal / n_images / images, which are not read otherwise).  No row: the reference's
 * unit cube (centre 0, width 2), n_leaves = 0.
 * HPMVS_ERR_ARG before any write for patch_init_maxlevel outside 0 .. HPMVS_MAX_TREE_DEPTH, for a bounding box that is not finite
 * (the reference would carry on with it) and for set_depths on a scene without depth maps.  A root width so small that its
 * halvings are subnormal is cut off at HPMVS_MAX_TREE_DEPTH levels.  Host or device pointers as for hpmvs_optimize_batch (info is
 * always a host structure); the call is host-synchronous in both forms: the record with the counts is read back once, and its
 * temporaries (O(n)) are freed on return. */
typedef struct {
    float root_center[3];
    float root_width;
    float scale_floor;
    int32_t n_rows;     /* rows with ok != 0 */
    int32_t n_leaves;   /* nonempty leaves */
} hpmvs_seed_tree_info;
int hpmvs_seed_tree_batch(hpmvs_scene *s, hpmvs_patch_batch *b, int patch_init_maxlevel, int set_depths,
                          hpmvs_seed_tree_info *info, int32_t *rows /*[n]*/, int32_t *cell_start /*[n+1]*/,
                          float *cell_center /*[n][3]*/, float *cell_width /*[n]*/, int32_t *cell_level /*[n]*/,
                          float *patch_center /*[n][3], nullable*/, int on_device, void *stream);

/* The scheduler's octree as CellProcessor::extend consults it (reference src/hpmvs/CellProcessor.cpp:122-125, 147-154): for every
 * point the leaf root->at(p) of any depth, getRoot()->contains(p) and the leaf DynOctTree::addConditional(p, add_width) would put
 * it in (include/hpmvs/doctree.h:250-255, 397-419; src/hpmvs/doctree.cpp:30-42).  The tree is given as PATH KEYS: a sentinel bit,
 * then 3 bits per level (z y x, a bit set where p > c_), the root being 1; at most HPMVS_MAX_TREE_DEPTH levels.  branch_key: every
 * Branch below the root (the root, or a subtree's root, is implicit); leaf_key: the NONEMPTY leaves.  An empty leaf is a key in
 * neither set below a branch; the empty tree (no key at all) has eight empty leaves at depth 1.  Centres and widths follow from
 * the root by Cell(parent, idx) (double arithmetic, float storage).
 *   inside[i]       root.contains(points[i])  (a point outside still descends to a leaf, as Branch::at does; a NaN coordinate
 *                   takes child bit 0)
 *   leaf_key[i]     key of the located leaf;  leaf_index[i]  its index in t->leaf_key, -1 for an empty leaf
 *   leaf_width[i], leaf_center[i]             its width_ / c_
 *   target_key[i]   0 when addConditional(points[i], add_width[i]) refuses (nonempty leaf, or leaf width < add_width), else the
 *                   key of the leaf reached by splitting while width / 2.0 > add_width (cut off at HPMVS_MAX_TREE_DEPTH levels,
 *                   where the reference would go on splitting); 0 everywhere without add_width
 * Every output is nullable.  n = 0 and an empty tree are valid.  HPMVS_ERR_ARG before any output is written when the keys are no
 * tree: a word that is no key of a cell below the root, a leaf deeper than HPMVS_MAX_TREE_DEPTH levels or a branch deeper than
 * HPMVS_MAX_TREE_DEPTH - 1, a key that occurs twice (in one array or in both), a key whose parent prefix is neither a branch nor the
 * root; also for a root that is not finite or has no positive width.  (Whether the branches' other children are complete is not
 * the table's business: what is in neither set is an empty leaf.)  The look-up table is built in a launch workspace of the scene
 * (12 bytes per slot, 2 x keys slots); host or device pointers as for hpmvs_optimize_batch (t is always a host structure, its
 * key arrays follow on_device).  The call is host-synchronous in both forms up to the table's verdict. */
typedef struct {
    float root_center[3];
    float root_width;
    int32_t n_branches;
    int32_t n_leaves;
    const uint64_t *branch_key;   /* [n_branches] */
    const uint64_t *leaf_key;     /* [n_leaves] */
} hpmvs_octree_index;
int hpmvs_octree_locate_batch(const hpmvs_scene *s, const hpmvs_octree_index *t, int n, const float *points /*[n][3]*/,
                              const float *add_width /*[n], nullable*/, uint8_t *inside /*[n]*/, uint64_t *leaf_key /*[n]*/,
                              int32_t *leaf_index /*[n]*/, float *leaf_width /*[n]*/, float *leaf_center /*[n][3]*/,
                              uint64_t *target_key /*[n]*/, int on_device, void *stream);

/* The candidate steps of one extend level against the real octree, in ONE call (reference src/hpmvs/CellProcessor.cpp:84-178): the
 * six candidates of every parent are built, looked up in the tree t (:122-125), those the tree does not pre-gate are refined and
 * gated (:127-133), and the refined ones are looked up again (:147-154).  The call equals HPMVS_EXPAND_EXTEND of
 * hpmvs_expand_batch with cell_center = 0, cell_width = width for every parent and the skip bytes computed on the device, and it
 * returns the keys of both look-ups; `out` and the keys are byte-identical to the composition hpmvs_expand_batch (everything
 * skipped) -> hpmvs_octree_locate_batch -> hpmvs_expand_batch (skip) -> hpmvs_octree_locate_batch at add_width.
 *   width        the leaf width of the level: an exact level width of the tree (root_width halved d >= 1 times, each time in
 *                double and narrowed to float).  addConditional's width is (float)((double)width * 0.9), so every target below
 *                lies at that depth d.
 *   skip[t]      the tree's verdict whatever else stops the candidate: its centre before optimize lies inside the root, in a leaf
 *                that is nonempty or narrower than width.  Such a candidate is built, not refined, and ends at stage 20.
 *   pre_key[t]   for a centre inside the root the leaf addConditional would put it in, 0 where it refuses; 0 outside (a centre
 *                outside the root is never pre-gated and matches no leaf: test pre_inside, not the key)
 *   border[t]    the candidate was refined (out->ok[t] != 0) and its centre left the root: it goes to the border queue
 *   post_key[t]  refined and inside: addConditional's target leaf, 0 where it refuses; 0 for every other candidate
 * Every pointer of keys is nullable, and so is keys; what is given is written in every entry.  parents->n == 0 and the empty tree
 * are valid.  HPMVS_ERR_ARG before any output is written for what hpmvs_expand_batch refuses (a bad batch, out->n != 6 n), what
 * hpmvs_octree_locate_batch refuses (keys that are no tree, a bad root), and for a width that is not finite or no level width of
 * the tree.  The look-up table is built ONCE, in device memory of the call's own (12 bytes per slot, 2 x keys slots; a launch
 * workspace would be handed to the refinement between the two look-ups), allocated before and freed after the call like
 * hpmvs_octree_insert_batch's scratch; the call is host-synchronous in both pointer forms. */
typedef struct {            /* every pointer nullable; [6 * parents->n] each; follow on_device */
    uint8_t  *skip;         /* 1: pre-gated (CellProcessor.cpp:124): built, not refined, stage 20 */
    uint8_t  *pre_inside;   /* getRoot()->contains(centre before optimize) */
    uint64_t *pre_key;      /* inside: addConditional's target leaf at (float)(width * 0.9); else 0 */
    uint8_t  *border;       /* refined (ok != 0) and outside the root (:147) */
    uint64_t *post_key;     /* refined and inside: the target leaf, 0 = addConditional refuses; else 0 */
} hpmvs_extend_tree_keys;
int hpmvs_extend_tree_batch(const hpmvs_scene *s, const hpmvs_options *o, const hpmvs_octree_index *t,
                            const hpmvs_patch_batch *parents, float width, hpmvs_patch_batch *out,
                            const hpmvs_extend_tree_keys *keys, int on_device, void *stream);

/* The same for ALL subtrees of a partition in one call.  main() never runs a level on one tree: getSubTrees cuts patchTree_ into
 * at least --subtrees subtrees and every CellProcessor consults its own (reference src/main.cpp:50-96).  A forest is a list
 * of trees given as CONCATENATED key arrays -- tree k's branch keys are branch_key[branch_first[k] .. branch_first[k + 1] - 1],
 * likewise its nonempty leaves' -- every key relative to its own tree's root, in any order within a tree (hpmvs_octree_partition's
 * leaf_sub_key / branch_sub_key, grouped by tree).  parent_tree[i] names the tree parent i extends in.
 *   CONTRACT     for every tree k, take the parents with parent_tree[i] == k in their given order: the rows 6 i .. 6 i + 5 of `out`
 *                and of every key array are byte-identical to what hpmvs_extend_tree_batch returns for tree k alone with those
 *                parents.  The parents of different trees may be interleaved in any order; the returned keys are relative to the
 *                candidate's own tree.
 * One expand_init, one refinement launch and one expand_gate serve all trees, so a level of 100 subtrees costs one launch, one
 * key upload and one verdict, not 100.  n_trees == 0 with parents->n == 0, trees without keys (eight empty leaves), trees without
 * parents and parents->n == 0 are valid.  HPMVS_ERR_ARG before any output byte is written, with the offending tree's index in
 * hpmvs_last_error ("tree K"), for whatever hpmvs_extend_tree_batch refuses for a single tree (keys that are no tree, a bad root,
 * a bad batch), offsets that are not non-decreasing from 0, a parent_tree[i] outside [0, n_trees) (the message names parent i)
 * and a parent in a tree of which `width` is no level width.  A tree WITHOUT parents may have any root width: a subtree rooted
 * below the level is the normal case after getSubTrees.  When several trees offend, the lowest index is named.
 * The look-up tables share ONE buffer of the call's own, tree k owning a power-of-two slot range of it, so equal keys of
 * different trees never meet.  root / branch_first / leaf_first are HOST arrays in both forms, like an hpmvs_octree_index; the
 * key arrays and parent_tree follow on_device.  Host-synchronous in both forms; ONE read-back carries every verdict.
 * Border patches: a candidate that leaves ITS tree's root comes back with border[t] = 1 whichever other tree contains it; the
 * caller routes and inserts them between levels (hpmvs_octree_route_batch / hpmvs_octree_insert_batch), never between the
 * subtrees of one level. */
typedef struct {
    int32_t n_trees;
    const float    *root;          /* [n_trees][4]: c_ x y z, width_   -- HOST array in both forms */
    const int32_t  *branch_first;  /* [n_trees + 1]  HOST */
    const int32_t  *leaf_first;    /* [n_trees + 1]  HOST */
    const uint64_t *branch_key;    /* [branch_first[n_trees]]  follows on_device */
    const uint64_t *leaf_key;      /* [leaf_first[n_trees]]    follows on_device */
} hpmvs_octree_forest;
int hpmvs_extend_forest_batch(const hpmvs_scene *s, const hpmvs_options *o, const hpmvs_octree_forest *f,
                              const hpmvs_patch_batch *parents, const int32_t *parent_tree /*[parents->n], follows on_device*/,
                              float width, hpmvs_patch_batch *out, const hpmvs_extend_tree_keys *keys, int on_device, void *stream);

/* The other two priorities of processCell -- L*10+1 regularize, L*10+2 removal or branch (reference CellProcessor.cpp:309-420) --
 * as ONE sweep over expanded cells of mixed flatness_, for all subtrees of a forest, in queue order (queue position = row index).
 * The tree is the key sets of hpmvs_extend_forest_batch: no cell centres travel, every leaf's Cell comes from its key.
 *   cells[i]             data[0] of cell i; cell_tree[i] its tree, cell_key[i] the key of its (nonempty) leaf in that tree
 *   leaf_patch_center    [leaf_first[n_trees]][3]: data[0]->center_ of every nonempty leaf, in leaf_key order
 *   flatness[i] < 0      the cell is REGULARIZED at position i (NaN is not < 0): 24 probes descend from its own tree's root, the
 *                        distinct nonempty leaves give 2.6 / 2.5 / RMS plane distance over width_, summed in first-probe order.
 *                        The tree a probe sees is the tree as it stands at position i: a leaf an earlier cell of the same tree
 *                        removed is empty, a leaf an earlier cell split is a branch -- one more octant step finds the child leaf
 *                        (data[0]: the first child in k order that went into that octant, at its refined centre) or an empty one
 *   any other cell       is SETTLED: (double)flatness > 2.4 removes the patch (setDepths(p, true), the leaf emptied), else
 *                        CellProcessor::branch: getLevelSupport(p, MINLEVEL) < 1 ends it, else the four diagonal children as
 *                        hpmvs_expand_batch(HPMVS_EXPAND_BRANCH) makes them in Cell(parent, idx) of the key.
 *                        split = !removed && support >= 1 && !(final_level && no child survived)
 *   depth maps           ONE ordered setDepths replay for the sweep, in row order across all trees: a removed cell's patch with
 *                        subtract; a split cell's patch with subtract, then its surviving children in k order
 * The sweep is the sequential loop over the rows as given, each cell acting in its own tree and all on the shared maps; cells of
 * different trees may be interleaved.  The tree is NOT modified: the caller applies removals and splits.
 * Outputs (every pointer of the result nullable, every entry written, all follow on_device): `out` (4 n rows) is what
 * hpmvs_expand_batch(BRANCH) returns with skip = 1 for the rows of every regularized, removed or support < 1 cell; child_key is
 * (cell_key << 3) | octant of the leaf child k went into (0: none; two children may share a key, the leaf's data[0] is the lower
 * k); n_neighbours is -2 for settled cells; neighbour_key holds the neighbours' keys in the cell's tree, first-probe order,
 * 0-padded.  flatness is in/out: updated for regularized cells only.
 * HPMVS_ERR_ARG before any output byte or map cell is written, the lowest offender named in hpmvs_last_error: whatever
 * hpmvs_extend_forest_batch refuses for the forest ("tree K"); a cell_tree[i] outside the forest, a cell_key[i] that is no
 * nonempty leaf of its tree, the same (tree, key) twice, a cell at depth HPMVS_MAX_TREE_DEPTH that would go to branch, a
 * regularized cell whose reference image is no view ("cell i"); out->n != 4 n, a max_images mismatch, 5 n * max_images >= 2^28.
 * A scene without depth maps: HPMVS_ERR_STATE, as hpmvs_depth_ops_batch.  n == 0, trees without cells, all cells regularized (no
 * refinement launch, no depth ops) and all settled are valid.  Host-synchronous in BOTH pointer forms: the tables, the op rows
 * and the sort's temporaries are the call's own and are freed when it returns. */
typedef struct {
    int32_t  *support;        /* [n] getLevelSupport(p, MINLEVEL) of every row */
    uint8_t  *removed;        /* [n] */
    uint8_t  *split;          /* [n] */
    uint8_t  *children;       /* [n][4] the children that go into the new leaves */
    uint64_t *child_key;      /* [n][4] */
    int32_t  *n_neighbours;   /* [n] */
    uint64_t *neighbour_key;  /* [n][24] */
} hpmvs_process_forest_result;
int hpmvs_process_forest_batch(hpmvs_scene *s, const hpmvs_options *o, const hpmvs_octree_forest *f, const float *leaf_patch_center,
                               const hpmvs_patch_batch *cells, const int32_t *cell_tree, const uint64_t *cell_key, float *flatness,
                               const uint8_t *final_level, hpmvs_patch_batch *out, const hpmvs_process_forest_result *res,
                               int on_device, void *stream);

/* A round's border patches (reference src/hpmvs/CellProcessor.cpp:487-540): candidates of CellProcessor::extend that passed every
 * gate but left their subtree's root.  distributeBorderCell hands each to the first processor whose root contains it;
 * processBorderCellQueue inserts them, in queue order, with addConditional(p, scale * 2.0).
 *
 * hpmvs_octree_insert_batch is that loop for one tree: addConditional(points[i], add_width[i]) for i = 0 .. n - 1 IN THAT ORDER,
 * every patch seeing the leaves the earlier ones created (the widths differ per patch, so an earlier insertion can leave a later
 * point a nonempty leaf, a leaf that has become too narrow, or a deeper leaf to start from).  The tree t is the caller's and is
 * NOT modified: the caller enters the accepted keys (the branches on the way are their proper prefixes).
 *   accepted[i]   1 when the patch was inserted
 *   leaf_key[i]   *outleaf: the key of the leaf the patch went into, or of the leaf that refused it (the located leaf of t when t
 *                 itself refuses -- nonempty, or narrower than add_width[i] --, else the leaf the earlier insertions left there)
 *   blocker[i]    -1 for an accepted patch and for a refusal by t itself; else the queue index of the earlier patch behind the
 *                 refusal: the owner of the nonempty leaf, or for a leaf that has become too narrow the accepted patch whose key
 *                 shares the longest prefix with the point's path (the lowest index among equals).  Nullable.
 * Splitting stops at HPMVS_MAX_TREE_DEPTH levels as for target_key above.  The comparisons are the reference's as written: a NaN
 * add_width refuses nothing and splits nothing, the patch goes into the leaf it finds.  n = 0 and the empty tree are valid; the
 * table is checked as for hpmvs_octree_locate_batch (HPMVS_ERR_ARG before any output is written).  Scratch of 44 n bytes plus the
 * sort's is the call's own; the call is host-synchronous in both forms.
 *
 * hpmvs_octree_route_batch: tree[i] = the first t in list order whose root (roots[t]: c_ x y z, width_) contains points[i]
 * (Cell::contains), -1 when none does (distributeBorderCell drops such a patch).  roots is a HOST array in both forms, like an
 * hpmvs_octree_index; a root that is not finite or has no positive width is HPMVS_ERR_ARG.  n = 0 and n_trees = 0 are valid. */
int hpmvs_octree_insert_batch(const hpmvs_scene *s, const hpmvs_octree_index *t, int n, const float *points /*[n][3]*/,
                              const float *add_width /*[n]*/, uint8_t *accepted /*[n]*/, uint64_t *leaf_key /*[n]*/,
                              int32_t *blocker /*[n], nullable*/, int on_device, void *stream);
int hpmvs_octree_route_batch(const hpmvs_scene *s, int n_trees, const float *roots /*[n_trees][4]: c_, width_*/, int n,
                             const float *points /*[n][3]*/, int32_t *tree /*[n]*/, int on_device, void *stream);

/* The same delivery for a whole round's border queue and ALL subtrees in ONE call: distributeBorderCell, every subtree's
 * processBorderCellQueue and the accepted patches' setDepths(p, false).  `border` is the queue in push order; the call reads
 * center and scale, with set_depths != 0 also normal, n_images and images; ok is neither read nor written and the batch is not
 * modified.  add_width[i] = (float)((double)scale[i] * 2.0) is formed on the device.
 *   CONTRACT     tree[] equals hpmvs_octree_route_batch over f->root.  For every tree k, take the rows with tree[i] == k in their
 *                given order: accepted and leaf_key of those rows are byte-identical to hpmvs_octree_insert_batch on tree k alone
 *                with those rows, and blocker is that call's blocker mapped back through the row selection (an index into THIS
 *                queue).  A row no root contains is dropped: tree -1, accepted 0, leaf_key 0, blocker -1.  With set_depths != 0
 *                the maps end as after hpmvs_set_depths_batch over the accepted rows (a float minimum: order plays no part).
 * The forest is NOT modified: the caller enters the accepted keys.  The rows of different trees may be interleaved in any order,
 * and two trees may hold the same sub-key: a run of the replay is a (tree, leaf key) pair.  root / branch_first / leaf_first are
 * HOST arrays in both forms; the key arrays, the batch and the result follow on_device.  Every pointer of the result is nullable,
 * and so is the result; what is given is written in every entry.  n == 0, n_trees == 0 (every tree is -1), trees without keys and
 * trees no patch reaches are valid.  HPMVS_ERR_ARG before any output byte or map cell is written, the lowest offender named, for
 * whatever hpmvs_extend_forest_batch refuses for the forest ("tree K") and for a bad batch; HPMVS_ERR_STATE, likewise before any
 * write, for set_depths on a scene without depth maps.  The tables and 56 bytes per patch plus the sorts' temporary storage are the
 * call's own; no allocation and no launch size depends on data read back.  Host-synchronous in both pointer forms. */
typedef struct {             /* every pointer nullable; [border->n] each; follow on_device */
    int32_t  *tree;          /* first tree in list order whose root contains center_, -1: none (the patch is dropped) */
    uint8_t  *accepted;      /* 1: inserted */
    uint64_t *leaf_key;      /* key IN THAT TREE of the leaf it went into / that refused it; 0 where tree == -1 */
    int32_t  *blocker;       /* as hpmvs_octree_insert_batch, as an index into THIS queue; -1 where tree == -1 */
} hpmvs_border_forest_result;
int hpmvs_border_forest_batch(hpmvs_scene *s, const hpmvs_octree_forest *f, const hpmvs_patch_batch *border,
                              int set_depths, const hpmvs_border_forest_result *res, int on_device, void *stream);

/* The split of the octree into subtrees that main() makes between initPatches and the first level (reference src/main.cpp:50-96,
 * getSubTrees(scene.patchTree_, subTrees, FLAGS_subtrees); DynOctTree::getSubTrees, doctree.h:513-523; Branch::nrLeafs,
 * doctree.h:236-247), and DynOctTree::cellHistogram (doctree.h:493-511), for a tree given as path keys:
 *   min_trees < 2      the list is the root alone (root_key[0] = 1): every key lies in tree 0 under its own key, no orphans
 *   else               a first split, whatever the tree holds: the BRANCH children of the root in child order 0 .. 7, empty
 *                      ones included; a child that is a LEAF enters no subtree.  Then, while the list is shorter than
 *                      min_trees: nrLeafs (NONEMPTY leaves) of every entry, the FIRST entry with the largest count; the loop
 *                      ends when that count is below min_split_leaves (also on an empty list); else that entry's BRANCH children
 *                      in child order come first in the new list, then all other entries in their old order.
 * min_split_leaves is the reference's constant 100 (main.cpp:78); smaller values let small trees go through the loop.
 *   info               n_trees; n_orphans: nonempty leaves in no subtree (they stay in the tree and in its PLY files, but no
 *                      CellProcessor ever sees them: reference behaviour); n_splits; stop; histogram
 *   root_key[k]        the roots in the reference's list order -- the order distributeBorderCell searches and
 *                      hpmvs_octree_route_batch takes; root_cell[k]: c_ x y z, width_ by the chain Cell(parent, idx).  A
 *                      subtree's rootLevel_ is the depth of its root_key
 *   leaf_order         indices into t->leaf_key in Leaf_iterator order (children 0 .. 7, depth first); the nonempty leaves of
 *                      subtree k are leaf_order[tree_first[k] .. tree_first[k] + tree_leaves[k] - 1], in the order initFromTree
 *                      (CellProcessor.cpp:422-455) pushes them
 *   leaf_tree[i]       the subtree whose root is a PROPER ancestor of t->leaf_key[i], -1 for an orphan; leaf_sub_key[i]: the key
 *                      re-based on that root (the sentinel, then the bits below the root's depth), 0 where the tree is -1
 *   branch_tree[j],    the same for t->branch_key[j]: a root itself and the branches above the roots are -1 / 0
 *   branch_sub_key[j]
 * cap = max(8, min_trees + 6): the list cannot end longer; entries from n_trees on come back 0.  Every array output is nullable;
 * info is always a host structure.  The key arrays may be in ANY order, as for hpmvs_octree_locate_batch, and are checked as
 * there: HPMVS_ERR_ARG before any output is written for keys that are no tree, a root that is not finite or has no positive
 * width, min_trees > HPMVS_MAX_SUBTREES and min_split_leaves < 1.  The empty tree is valid (min_trees >= 2: no subtree at all).
 * The list is cut by ONE wavefront with the list in LDS (kernel_octree_partition.hip); scratch of 24 n_leaves bytes plus the
 * sort's and at most 192 KB for the roots is the call's own.  Host or device pointers as for the other octree calls; the call is
 * host-synchronous in both forms, and the only read-back besides the table's verdict is the info record. */
#define HPMVS_MAX_SUBTREES 4096
typedef struct {
    int32_t n_trees;
    int32_t n_orphans;     /* nonempty leaves in no subtree */
    int32_t n_splits;      /* iterations of the while loop that cut a subtree */
    int32_t stop;          /* 0: min_trees < 2, the root alone; 1: the list reached min_trees; 2: the largest subtree is below
                              min_split_leaves (or the list is empty) */
    int32_t histogram[HPMVS_MAX_TREE_DEPTH + 1];   /* cellHistogram: nonempty leaves by depth below t's root */
} hpmvs_octree_partition_info;
int hpmvs_octree_partition(const hpmvs_scene *s, const hpmvs_octree_index *t, int min_trees, int min_split_leaves,
                           hpmvs_octree_partition_info *info,
                           uint64_t *root_key      /*[cap]*/,  float *root_cell /*[cap][4]: c_, width_*/,
                           int32_t *tree_first     /*[cap]*/,  int32_t *tree_leaves /*[cap]*/,
                           int32_t *leaf_order     /*[n_leaves]: indices into t->leaf_key in Leaf_iterator order*/,
                           int32_t *leaf_tree      /*[n_leaves]*/,   uint64_t *leaf_sub_key   /*[n_leaves]*/,
                           int32_t *branch_tree    /*[n_branches]*/, uint64_t *branch_sub_key /*[n_branches]*/,
                           int on_device, void *stream);

/* Host-pointer calls and pinned memory.  An array of a host-pointer call (on_device = 0) that lies in pinned host memory
 * mapped into the GPU's address space -- hipHostMalloc / hipHostRegister, torch's pin_memory(), hpmvs_host_alloc below --
 * is used IN PLACE: the kernels read a patch's inputs once and write its outputs once, so they travel over PCIe while the
 * kernel runs; pageable arrays are copied through device buffers as before, array by array.  Results are identical either
 * way (outputs the kernel does not write for a failed patch -- color, ncc -- read 0, as after a staged call).  The
 * reference has no counterpart: its patches live in host containers (Scene.cpp:94-96, CellProcessor.cpp:129).
 * HPMVS_ZERO_COPY=0 in the environment switches the detection off.
 * ON AN INFRASTRUCTURE ERROR (negative status: a HIP error while enqueueing, no workspace) the two forms differ: a staged
 * call leaves the caller's arrays untouched, an in-place call may already have refined some patches in place (center,
 * normal, n_images, images) and zero-filled color / ncc -- treat the in/out arrays of a pinned batch as undefined after a
 * negative status and rebuild them.  Argument errors (HPMVS_ERR_ARG / _STATE) are detected before the first write in
 * both forms.  Per-patch failure (ok[i] == 0) is not an error and leaves that patch untouched in both forms. */
void *hpmvs_host_alloc(size_t bytes);   /* NULL on failure */
void hpmvs_host_free(void *p);
/* of the last host-pointer hpmvs_optimize_batch call above the small-batch thresholds: bytes copied through device
 * buffers and bytes used in place */
int hpmvs_last_staging(const hpmvs_scene *s, unsigned long long *staged_bytes, unsigned long long *in_place_bytes);

/* last optimize launch: kernel time measured with HIP events on the launch stream (ms).  Meaningful with ONE caller at a
 * time: the scene holds a single event pair, so concurrent launches from several host threads can pair the start of one
 * launch with the end of another. */
int hpmvs_last_kernel_ms(const hpmvs_scene *s, float *ms);
/* How many patches of the last refinement launch outgrew the batch kernel's HPMVS_FAST_IMAGES-id rows and were redone by the
 * wide kernel behind it (synchronises the device). */
int hpmvs_last_wide_patches(const hpmvs_scene *s, int32_t *n);

/* ---- multi-GPU: the per-round exchange of refined patches ---------------------------------------------------------
 * Patches are independent (PatchOptimizer.cpp:78-103 reads only its patch and the immutable scene; the reference
 * runs them as an OpenMP loop, Scene.cpp:94-96,114), so every rank (one process per GPU, scene replicated)
 * refines a contiguous slice of the round's batch and the only exchange is ONE all-gather of fixed-size records,
 * after which every rank holds the whole refined set for its host scheduler (main.cpp:145-181: one barrier per
 * priority level).  These entry points make that reachable from a C/C++ host without Python:
 *   hpmvs_pack_records       SoA batch (device arrays) -> n records (device), one kernel on `stream`
 *   hpmvs_allgather_records  ncclAllGather of `count` records per rank over the caller's RCCL communicator
 *                            (xGMI inside a node); RCCL is looked up at run time in the process (the library the
 *                            communicator came from), else librccl.so.1 is opened -- no link-time dependency;
 *                            $HPMVS_RCCL_LIBRARY names another library to take it from.  HPMVS_ERR_STATE when
 *                            none is found; HPMVS_ERR_ARG for a null communicator, for host pointers and for
 *                            send / recv buffers on two different devices (checked before the collective starts)
 *   hpmvs_unpack_records     records (device) -> SoA batch (device arrays); ok / color / fmin included
 * Ragged rounds (n not divisible by the ranks): pad every rank to the largest slice, records beyond a rank's
 * count are zero (ok = 0). */
typedef struct hpmvs_record {
    float center[4];
    float normal[4];
    float color[3];
    float scale;
    double fmin;
    uint8_t ok;
    uint8_t pad0;
    uint16_t n_images;
    uint8_t pad1[4];
    uint16_t images[HPMVS_RECORD_IMAGES]; /* unused slots 0xFFFF; n_images > HPMVS_RECORD_IMAGES: the first 64 ids */
} hpmvs_record;                        /* 192 bytes */
/* Lists longer than the record's HPMVS_RECORD_IMAGES ids (rare: a refined list of a dense scene): the record keeps the true
 * n_images and the first 64 ids, the ids from 64 on travel in a TAIL of the sender's overflow segment -- one more all-gather,
 * made only when some rank has a tail (every rank can tell from the gathered records: n_images > 64 with ok set).  The 192-byte
 * record is unchanged (format version 1 = no tails anywhere = what rounds 1-5 sent).
 *   hpmvs_pack_record_tails    tails of the refined patches (ok != 0) with n_images > 64, in patch order; *n_tails (host int) is
 *                              their number (the call synchronises the stream); HPMVS_ERR_ARG when `cap` tails do not hold them
 *   hpmvs_unpack_record_tails  ids 64.. of patch (patch_offset + tail.patch) of a batch that hpmvs_unpack_records has filled.
 *                              A tail whose patch falls outside the batch is dropped; an all-zero tail (the padding of a gathered
 *                              segment: patch 0, count 0) writes nothing; a MALFORMED tail, count > HPMVS_MAX_IMAGES -
 *                              HPMVS_RECORD_IMAGES, is rejected whole: none of its ids is written, the tails around it are applied
 *                              (hpmvs_amd.distributed.unpack_records raises ValueError for such a tail) */
typedef struct hpmvs_record_tail {
    int32_t patch;   /* index of the patch in the sender's shard */
    uint16_t count;  /* ids in this tail = n_images - 64 */
    uint16_t pad;
    uint16_t images[HPMVS_MAX_IMAGES - HPMVS_RECORD_IMAGES];
} hpmvs_record_tail; /* 392 bytes */
int hpmvs_pack_record_tails(const hpmvs_patch_batch *b, hpmvs_record_tail *tails, int32_t cap, int32_t *n_tails, void *stream);
int hpmvs_unpack_record_tails(const hpmvs_record_tail *tails, int32_t n_tails, int32_t patch_offset, hpmvs_patch_batch *b, void *stream);
int hpmvs_pack_records(const hpmvs_patch_batch *b, hpmvs_record *records, void *stream);
int hpmvs_unpack_records(const hpmvs_record *records, int n, hpmvs_patch_batch *b, void *stream);
int hpmvs_allgather_records(void *nccl_comm, const hpmvs_record *send, size_t count, hpmvs_record *recv, void *stream);

/* ---- the patch cloud as an extended PLY file (reference DynOctTree::toExtPly, include/hpmvs/doctree.h:526-622) -------------------
 * The header's lines; then per row x y z [nx ny nz] red green blue [scalar_scale]; then, with VISIBILITY, per row the list
 * "n id id ...".  ASCII (the reference's default): every field is followed by one space and every line ends " \n"; a float is
 * what `ostream << float` writes, printf("%.6g") of its exact value, n is written as int and an id as uint32_t (-1 prints
 * 4294967295).  Binary: per row 3 floats, [3 floats], 3 bytes, [1 float], then per row uint32 n and n uint32 ids, little endian.
 * A colour is the float truncated towards zero; below 0 it is 0, from 256 up 255, a NaN 0 (there the reference's ASCII path
 * prints (int) of the float, 300 or -3, and its binary path's (unsigned char) is undefined).
 * The conversion is integer arithmetic on the float's exact value (hpmvs_amd/csrc/ply_text.hpp) and runs on the device, as do the
 * placement of the lines (a 64-bit prefix sum: a cloud's text can pass 4 GiB) and their writing; DESIGN.md 3.21. */
#define HPMVS_PLY_BINARY 1
#define HPMVS_PLY_NORMAL 2
#define HPMVS_PLY_SCALE 4
#define HPMVS_PLY_VISIBILITY 8
/* The file DynOctTree::toExtPly writes for the rows order[0 .. n_rows-1] of b (order == NULL: rows 0 .. b->n-1, n_rows ignored;
 * a row may be named more than once), header included.  Reads center, normal, scale, color, n_images, images (those the flags
 * ask for; max_images may be any row stride >= 0); b's arrays and order are host pointers, or with on_device device pointers on
 * `device`; out is host memory.  out == NULL: *n = the file's exact length and nothing else is written.  cap smaller than the
 * file: HPMVS_ERR_ARG, nothing written, *n the length needed.  Zero rows give the header alone.
 * HPMVS_ERR_ARG before the device is looked for (HPMVS_ERR_NODEVICE): NULL b or n, a negative b->n, max_images or (with order)
 * n_rows, unknown flag bits, a cap with out == NULL, a missing array.  HPMVS_ERR_ARG with nothing written and the lowest such
 * row named in hpmvs_last_error: an order entry outside [0, b->n), and with VISIBILITY an n_images outside [0, max_images].
 * The call waits for its result (out is complete on return) and keeps nothing between calls. */
int hpmvs_ply_ext_batch(int device, const hpmvs_patch_batch *b, const int32_t *order, int n_rows, int flags,
                        uint8_t *out, size_t cap, size_t *n, int on_device, void *stream);
/* diagnostics (tools/ply_ext_scale.py): the same for host pointers with the stage times by HIP events: staging in, ply_len_kernel,
 * the scan and the total's read-back, ply_vertex_kernel, ply_list_kernel, the copy to the host */
int hpmvs_ply_ext_timed(int device, const hpmvs_patch_batch *b, const int32_t *order, int n_rows, int flags,
                        uint8_t *out, size_t cap, size_t *n, float *ms /*[6]*/);

/* ---- diagnostics --------------------------------------------------------------------------------------------------
 * The optimiser that optimize_kernel runs per lane (NLopt 2.4.2 LN_BOBYQA as PatchOptimizer.cpp:348-365 configures
 * it: 3 variables, xtol_rel 1e-7, default initial step), driven ON THE GPU by the analytic objectives of
 * hpmvs_amd/csrc/selftest_obj.h instead of the photometric one, 32 different problems per wavefront.  Exists so
 * that the device build of the blocks the photometric objective never reaches (rescue_, bobyqa.c:143-742; active
 * bounds; ROUNDOFF_LIMITED) can be compared evaluation by evaluation with the genuine library.  Host arrays:
 * kind[n], params[n][8], x0/lb/ub[n][3] in; xfinal[n][3], minf[n], result[n] (nlopt_result), nevals[n],
 * rescue_calls[n] out; trace[n][trace_cap][4] = (x0, x1, x2, f) of every evaluation (may be NULL).
 * A `device` that is no index of a visible device is HPMVS_ERR_ARG "selftest_bobyqa: bad device index", also for n = 0 (it
 * used to be HPMVS_ERR_HIP with the text of the failed hipSetDevice, and HPMVS_OK for n = 0). */
int hpmvs_selftest_bobyqa(int device, int n, const int32_t *kind, const double *params, const double *x0,
                          const double *lb, const double *ub, int maxeval, double *xfinal, double *minf,
                          int32_t *result, int32_t *nevals, int32_t *rescue_calls, double *trace, int trace_cap);

#ifdef __cplusplus
}
#endif
#endif /* HPMVS_AMD_H */
