/*
 * amos_frontend.h -- C ABI of the MI355X-native Amos-SLAM front-end hot path.
 *
 * This is the drop-in boundary.  Every entry point below replaces one member of the
 * reference's C++ front-end API (file:line under /root/reference):
 *
 *   ORBextractor::ORBextractor        src/ORBextractor.cc:492-609   -> amos_orb_create / amos_orb_tables
 *   ORBextractor::operator() (3-arg)  src/ORBextractor.cc:1672-1686 -> amos_orb_detect (+ amos_orb_level_keypoints)
 *   ORBextractor::MovingKeyPoints     src/ORBextractor.cc:1688-1745 -> amos_orb_gate
 *   ORBextractor::ProcessDesp         src/ORBextractor.cc:1747-1820 -> amos_orb_describe
 *   ORBextractor::operator() (4-arg)  src/ORBextractor.cc:1544-1668 -> amos_orb_extract
 *   ORBextractor::mvImagePyramid      include/ORBextractor.h:168    -> amos_orb_level_image
 *   ORBmatcher::DescriptorDistance    src/ORBmatcher.cc:1913-1933   -> amos_match_distances / amos_match_list_distances
 *   inner best / second-best loops of ORBmatcher::Search* (src/ORBmatcher.cc:70-175, 230-382,
 *     515-643, 1569-1728)                                           -> amos_match_list_best2 / amos_match_bruteforce_best2
 *
 * The host-side C++ classes with the reference's names (ORB_SLAM2::ORBextractor, ORBmatcher)
 * live in amos-slam_amd/host/ and are thin wrappers over these functions; INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes only, no C++ or torch types.  Every function returns
 * AMOS_OK (0) or a negative error code; amos_last_error() returns a thread-local description.
 * Unless a name ends in _device, pointers are HOST pointers and the call is synchronous.
 * All work of one handle is issued on one HIP stream owned by that handle (or handed in at create).
 * A handle is stateful exactly like an ORBextractor instance (one frame/batch in flight per handle);
 * distinct handles may be used from distinct threads concurrently.
 */
#ifndef AMOS_FRONTEND_H
#define AMOS_FRONTEND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMOS_OK 0
#define AMOS_ERR_INVALID (-1)   /* bad argument (null, size, range)                              */
#define AMOS_ERR_DEVICE (-2)    /* HIP runtime error; text in amos_last_error()                  */
#define AMOS_ERR_CAPACITY (-3)  /* caller buffer too small, or frame larger than the handle's max */
#define AMOS_ERR_STATE (-4)     /* call order violated (e.g. describe before detect)             */

#define AMOS_EDGE_THRESHOLD 19  /* border of every pyramid plane, ORBextractor.cc:93             */
#define AMOS_MAX_LEVELS 16
#define AMOS_FRAME_GRID_ROWS 48 /* Frame.h:56 */
#define AMOS_FRAME_GRID_COLS 64 /* Frame.h:61 */
#define AMOS_TH_HIGH 100        /* ORBmatcher.cc:49 */
#define AMOS_TH_LOW 50          /* ORBmatcher.cc:50 */
#define AMOS_HISTO_LENGTH 30    /* ORBmatcher.cc:51 */

/* Same field order and widths as cv::KeyPoint (pt.x, pt.y, size, angle, response, octave,
 * class_id), so a std::vector<cv::KeyPoint> can be filled with one memcpy. */
typedef struct amos_keypoint {
    float x, y;
    float size;
    float angle;
    float response;
    int32_t octave;
    int32_t class_id;
} amos_keypoint;

/* The five ORBextractor.* YAML parameters (Tracking.cc:161-177). */
typedef struct amos_orb_params {
    int32_t n_features;
    float scale_factor;
    int32_t n_levels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
} amos_orb_params;

typedef struct amos_orb amos_orb;
typedef struct amos_match amos_match;
typedef struct amos_mask_pre amos_mask_pre;

/* Result of a best / second-best reduction over one query's candidate list, ties resolved as the
 * reference's sequential `if(dist<best) ... else if(dist<best2)` loop does (first candidate wins). */
typedef struct amos_best2 {
    int32_t best_idx;     /* train index, -1 if no candidate beat init_dist */
    int32_t best_dist;    /* init_dist if none */
    int32_t second_idx;   /* -1 if none */
    int32_t second_dist;  /* init_dist if none */
} amos_best2;

const char *amos_last_error(void);
/* Number of HIP devices visible, or a negative error code. */
int amos_device_count(void);
/* The calling thread's current HIP device (hipGetDevice), or a negative error code.  The C++ drop-in classes
 * (amos-slam_amd/host) create their handles on it unless AMOS_DEVICE names another: a one-process-per-GPU host
 * that has called hipSetDevice / torch.cuda.set_device gets its objects on ITS GPU (the reference has no such
 * notion: its extractor is CPU code, ORBextractor.cc:492). */
int amos_current_device(void);
/* Which build of the library this is: "default" for the product build, otherwise the names of the timing-experiment
 * switches it was compiled with (AMOS_FAST_EXP=n, AMOS_W24_EXP_*, AMOS_FAST_LDS_PAD=n: builds whose RESULTS ARE WRONG,
 * tools/orb_variants.sh / tools/w24_variants.sh).  bench.py and the tests refuse anything but "default". */
const char *amos_build_variant(void);

/* ---------------------------------------------------------------- ORB extractor ------------- */

/* Allocates every device buffer for frames up to max_width x max_height and batches of up to
 * max_batch frames on HIP device `device`.  `stream` is a hipStream_t to issue on, or NULL to
 * let the handle create its own. */
int amos_orb_create(const amos_orb_params *params, int max_width, int max_height, int max_batch,
                    int device, void *stream, amos_orb **out);
void amos_orb_destroy(amos_orb *h);

/* Host-only capacity check (no device is touched): would a handle created for frames up to
 * max_width x max_height accept a width x height frame?  need / cap (either may be NULL) receive
 * {FAST cells, candidate slots, compacted candidates, per-level keypoint slots, resize tap records,
 * pyramid bytes / 256} of the frame and of the allocation.  Returns AMOS_OK, AMOS_ERR_CAPACITY
 * (a bound is exceeded: amos_orb_create's sizing would be wrong) or AMOS_ERR_INVALID (the frame has a
 * level without a FAST cell, which the reference cannot process either, ORBextractor.cc:1083-1086). */
int amos_orb_geometry_probe(const amos_orb_params *params, int max_width, int max_height, int width,
                            int height, int32_t need[6], int32_t cap[6]);

/* Constructor tables (a1).  Any pointer may be NULL.  Arrays hold n_levels entries, umax 16. */
int amos_orb_tables(const amos_orb *h, float *scale_factor, float *inv_scale_factor,
                    float *level_sigma2, float *inv_level_sigma2, int32_t *features_per_level,
                    int32_t *umax);
/* The same tables from the parameters alone: host arithmetic only, no device is touched and no handle is needed
 * (the reference's constructor is host code too, ORBextractor.cc:492-609).  Arrays hold params->n_levels entries. */
int amos_orb_tables_host(const amos_orb_params *params, float *scale_factor, float *inv_scale_factor,
                         float *level_sigma2, float *inv_level_sigma2, int32_t *features_per_level, int32_t *umax);
/* Level geometry for a w x h input: width/height per level.  Returns n_levels. */
int amos_orb_level_sizes(const amos_orb *h, int width, int height, int32_t *level_w, int32_t *level_h);

/* a7: pyramid + per-cell FAST + quad-tree distribution + orientation for ONE host frame
 * (8-bit gray, `stride` bytes per row).  Afterwards per-level keypoints (level coordinates,
 * not rescaled) are available through amos_orb_level_keypoints(frame = 0). */
int amos_orb_detect(amos_orb *h, const uint8_t *gray, size_t stride, int width, int height);

/* Number of keypoints of (frame, level) after the last detect/gate, or a negative error. */
int amos_orb_level_count(amos_orb *h, int frame, int level);
int amos_orb_level_keypoints(amos_orb *h, int frame, int level, amos_keypoint *out, int cap);
/* Replaces the device-resident list of (frame, level) by the caller's (the reference hands the
 * per-level vectors back into MovingKeyPoints / ProcessDesp, Frame.cc:491-496,633). */
int amos_orb_set_level_keypoints(amos_orb *h, int frame, int level, const amos_keypoint *kps, int n);

/* Bulk forms of the two calls above for the C++ drop-in classes: one transfer for all levels.
 * Layout: the list of level l occupies buf[offsets[l] .. offsets[l] + counts[l]), capacity
 * caps[l]; total = buffer length in keypoints.  offsets/caps depend on the frame size only. */
int amos_orb_level_layout(amos_orb *h, int32_t *offsets, int32_t *caps, int32_t *total);
int amos_orb_fetch_levels(amos_orb *h, int frame, int32_t *counts, amos_keypoint *buf, int buf_len);
int amos_orb_store_levels(amos_orb *h, int frame, const int32_t *counts, const amos_keypoint *buf, int buf_len);

/* a8: closing (dilate then erode, 31x31 ellipse) of the 8-bit mask of the level-0 frame size and
 * removal of every keypoint whose scaled position hits a non-zero closed-mask pixel or a removed
 * cluster.  `labels` (row-major doubles, lstride elements per row), `center_ids`, `rm_vector`
 * describe the SLIC/k-means label gate and may all be NULL (label gate off).  Removed keypoints
 * are returned in the reference's order (level by level, list order).  Operates on frame 0. */
int amos_orb_gate(amos_orb *h, const uint8_t *mask, size_t mask_stride, const double *labels,
                  size_t lstride, const int32_t *center_ids, int n_centers,
                  const int32_t *rm_vector, int n_rm, amos_keypoint *removed, int cap,
                  int *n_removed);
/* The closed mask of the last amos_orb_gate call (for parity tests).  AMOS_ERR_STATE when no gate has run, and when the last gate
 * was a batch gate on bit planes (amos_orb_gate_mode 1, the default): that gate makes no grey closed mask. */
int amos_orb_closed_mask(amos_orb *h, uint8_t *dst, size_t dst_stride);

/* a9: 7x7 sigma-2 blur of every level, 256-bit rBRIEF of the current per-level lists, rescale of
 * the coordinates to level 0, concatenation in level order.  desc is n x 32 bytes row-major. */
int amos_orb_describe(amos_orb *h, amos_keypoint *kps, uint8_t *desc, int cap, int *n);

/* a11 = detect + describe without gating. */
int amos_orb_extract(amos_orb *h, const uint8_t *gray, size_t stride, int width, int height,
                     amos_keypoint *kps, uint8_t *desc, int cap, int *n);

/* mvImagePyramid[level] of `frame`: the level image (padded != 0: with its 19-px reflect-101
 * border, i.e. (w+38) x (h+38)) copied to host memory. */
int amos_orb_level_image(amos_orb *h, int frame, int level, uint8_t *dst, size_t dst_stride,
                         int padded);
/* All level planes of one frame at once (mvImagePyramid of the C++ class): dst[l] / dst_strides[l] per level (dst[l] NULL skips the level);
 * padded != 0 copies the (w + 38) x (h + 38) plane including the reflect-101 border, as amos_orb_level_image does.  One device-to-host
 * transfer of the frame's pyramid through a pinned staging buffer. */
int amos_orb_pyramid_images(amos_orb *h, int frame, uint8_t *const *dst, const size_t *dst_strides, int padded);
/* The blurred level used by the last describe (unpadded, w x h). */
int amos_orb_blurred_image(amos_orb *h, int frame, int level, uint8_t *dst, size_t dst_stride);
/* FAST candidates of (frame, level) before the quad-tree, in the reference's order
 * (cell-row-major, then row-major inside the cell): x, y relative to (minBorderX, minBorderY),
 * response = score.  For parity tests. */
int amos_orb_level_candidates(amos_orb *h, int frame, int level, amos_keypoint *out, int cap);

/* Batched, device-resident path.  d_gray holds n_frames frames, frame f at
 * d_gray + f * frame_stride, rows `row_stride` bytes apart.  Runs a11 on every frame; results stay
 * on the device (amos_orb_batch_results_device) and nothing is copied to the host.  Asynchronous on
 * the handle's stream; amos_orb_sync() waits. */
int amos_orb_extract_batch_device(amos_orb *h, const uint8_t *d_gray, size_t frame_stride,
                                  size_t row_stride, int width, int height, int n_frames);
/* The same split in stages for the full front-end with the mask (a7 -> a8 -> a9 per frame of the
 * batch, everything device-resident): detect, then gate with n_frames 8-bit masks (frame f at
 * d_masks + f * mask_frame_stride; label gate off), then describe.  Asynchronous. */
int amos_orb_detect_batch_device(amos_orb *h, const uint8_t *d_gray, size_t frame_stride, size_t row_stride,
                                 int width, int height, int n_frames);
int amos_orb_gate_batch_device(amos_orb *h, const uint8_t *d_masks, size_t mask_frame_stride,
                               size_t mask_row_stride);
/* The same gate with CalDyna's label gate per frame (ORBextractor::MovingKeyPoints with labelMask, centers[].id, rmVector,
 * Frame.cc:633): a keypoint is also removed where rm[centers[(int) labels(y, x) - 1].id] == 1.  Frame f reads d_labels + f *
 * label_frame_stride (doubles, rows label_row_stride elements apart), d_centers + f * centers_frame_stride (records; .id is read) and
 * d_rm + f * rm_frame_stride (n_rm int32).  d_status [n_frames]: 0, or bit 1 a keypoint outside the mask, bit 2 a label outside
 * [1, n_centers] or an id outside [0, n_rm) (the keypoint is then kept, as amos_orb_gate does).  Follow with amos_orb_describe_batch_device. */
struct amos_slic_center;
int amos_orb_gate_labels_batch_device(amos_orb *h, const uint8_t *d_masks, size_t mask_frame_stride, size_t mask_row_stride,
                                      const double *d_labels, size_t label_frame_stride, size_t label_row_stride,
                                      const struct amos_slic_center *d_centers, size_t centers_frame_stride, int n_centers,
                                      const int32_t *d_rm, size_t rm_frame_stride, int n_rm, int32_t *d_status);
int amos_orb_describe_batch_device(amos_orb *h);
/* How the two batch gates close the masks.  1 (default): on bit planes -- the gate only asks closed(y, x) != 0, and the non-zero set of
 * the grey closing is the binary closing of the mask's non-zero set; the same keypoints are removed, amos_orb_closed_mask is not
 * available afterwards.  0: grey planes, as amos_orb_gate.  Other values only query.  Returns the previous mode; the initial value is
 * AMOS_GATE_BITS=0 / 1 in the environment, read once per process. */
int amos_orb_gate_mode(int mode);
/* The keypoints the last gate removed from `frame` of the batch, in the reference's order, to host memory (removed may be NULL: the
 * count only).  Synchronises the handle's stream.  For parity tests. */
int amos_orb_batch_removed(amos_orb *h, int frame, amos_keypoint *removed, int cap, int *n_removed);

/* ---- callers either side of the path (SURVEY 8f "next" rows), device resident ----
 * Tracking::GrabImageRGBD's cvtColor(..., CV_{BGR,RGB}[A]2GRAY) (Tracking.cc:308-321) fused into the
 * level-0 import: d_color holds interleaved 8-bit frames with `channels` = 3 or 4 bytes per pixel,
 * rgb_order != 0 for RGB[A] (Tracking's mbRGB), 0 for BGR[A].  Otherwise as amos_orb_extract_batch_device. */
int amos_orb_extract_batch_device_color(amos_orb *h, const uint8_t *d_color, size_t frame_stride, size_t row_stride,
                                        int width, int height, int n_frames, int channels, int rgb_order);
/* Frame::ComputeStereoFromRGBD (Frame.cc:1576-1615) and the cell of Frame::AssignFeaturesToGrid /
 * PosInGrid (Frame.cc:431-461, 1007-1030) for every keypoint of the last batch.  The depth map is 16-bit with Tracking's convertTo(CV_32F,
 * depth_map_factor) applied on the fly (depth_is_u16 != 0) or already float32; d_depth NULL = monocular
 * (grid cells only).  d_kps_un = mvKeysUn from amos_frame_undistort_batch_device, or NULL for a
 * zero-distortion camera (mvKeysUn == mvKeys, as for TUM3): the depth is read at mvKeys, uRight and the
 * cell use mvKeysUn.  Outputs are [n_frames][capacity] arrays on the device (capacity from amos_orb_batch_results_device):
 * u_right / depth = -1 where the depth is not positive, grid_cell = col * 48 + row or -1. */
int amos_frame_rgbd_glue_batch_device(amos_orb *h, const void *d_depth, int depth_is_u16, float depth_map_factor,
                                      size_t depth_frame_stride_bytes, size_t depth_row_stride_bytes, float mbf,
                                      float min_x, float max_x, float min_y, float max_y,
                                      const amos_keypoint *d_kps_un, float *d_u_right, float *d_depth_out,
                                      int32_t *d_grid_cell);
/* Frame::ComputeStereoMatches (Frame.cc:1179-1573) for n_pairs stereo pairs of resident extractions: the band search over the right
 * keypoints (rows floor(yR - r) .. ceil(yR + r), r = 2 * scale[octaveR]; octave within +-1; uL - mbf / min_z <= uR <= uL) with its Hamming
 * loop, the 11 x 11 SAD over 11 shifts on the level of the left keypoint, the parabola fit, depth = mbf / disparity and the rejection of
 * every match whose SAD is not below 1.5f * 1.4f * median.  Integer Hamming and SAD, float32 in the source's order, nothing fused.
 * Pairing: with two handles pair p is frame p of each; with left == right pair p is frames 2p (left) and 2p + 1 (right) of the one batch.
 * The handles need the same amos_orb_params and frame size and live on one device.  mbf, min_z > 0; the reference's minZ is its mb,
 * i.e. the caller passes min_z = mbf / fx.
 * The first entry matches each handle's batch results (amos_orb_batch_results_device); the second takes the keypoints, descriptors
 * (16-byte aligned, 32 bytes each) and counts explicitly -- laid out [frames][capacity] and indexed by the same frame numbers -- and uses
 * the handles for their pyramid planes and tables only.
 * Outputs, on the device: d_u_right, d_depth [n_pairs][capacity_l] (capacity_l = left's capacity in the first entry), -1 where there is no
 * match; d_sad [n_pairs][capacity_l] (may be NULL): the best SAD of every match accepted BEFORE the median step, else -1; d_status
 * [n_pairs] (may be NULL): 0, or bit 1 when a left keypoint's row is outside [0, height) or a keypoint's octave outside the pyramid (such
 * a keypoint is skipped).  Window rows and columns are clamped into the padded plane (the reference does not check them).  A pair
 * without an accepted match is left all -1 (the reference indexes an empty vector there).
 * Asynchronous on left's stream; when the handles differ, left's stream waits for an event recorded on right's (and right's next work
 * for the two launches): no host synchronisation.  AMOS_ERR_STATE before an extraction, AMOS_ERR_INVALID otherwise. */
int amos_frame_stereo_match_batch_device(amos_orb *left, amos_orb *right, int n_pairs, float mbf, float min_z, float *d_u_right,
                                         float *d_depth, int32_t *d_sad, int32_t *d_status);
int amos_frame_stereo_match_arrays_device(amos_orb *left, amos_orb *right, int n_pairs, const amos_keypoint *d_kps_l,
                                          const uint8_t *d_desc_l, const int32_t *d_counts_l, int capacity_l,
                                          const amos_keypoint *d_kps_r, const uint8_t *d_desc_r, const int32_t *d_counts_r,
                                          int capacity_r, float mbf, float min_z, float *d_u_right, float *d_depth, int32_t *d_sad,
                                          int32_t *d_status);
/* The host form for the C++ drop-in (amos-slam_amd/host/FrameStereo.h): pair 0 of the two handles' last extractions (left == right: frames
 * 0 and 1 of the one batch), synchronous; u_right / depth are HOST arrays that receive the first n entries (n = number of left keypoints,
 * at most left's capacity) in ONE device-to-host transfer of the two float arrays.  No pyramid plane leaves the device. */
int amos_frame_stereo_match(amos_orb *left, amos_orb *right, float mbf, float min_z, float *u_right, float *depth, int n);
/* Frame::UndistortKeyPoints (Frame.cc:1052-1118) for every keypoint of the last batch:
 * cv::undistortPoints(pts, pts, K, distCoef, Mat(), K) with OpenCV's default criteria (5 iterations, double
 * arithmetic), distCoef = (k1, k2, p1, p2[, k3]) as Tracking reads them from the YAML (n_dist = 4 or 5;
 * n_dist = 0 or k1 == 0 copies the keypoints, Frame.cc:1057-1061).  d_kps_un is [n_frames][capacity]. */
int amos_frame_undistort_batch_device(amos_orb *h, float fx, float fy, float cx, float cy, const float *dist_coef,
                                      int n_dist, amos_keypoint *d_kps_un);
/* Frame::ComputeImageBounds (Frame.cc:1121-1170): bounds = {mnMinX, mnMaxX, mnMinY, mnMaxY} from the four
 * undistorted image corners (host; the same point routine as the kernel). */
int amos_frame_image_bounds(int width, int height, float fx, float fy, float cx, float cy, const float *dist_coef,
                            int n_dist, float bounds[4]);

/* Device pointers of the batch results: keypoints [max_batch][capacity], descriptors
 * [max_batch][capacity][32], counts [max_batch].  Valid until destroy. */
int amos_orb_batch_results_device(amos_orb *h, const amos_keypoint **d_kps, const uint8_t **d_desc,
                                  const int32_t **d_counts, int *capacity);
/* Copies frame `frame` of the last batch to host buffers. */
int amos_orb_batch_fetch(amos_orb *h, int frame, amos_keypoint *kps, uint8_t *desc, int cap, int *n);
int amos_orb_sync(amos_orb *h);

/* Per-kernel timing with HIP events on the handle's stream (measurement, bench.py's roofline).
 * After amos_orb_timing_enable(h, max_records) every batch / extract pass records one event
 * between consecutive stages; amos_orb_timing_collect() synchronises, returns the average
 * duration of each stage in milliseconds over the recorded passes and resets the record count.
 * Stages: 0 level-0 import (k_pyramid_level0), 1 resize levels (n_levels - 1 launches of
 * k_pyramid_level), 2 FAST cells, 3 quad-tree, 4 orientation, 5 blur (side stream, overlaps
 * FAST), 6 rBRIEF.  max_records = 0 switches timing off. */
#define AMOS_ORB_STAGES 7
int amos_orb_timing_enable(amos_orb *h, int max_records);
int amos_orb_timing_collect(amos_orb *h, float *avg_ms, int *n_records);
/* The hipStream_t the handle issues on. */
void *amos_orb_stream(amos_orb *h);

/* ---------------------------------------------------------------- matcher ------------------- */

int amos_match_create(int device, void *stream, amos_match **out);
void amos_match_destroy(amos_match *m);
int amos_match_sync(amos_match *m);
void *amos_match_stream(amos_match *m);

/* a12, dense: out[i*nt + j] = Hamming(q_i, t_j), descriptors 32 bytes each, row-major. */
int amos_match_distances(amos_match *m, const uint8_t *q, int nq, const uint8_t *t, int nt,
                         uint16_t *out);
/* a12 over candidate lists (CSR): query i owns cand_idx[cand_off[i] .. cand_off[i+1]);
 * out[k] = Hamming(q_i, t_{cand_idx[k]}).  This is what the greedy Search* loops consume. */
int amos_match_list_distances(amos_match *m, const uint8_t *q, int nq, const uint8_t *t, int nt,
                              const int32_t *cand_off, const int32_t *cand_idx, uint16_t *out);
/* a13 inner reduction over candidate lists: best and second best in candidate order.
 * init_dist is the loop's initial bestDist (256 in SearchByProjection, INT_MAX in
 * SearchForInitialization): only distances < init_dist can win. */
int amos_match_list_best2(amos_match *m, const uint8_t *q, int nq, const uint8_t *t, int nt,
                          const int32_t *cand_off, const int32_t *cand_idx, int init_dist,
                          amos_best2 *out);
/* The same with every train descriptor as candidate, in index order (N_q x N_t brute force). */
int amos_match_bruteforce_best2(amos_match *m, const uint8_t *q, int nq, const uint8_t *t, int nt,
                                int init_dist, amos_best2 *out);
/* Which kernel the two brute-force entry points run: 0 = chosen by size (default), 1 = xor + popcount on the vector
 * units, 2 = exact-integer i8 MFMA (ham = |q| + sum_k t_k (1 - 2 q_k), v_mfma_i32_32x32x32_i8).  Identical results;
 * a measurement / test switch. */
int amos_match_set_bruteforce_kernel(amos_match *m, int mode);
/* Device-pointer form for the batched pipeline: for each of n_pairs (query frame, train frame)
 * pairs: descriptors at d_desc + frame * frame_stride_bytes, counts in d_counts[frame]; out is
 * [n_pairs][capacity] amos_best2 on the device.  Asynchronous on the matcher's stream. */
int amos_match_bruteforce_best2_batch_device(amos_match *m, const uint8_t *d_desc,
                                             size_t frame_stride_bytes, const int32_t *d_counts,
                                             const int32_t *d_pairs_q, const int32_t *d_pairs_t,
                                             int n_pairs, int capacity, int init_dist,
                                             amos_best2 *d_out);

/* ---------------------------------------------------------------- resident search (8f-1) ---- */

/* Frame::AssignFeaturesToGrid (Frame.cc:431-461) for a batch on the device.  d_grid_cell is the
 * per-keypoint cell number written by amos_frame_rgbd_glue_batch_device ([n_frames][capacity], -1 =
 * outside the grid); d_counts the keypoint counts.  Output, per frame: CSR d_cell_start
 * [64*48 + 1] (cell = x * 48 + y, as mGrid[x][y]) and d_items [capacity] holding keypoint indices,
 * ascending inside a cell (the reference's push_back order).  Asynchronous on the matcher's stream. */
int amos_frame_grid_build_batch_device(amos_match *m, const int32_t *d_grid_cell, const int32_t *d_counts,
                                       int n_frames, int capacity, int32_t *d_cell_start,
                                       int32_t *d_items);

/* Frame::GetFeaturesInArea (Frame.cc:894-1003) + the best / second-best candidate loop of
 * ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1629-1690) for a
 * batch of (query frame, train frame) pairs of resident extraction results.  Query i of pair p is
 * keypoint i of frame d_pairs_q[p]; it is searched in frame d_pairs_t[p] around d_query_uv[p][i]
 * (its own position when d_query_uv is NULL) with radius th * scale_factors[octave] and the level
 * window of mode (0: octave-1..octave+1, 1 = bForward: >= octave, 2 = bBackward: <= octave).  With
 * d_u_right and d_query_invz the stereo gate |u - mbf*invz - uRight[i2]| > radius rejects (:1662-1669).
 * d_out[p][i] = best / second best in candidate order under "dist < init_dist" (256 in the reference).
 * The greedy skip of already-matched features (:1658-1660) is the caller's: the unrestricted best
 * equals the restricted best whenever it is still free. */
typedef struct amos_window_search {
    const amos_keypoint *d_kps;   /* [frames][capacity]      (amos_orb_batch_results_device) */
    const uint8_t *d_desc;        /* [frames][capacity][32] */
    const int32_t *d_counts;      /* [frames] */
    const int32_t *d_cell_start;  /* [frames][64*48+1]       (amos_frame_grid_build_batch_device) */
    const int32_t *d_items;       /* [frames][capacity] */
    const float *d_query_uv;      /* [n_pairs][capacity][2] or NULL */
    const float *d_query_invz;    /* [n_pairs][capacity] or NULL */
    const float *d_u_right;       /* [frames][capacity] or NULL */
    const int32_t *d_pairs_q, *d_pairs_t; /* [n_pairs] */
    const float *scale_factors;   /* host, n_levels entries (mvScaleFactors) */
    int32_t n_pairs, capacity, n_levels;
    int32_t mode, init_dist;
    float th, mbf;
    float min_x, max_x, min_y, max_y; /* Frame::mnMinX .. mnMaxY */
} amos_window_search;
int amos_match_window_best2_batch_device(amos_match *m, const amos_window_search *w, amos_best2 *d_out);

/* ---------------------------------------------------------------- local map search ---------- */

/* Step 2 of Tracking::SearchLocalPoints (Tracking.cc:2352-2389) for a batch of resident frames: Frame::isInFrustum (Frame.cc:761-891)
 * with MapPoint::PredictScale (MapPoint.cc:571-586) on every local map point, then ORBmatcher::SearchByProjection(Frame&, const
 * vector<MapPoint*>&, th) (ORBmatcher.cc:70-175) over the points in view, greedy loop included: three launches, nothing returns to the host.
 *
 * Arithmetic (PARITY UNPINNED, like the other OpenCV-derived stages): float32, every operation rounded, nothing fused, except
 *   Pc = Rcw * P + tcw       one gemm per row: ((R0 P0 + R1 P1) + R2 P2) + t in double, one rounding to float; PcZ < 0 is out of view
 *   invz = 1.0f / PcZ;  u = ((fx * PcX) * invz) + cx;  v alike;  projXR = u - mbf * invz
 *   a u or v that is not finite is out of view and sets bit 0 (value 1) of the frame's status (the reference goes on to convert it
 *   to int, which is undefined);
 *   u < min_x || u > max_x || v < min_y || v > max_y is out of view
 *   PO = P - Ow;  dist = (float) sqrt(((double) PO0^2 + (double) PO1^2) + (double) PO2^2)            (cv::norm on CV_32F)
 *   dist < 0.8f * min_distance || dist > 1.2f * max_distance is out of view
 *   viewCos = (float) ((((double) PO0 Pn0 + (double) PO1 Pn1) + (double) PO2 Pn2) / (double) dist)  (Mat::dot returns double)
 *   viewCos < view_cos_limit is out of view
 *   level = number of m in [0, n_levels) with max_distance / dist > scale_factors[m], at most n_levels - 1 (a NaN ratio gives 0): this
 *   is ceil(logf(ratio) / mfLogScaleFactor) clamped, without a library logarithm; the two differ only for a ratio within rounding of
 *   a table entry.
 * Search: radius r * scale_factors[level], r = ((double) viewCos > 0.998 ? 2.5f : 4.0f), times th when th != 1; levels level - 1 .. level;
 * features with d_occupied set or already matched by a point with observations are skipped; a feature with uRight > 0 is rejected when
 * |projXR - uRight| > radius; first candidate wins ties; accepted when bestDist <= AMOS_TH_HIGH and not (the two best are on one level and
 * (float) bestDist > nn_ratio * (float) bestDist2).  A later point may overwrite the match of a point without observations. */
typedef struct amos_map_point {        /* one MapPoint as isInFrustum / PredictScale / the search read it: 80 bytes */
    float pos[3];                      /* GetWorldPos() */
    float normal[3];                   /* GetNormal() */
    float min_distance, max_distance;  /* mfMinDistance, mfMaxDistance (raw: the 0.8f / 1.2f factors are applied on the device) */
    int32_t flags;                     /* bit 0: skip (isBad() or mnLastFrameSeen == frame id), bit 1: Observations() > 0 */
    uint8_t desc[32];                  /* GetDescriptor() */
    uint8_t pad[12];                   /* to a multiple of 16 bytes */
} amos_map_point;
#define AMOS_MAP_POINT_SKIP 1
#define AMOS_MAP_POINT_HAS_OBS 2

typedef struct amos_local_camera {     /* per frame: 92 bytes */
    float Rcw[9], tcw[3], Ow[3];       /* Frame::mRcw (row-major), mtcw, mOw */
    float fx, fy, cx, cy, mbf;
    float view_cos_limit;              /* 0.5 in Tracking.cc:2365 */
    float th, nn_ratio;                /* 1 / 3 / 5 and 0.8 in Tracking.cc:2378-2389 */
} amos_local_camera;

typedef struct amos_local_stats {
    int32_t n_in_view;                 /* points that passed isInFrustum */
    int32_t n_matches;                 /* the search's return value */
    int32_t n_researched;              /* points in view whose window was searched again because a best-two feature had been taken */
    int32_t status;                    /* a bit mask: 0, or bit 0 (value 1) set: a projection of the frame was not finite */
} amos_local_stats;

struct amos_map_query;                 /* include/amos_host_types.h: mTrackProjX/Y/XR, mTrackViewCos, mnTrackScaleLevel, has_obs, descriptor */

typedef struct amos_local_search {
    const amos_keypoint *d_kps;        /* [frames][capacity]: the caller's undistorted keypoints (mvKeysUn) */
    const uint8_t *d_desc;             /* [frames][capacity][32] */
    const int32_t *d_counts;           /* [frames] */
    const int32_t *d_cell_start;       /* [frames][64*48+1]       (amos_frame_grid_build_batch_device) */
    const int32_t *d_items;            /* [frames][capacity] */
    const float *d_u_right;            /* [frames][capacity] or NULL (monocular) */
    const amos_map_point *d_points;    /* frame f owns points [point_off[f], point_off[f + 1]) */
    const int32_t *point_off;          /* host, n_frames + 1 entries, ascending from >= 0 */
    const amos_local_camera *cameras;  /* host, n_frames entries */
    const uint8_t *d_occupied;         /* [frames][capacity]: 1 where F.mvpMapPoints[idx] is set and has Observations() > 0 on entry */
    const float *scale_factors;        /* host, n_levels entries (mvScaleFactors) */
    struct amos_map_query *d_query;    /* out, one per point: every tested point is written, the values hold where it is in view */
    uint8_t *d_in_view;                /* out, one per point: mbTrackInView */
    int32_t *d_match;                  /* out, [frames][capacity]: index of the matched point inside the frame's own list, or -1 */
    amos_local_stats *d_stats;         /* out, [frames] */
    int32_t n_frames, capacity, n_levels;
    float min_x, max_x, min_y, max_y;  /* Frame::mnMinX .. mnMaxY */
} amos_local_search;
/* Asynchronous on the matcher's stream (the two host arrays and the table are consumed before the call returns).  capacity <= 65536: the CSR
 * position is packed in 16 bits of the reduction key.  AMOS_ERR_INVALID for a NULL argument, a capacity or n_levels out of range, a
 * point_off that descends or empty image bounds. */
int amos_match_local_points_batch_device(amos_match *m, const amos_local_search *s);
/* The host form for a C++ drop-in: ONE frame of n features (mvKeysUn, mDescriptors, mvuRight or
 * NULL) and n_points map points, host arrays in and out, synchronous: one upload (the grid cells of Frame::PosInGrid are computed on the
 * way), AssignFeaturesToGrid and the three launches on the device, one download.  occupied [n]; query, in_view [n_points]; match [n]. */
int amos_match_local_points(amos_match *m, const amos_keypoint *kps_un, const uint8_t *desc, const float *u_right, int n,
                            const amos_map_point *points, int n_points, const amos_local_camera *camera, const uint8_t *occupied,
                            const float *scale_factors, int n_levels, float min_x, float max_x, float min_y, float max_y,
                            struct amos_map_query *query, uint8_t *in_view, int32_t *match, amos_local_stats *stats);

/* ---------------------------------------------------------------- motion-model search ------- */

/* Tracking::TrackWithMotionModel's search (Tracking.cc:1925-1945) for a batch of resident frames: the fill of mvpMapPoints with NULL,
 * ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1569-1728) -- projection, window search, greedy loop,
 * rotation histogram with ComputeThreeMaxima -- and the second search with th_retry when the first returned fewer than retry_below
 * matches.  Three launches (projection, window search, acceptance) plus two for the second search; nothing returns to the host.
 *
 * Arithmetic (PARITY UNPINNED, like the other OpenCV-derived stages): float32, every operation rounded, nothing fused, except
 *   x3Dc = Rcw * P + tcw     one gemm per row: ((R0 P0 + R1 P1) + R2 P2) + t in double, one rounding to float
 *   invzc = (float) (1.0 / (double) zc);  invzc < 0 is skipped
 *   u = ((fx * xc) * invzc) + cx;  v alike
 *   a u or v that is not finite is skipped and sets bit 0 (value 1) of the frame's status (the reference goes on to convert it to int);
 *   an octave outside [0, n_levels) is skipped and sets bit 1 (value 2) (the reference indexes mvScaleFactors with it)
 *   u < min_x || u > max_x || v < min_y || v > max_y is skipped
 *   twc = -Rcw^T tcw;  tlc = Rlw twc + tlw, one gemm each (host);  bForward = tlc.z > mb && !mono;  bBackward = -tlc.z > mb && !mono
 * Search: radius th * scale_factors[octave]; levels >= octave when bForward, else 0 .. octave when bBackward, else octave - 1 .. octave + 1
 * (GetFeaturesInArea's bCheckLevels rule, Frame.cc:894-1003); a feature with uRight > 0 is rejected when |(u - mbf * invzc) - uRight| >
 * radius; a feature matched by a point with observations is skipped; the first candidate wins ties; accepted when bestDist <=
 * AMOS_TH_HIGH (no ratio test).  A later point may overwrite the match of a point without observations.
 * Rotation consistency (check_orientation): rot = angleLast - angleCur, + 360.0f when rot < 0; bin = (int) roundf(rot * (30 / 360.0f)),
 * 30 becomes 0.  The histogram holds one entry per ACCEPTED POINT (:1683-1698), so a feature that was overwritten is in it once per
 * accepting point; every entry of a bin that is not one of ComputeThreeMaxima's three (strict comparisons, max2 < 0.1f * max1 drops the
 * second and third, max3 < 0.1f * max1 the third) sets its feature to -1 and lowers n_matches, unconditionally (:1714-1724).
 * Second search: when retry_below > 0 and the first search's n_matches (after the pruning) is below it, d_match is reset and the search
 * runs again from the empty frame with th_retry; its result stands whatever it is. */
typedef struct amos_last_point {       /* LastFrame feature i as the search reads it: 64 bytes */
    float pos[3];                      /* LastFrame.mvpMapPoints[i]->GetWorldPos() */
    float angle;                       /* LastFrame.mvKeysUn[i].angle */
    int32_t octave;                    /* LastFrame.mvKeys[i].octave */
    int32_t flags;                     /* bit 0: skip (no map point, or mvbOutlier[i]); bit 1: Observations() > 0 */
    uint8_t desc[32];                  /* pMP->GetDescriptor() (the map point's, not the feature's) */
    uint8_t pad[8];
} amos_last_point;
#define AMOS_LAST_POINT_SKIP 1
#define AMOS_LAST_POINT_HAS_OBS 2

typedef struct amos_motion_camera {    /* per frame: 140 bytes */
    float Rcw[9], tcw[3];              /* CurrentFrame.mTcw (after SetPose(mVelocity * mLastFrame.mTcw)), rotation row-major */
    float Rlw[9], tlw[3];              /* LastFrame.mTcw */
    float fx, fy, cx, cy, mbf, mb;
    float th, th_retry;                /* 15 / 30 (7 / 14 for stereo), Tracking.cc:1929-1944 */
    int32_t retry_below;               /* 20; 0 = never search again */
    int32_t mono, check_orientation;   /* bMono; mbCheckOrientation (true in Tracking.cc:1910) */
} amos_motion_camera;

typedef struct amos_motion_stats {     /* 32 bytes */
    int32_t n_projected;               /* points that reached GetFeaturesInArea */
    int32_t n_matches;                 /* the return value of the search whose result stands (may count a feature twice, see above) */
    int32_t n_first;                   /* the return value of the first search */
    int32_t pass;                      /* 1 or 2: which radius produced d_match */
    int32_t n_researched;              /* of the pass that stands: points whose window was searched again because both of its best two were taken */
    int32_t flags;                     /* bit 0 bForward, bit 1 bBackward */
    int32_t status;                    /* bit 0: a projection was not finite; bit 1: an octave outside the table */
    int32_t pad;
} amos_motion_stats;

struct amos_proj_query;                /* include/amos_host_types.h: u, v, invz, octave, angle, has_obs, descriptor */

typedef struct amos_motion_search {
    const amos_keypoint *d_kps;        /* [frames][capacity]: the current frames' undistorted keypoints (mvKeysUn) */
    const uint8_t *d_desc;             /* [frames][capacity][32] */
    const int32_t *d_counts;           /* [frames] */
    const int32_t *d_cell_start;       /* [frames][64*48+1]       (amos_frame_grid_build_batch_device) */
    const int32_t *d_items;            /* [frames][capacity] */
    const float *d_u_right;            /* [frames][capacity] or NULL (monocular) */
    const amos_last_point *d_points;   /* frame f owns points [point_off[f], point_off[f + 1]) */
    const int32_t *point_off;          /* host, n_frames + 1 entries, ascending from >= 0 */
    const amos_motion_camera *cameras; /* host, n_frames entries */
    const float *scale_factors;        /* host, n_levels entries (mvScaleFactors) */
    struct amos_proj_query *d_query;   /* out, one per point: every point is written, u / v / invz hold where it is projected */
    uint8_t *d_projected;              /* out, one per point: 1 where the point reached GetFeaturesInArea */
    int32_t *d_match;                  /* out, [frames][capacity]: index of the matched point inside the frame's own list, or -1 (reset by the call) */
    amos_motion_stats *d_stats;        /* out, [frames] */
    int32_t n_frames, capacity, n_levels;
    float min_x, max_x, min_y, max_y;  /* Frame::mnMinX .. mnMaxY */
} amos_motion_search;
/* Asynchronous on the matcher's stream (the two host arrays and the table are consumed before the call returns).  capacity <= 65536.
 * AMOS_ERR_INVALID, before the device is touched, for a NULL handle or argument, a capacity or n_levels out of range, a point_off that
 * descends or empty image bounds.  Five launches; three when every retry_below is 0. */
int amos_match_motion_model_batch_device(amos_match *m, const amos_motion_search *s);
/* The host form for a C++ drop-in (amos-slam_amd/host/FrameMotionModel.h): ONE current frame of n features (mvKeysUn, mDescriptors, mvuRight
 * or NULL) and n_points last-frame features, host arrays in and out, synchronous: one upload (the grid cells of Frame::PosInGrid are
 * computed on the way), AssignFeaturesToGrid and the launches on the device, one download.  query, projected [n_points]; match [n]. */
int amos_match_motion_model(amos_match *m, const amos_keypoint *kps_un, const uint8_t *desc, const float *u_right, int n,
                            const amos_last_point *points, int n_points, const amos_motion_camera *camera, const float *scale_factors,
                            int n_levels, float min_x, float max_x, float min_y, float max_y, struct amos_proj_query *query,
                            uint8_t *projected, int32_t *match, amos_motion_stats *stats);

/* ---------------------------------------------------------------- pose optimisation ---------- */

/* Optimizer::PoseOptimization(&mCurrentFrame) (Optimizer.cc:363-605) for a batch of resident frames, behind any search that writes
 * d_match: the motion-only bundle adjustment that follows every search of the tracking thread (Tracking.cc:1764, :1953, :2014 and the calls
 * inside Relocalization), with g2o's Levenberg-Marquardt, Huber kernel, projection edges and dense LDL^T solve restated in double
 * (amos-slam_amd/csrc/amos_pose_core.h: PARITY WITH g2o UNPINNED; the header lists the deviations).  ONE launch, one work-group per frame.
 *
 * Feature i < d_counts[f] with d_match[i] >= 0 is an edge: monocular when d_u_right is NULL or d_u_right[i] < 0, else stereo; its point is
 * record point_off[f] + d_match[i] of d_points, its weight inv_level_sigma2[octave].  A feature whose octave lies outside [0, n_levels)
 * or whose match index lies outside the frame's points is skipped and sets bit 0 / bit 1 of status.  Fewer than 3 edges: the result holds
 * the input pose, n_inliers = 0, rounds = 0, and d_outlier / d_match are not written.  Otherwise d_outlier[i] is written for every edge
 * (other features keep what the array held) and the result is the last executed round's pose. */
typedef struct amos_pose_camera {      /* per frame: 68 bytes */
    float Rcw[9], tcw[3];              /* the frame's mTcw on entry, rotation row-major */
    float fx, fy, cx, cy, mbf;
} amos_pose_camera;

typedef struct amos_pose_result {      /* per frame: 272 bytes */
    double Rt[12];                     /* the optimised pose in double: R row-major, then t */
    float Tcw[12], Ow[3];              /* what SetPose / UpdatePoseMatrices store: rows of [R|t] as float; Ow = -Rcw^T tcw, one gemm per row in double, one rounding */
    int32_t n_edges;                   /* nInitialCorrespondences */
    int32_t n_inliers;                 /* the return value: nInitialCorrespondences - nBad */
    int32_t n_inliers_with_obs;        /* inlier edges whose point has the has_obs bit (all of them when flags_offset is -1): nmatchesMap */
    int32_t rounds;                    /* executed rounds: 0, 1 (fewer than 10 edges) or 4 */
    int32_t status;                    /* bit 0: an octave outside the table; bit 1: a match index outside the frame's points */
    int32_t iterations[4], trials[4];  /* per round: calls of the Levenberg solve, and its trial steps in all */
    double lambda[4], chi2[4];         /* at each round's end: the damping, the active robust chi2 */
} amos_pose_result;

typedef struct amos_pose_optimization {
    const amos_keypoint *d_kps;        /* [frames][capacity]: mvKeysUn */
    const float *d_u_right;            /* [frames][capacity] or NULL: every edge monocular */
    const int32_t *d_counts;           /* [frames] */
    int32_t *d_match;                  /* [frames][capacity]: index into the frame's point list or -1 (a search's output; written only with clear_outliers) */
    const void *d_points;              /* records of point_stride bytes that begin with float pos[3]: amos_map_point, amos_last_point, or a bare float[3] */
    int32_t point_stride;              /* a multiple of 4, >= 12 */
    int32_t flags_offset;              /* byte offset of the record's int32 flags (a multiple of 4), or -1: no flags */
    int32_t has_obs_bit;               /* AMOS_MAP_POINT_HAS_OBS / AMOS_LAST_POINT_HAS_OBS */
    const int32_t *point_off;          /* host, n_frames + 1 entries, ascending from >= 0: frame f owns points [point_off[f], point_off[f + 1]) */
    const amos_pose_camera *cameras;   /* host, n_frames entries */
    const float *inv_level_sigma2;     /* host, n_levels entries (mvInvLevelSigma2) */
    uint8_t *d_outlier;                /* out, [frames][capacity]: mvbOutlier */
    amos_pose_result *d_result;        /* out, [frames] */
    int32_t n_frames, capacity, n_levels;
    int32_t clear_outliers;            /* 1: the loop of Tracking.cc:1770-1791: d_match[i] = -1 and d_outlier[i] = 0 where an outlier was; 0: d_match is only read (TrackLocalMap) */
} amos_pose_optimization;
/* Asynchronous on the matcher's stream (the three host arrays are consumed before the call returns).  AMOS_ERR_INVALID, before the device
 * is touched, for a NULL handle or argument (d_u_right apart), n_frames < 1, a capacity outside 1 .. 65536, n_levels outside
 * 1 .. AMOS_MAX_LEVELS, a point_stride / flags_offset that breaks the rules above, a clear_outliers other than 0 / 1, or a point_off that
 * descends. */
int amos_match_pose_optimization_batch_device(amos_match *m, const amos_pose_optimization *s);
/* The host form for a C++ drop-in (amos-slam_amd/host/FramePoseOptimization.h): ONE frame of n features, host arrays in and out,
 * synchronous: one upload, the launch, one download.  match [n] and outlier [n] are read and written in place; points_xyz [n_points][3];
 * has_obs [n_points] (Observations() > 0) or NULL: every point counts.  The return value of PoseOptimization is result->n_inliers. */
int amos_match_pose_optimization(amos_match *m, const amos_keypoint *kps_un, const float *u_right, int n, int32_t *match, const float *points_xyz,
                                 const uint8_t *has_obs, int n_points, const amos_pose_camera *camera, const float *inv_level_sigma2, int n_levels,
                                 int clear_outliers, uint8_t *outlier, amos_pose_result *result);

/* ---------------------------------------------------------------- relocalisation search ----- */

/* Step 6 of Tracking::Relocalization's candidate loop (Tracking.cc:2732, :2756): ORBmatcher::SearchByProjection(CurrentFrame, pKF,
 * sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1731-1863) for a batch of PAIRS, one (current frame, candidate keyframe) combination each.
 * Several pairs may name the same resident frame (frame_of_pair): its keypoints, descriptors and grid are read, never written.  Every pair
 * has its own d_match row ([pairs][capacity], read and written), its own point range, camera and stats.  The index of a point in its
 * pair's list is the keyframe feature index -- what SearchByBoW(pKF, F) writes into d_match -- so the matches of both index one list and
 * the pose kernel reads it with point_stride = 64, flags_offset = 24, has_obs_bit = AMOS_RELOC_POINT_HAS_OBS.
 *
 * Already found (sAlreadyFound.count(pMP)): point j is found when d_found[j] != 0 (d_found may be NULL), and, with found_from_match, also
 * when some feature i < count has d_match[i] == j on entry (the rebuild of Tracking.cc:2752-2755).  A list that holds one MapPoint* at two
 * indices must be marked by the caller at both: the library sees indices, not pointers.
 *
 * Arithmetic (PARITY UNPINNED, like the other searches): float32, every operation rounded, nothing fused, except
 *   x3Dc = Rcw * P + tcw     one gemm per row: ((R0 P0 + R1 P1) + R2 P2) + t in double, one rounding to float
 *   invzc = (float) (1.0 / (double) zc).  There is NO invzc < 0 test: a point behind the camera is projected and searched (:1762-1770)
 *   u = ((fx * xc) * invzc) + cx;  v alike
 *   a u or v that is not finite is skipped and sets bit 0 (value 1) of the pair's status (the reference goes on to convert it to int)
 *   u < min_x || u > max_x || v < min_y || v > max_y is skipped
 *   PO = P - Ow;  dist3D = (float) sqrt(((double) PO0^2 + (double) PO1^2) + (double) PO2^2)
 *   dist3D < 0.8f * min_distance || dist3D > 1.2f * max_distance is skipped (both strict)
 *   level = number of m in [0, n_levels) with max_distance / dist3D > scale_factors[m], at most n_levels - 1: the table-count form of
 *   MapPoint::PredictScale of the local map search.  The ratio is mfMaxDistance / dist3D (MapPoint.cc:576): the 1.2f of
 *   GetMaxDistanceInvariance() enters the range test above, not the ratio.
 * Pose: with d_pose == NULL the camera's Rcw / tcw, and Ow = -Rcw^T tcw on the host, one gemm per row in double, one rounding (as
 * amos_pose_result.Ow); else pair k reads Tcw and Ow of d_pose[k] on the device, so PoseOptimization -> search -> PoseOptimization runs
 * without a host step.
 * Search: radius th * scale_factors[level]; levels level - 1 .. level + 1; no right gate.  A feature with d_match[i] >= 0, on entry or set
 * by an earlier point of this call, is skipped; best candidate only, the first wins ties; accepted when bestDist <= orb_dist (0 .. 255: the
 * reference starts from bestDist = 256 with bestIdx2 = -1, a larger value would accept index -1); no ratio test.
 * Rotation consistency (check_orientation): rotation_bin(point.angle, keysUn[best].angle), one entry per accepted point; after
 * ComputeThreeMaxima every entry of a losing bin sets its feature to -1 and lowers n_matches.  Only features matched by this call can be
 * cleared; the matches present on entry are never touched. */
typedef struct amos_reloc_point {      /* keyframe feature i of the candidate as the search reads it: 64 bytes */
    float pos[3];                      /* pKF->GetMapPoint(i)->GetWorldPos() */
    float angle;                       /* pKF->mvKeysUn[i].angle */
    float min_distance, max_distance;  /* mfMinDistance, mfMaxDistance (raw: the 0.8f / 1.2f factors are applied on the device) */
    int32_t flags;                     /* bit 0: skip (no point, or isBad()); bit 1: Observations() > 0 (for the pose kernel; the search does not read it) */
    uint8_t desc[32];                  /* pMP->GetDescriptor() */
    uint8_t pad[4];
} amos_reloc_point;
#define AMOS_RELOC_POINT_SKIP 1
#define AMOS_RELOC_POINT_HAS_OBS 2

typedef struct amos_reloc_camera {     /* per pair: 84 bytes */
    float Rcw[9], tcw[3];              /* CurrentFrame.mTcw, rotation row-major (not read when d_pose is given) */
    float fx, fy, cx, cy;
    float th;                          /* 10 / 3 in Tracking.cc:2732, :2756: finite and > 0 */
    int32_t orb_dist;                  /* 100 / 64: 0 .. 255 */
    int32_t check_orientation;         /* mbCheckOrientation */
    int32_t found_from_match;          /* 1: a point that d_match names on entry is found */
    int32_t enabled;                   /* 0: the pair's work-groups return at once; d_match is untouched, the stats are zero with skipped = 1 */
} amos_reloc_camera;

typedef struct amos_reloc_stats {      /* 32 bytes */
    int32_t n_candidates;              /* points neither skipped nor found */
    int32_t n_projected;               /* points that reached GetFeaturesInArea */
    int32_t n_matches;                 /* the return value: nadditional */
    int32_t n_researched;              /* points whose best two among the features free on entry were both taken at their turn */
    int32_t n_found;                   /* points without the skip bit that were found */
    int32_t n_occupied;                /* features i < count with d_match[i] >= 0 on entry */
    int32_t status;                    /* bit 0: a projection was not finite */
    int32_t skipped;                   /* 1: enabled was 0 */
} amos_reloc_stats;

struct amos_kf_query;                  /* include/amos_host_types.h: u, v, level, angle, descriptor */
struct amos_pose_result;

typedef struct amos_reloc_search {
    const amos_keypoint *d_kps;        /* [frames][capacity]: the current frames' undistorted keypoints (mvKeysUn) */
    const uint8_t *d_desc;             /* [frames][capacity][32] */
    const int32_t *d_counts;           /* [frames] */
    const int32_t *d_cell_start;       /* [frames][64*48+1]       (amos_frame_grid_build_batch_device) */
    const int32_t *d_items;            /* [frames][capacity] */
    const amos_reloc_point *d_points;  /* pair k owns points [point_off[k], point_off[k + 1]) */
    const int32_t *frame_of_pair;      /* host, n_pairs entries in [0, n_frames) */
    const int32_t *point_off;          /* host, n_pairs + 1 entries, ascending from >= 0 */
    const amos_reloc_camera *cameras;  /* host, n_pairs entries */
    const uint8_t *d_found;            /* one byte per point, or NULL */
    const struct amos_pose_result *d_pose; /* [pairs], or NULL: the cameras' poses */
    const float *scale_factors;        /* host, n_levels entries (mvScaleFactors) */
    struct amos_kf_query *d_query;     /* out, one per point of an enabled pair: angle and descriptor always, u / v / level where projected (else 0) */
    uint8_t *d_projected;              /* out, one per point of an enabled pair: 1 where the point reached GetFeaturesInArea */
    int32_t *d_match;                  /* in / out, [pairs][capacity]: index of the matched point inside the pair's own list, or -1 */
    amos_reloc_stats *d_stats;         /* out, [pairs] */
    int32_t n_frames, n_pairs, capacity, n_levels;
    float min_x, max_x, min_y, max_y;  /* Frame::mnMinX .. mnMaxY */
} amos_reloc_search;
/* Asynchronous on the matcher's stream (the three host arrays and the table are consumed before the call returns).  Three launches
 * (projection, window search, acceptance), and one more ahead of them when a pair has found_from_match.  AMOS_ERR_INVALID, before the device
 * is touched, for a NULL handle or required pointer, n_pairs < 1, n_frames < 1, a capacity outside 1 .. 65536, n_levels outside
 * 1 .. AMOS_MAX_LEVELS, a frame_of_pair outside [0, n_frames), a point_off that descends or starts below 0, empty bounds, an orb_dist
 * outside 0 .. 255 or a th that is not finite or not positive. */
int amos_match_reloc_batch_device(amos_match *m, const amos_reloc_search *s);
/* The host form for a C++ drop-in (amos-slam_amd/host/FrameRelocalization.h): ONE pair, host arrays in and out, synchronous: one upload (the
 * grid cells of Frame::PosInGrid are computed on the way), AssignFeaturesToGrid and the launches on the device, one download.  found
 * [n_points] or NULL; query, projected [n_points]; match [n] is read and written in place. */
int amos_match_reloc(amos_match *m, const amos_keypoint *kps_un, const uint8_t *desc, int n, const amos_reloc_point *points, int n_points,
                     const uint8_t *found, const amos_reloc_camera *camera, const float *scale_factors, int n_levels, float min_x,
                     float max_x, float min_y, float max_y, struct amos_kf_query *query, uint8_t *projected, int32_t *match /* in/out [n] */,
                     amos_reloc_stats *stats);

/* ---------------------------------------------------------------- relocalisation PnP -------- */

/* Step 3 of Tracking::Relocalization's candidate loop (Tracking.cc:2650-2713): ORB-SLAM2's PnPsolver (src/PnPsolver.cc:120-458) for a batch
 * of PAIRS (lost frame, candidate keyframe), ONE iterate() call per pair and launch, and the loop of Tracking.cc:2704-2713 behind it.  The
 * EPnP is the restated one of amos-slam_amd/csrc/amos_pnp_core.h with the pixel taken as it is: PARITY WITH THE REFERENCE'S OPENCV-BACKED
 * EPnP UNPINNED; what is pinned, bit for bit, is tests/reloc_pnp_restatement.py.
 *
 * Correspondences (the constructor): features i < d_counts[frame] in ascending order with d_bow_match[i] = j >= 0 whose point j of the
 * pair's list does not carry AMOS_RELOC_POINT_SKIP: P2D = d_kps[i].x / .y, sigma2 = level_sigma2[octave], P3D = point j's pos.  An octave
 * outside [0, n_levels) skips the feature and sets bit 0 of status, a j outside the pair's points bit 1.  More than 4096 correspondences:
 * code = -3, no other output is written.
 * SetRansacParameters(probability, min_inliers, max_iterations, 4, epsilon, th2) runs with reset = 1 (and when the carried state does not
 * belong to a solver of as many correspondences: bit 2 of status); its adjusted values come back in the result.  The reference's unseeded
 * rand() is one cv::RNG state per solver, seeded with `seed` at a reset and carried: a later call continues the stream.
 * iterate(n_iterations): the reference's loop, `while (mnIterations < maxIts || nCurrentIterations < nIterations)` included; it ends
 * early with the refined pose where Refine succeeds (more than min_inliers inliers, strictly), else with the best pose once
 * mnIterations >= maxIts (no_more) if that had min_inliers inliers, else without a pose.
 * A carried state holds inlier sets by correspondence index: d_kps, d_counts, d_bow_match, d_points and level_sigma2 of a pair must be
 * the same in every call on its state, and d_match must not be d_bow_match. */
typedef struct amos_reloc_pnp_params {   /* per pair: 64 bytes */
    float fx, fy, cx, cy;                /* the frame's camera (PnPsolver keeps them as doubles of these floats) */
    double probability;                  /* in (0, 1): 0.99 */
    int32_t min_inliers, max_iterations; /* 10, 300; max_iterations 1 .. 65536 */
    float epsilon, th2;                  /* 0.5, 5.991: finite and positive */
    int32_t n_iterations;                /* iterate's argument: 5; 1 .. 65536 */
    int32_t reset;                       /* 1: constructor + SetRansacParameters first; 0: go on from d_state */
    uint64_t seed;                       /* the generator's state at a reset */
    int32_t enabled;                     /* 0: only the result record is written (zeros, skipped = 1) */
    int32_t pad;
} amos_reloc_pnp_params;

typedef struct amos_reloc_pnp_result {   /* per pair: 104 bytes */
    float Tcw[12];                       /* rows of [R | t] as the reference stores them (double -> float); zeros without a pose */
    int32_t code;                        /* 0, or -3: more than 4096 correspondences */
    int32_t has_pose, no_more, refined;  /* !Tcw.empty(), bNoMore, the pose is Refine's */
    int32_t n_inliers;                   /* nInliers (0 without a pose) */
    int32_t n_correspondences;           /* N */
    int32_t min_inliers, max_iterations; /* mRansacMinInliers, mRansacMaxIts as SetRansacParameters adjusted them */
    int32_t iterations, iterations_call; /* mnIterations, nCurrentIterations */
    int32_t best_inliers;                /* mnBestInliers */
    int32_t status;                      /* bit 0: an octave outside the table; bit 1: a match outside the pair's points; bit 2: state restarted */
    int32_t skipped;                     /* 1: enabled was 0 */
    int32_t pad;
} amos_reloc_pnp_result;

typedef struct amos_reloc_pnp {
    const amos_keypoint *d_kps;          /* [frames][capacity]: mvKeysUn (x, y, octave are read) */
    const int32_t *d_counts;             /* [frames] */
    const int32_t *frame_of_pair;        /* host, n_pairs entries in [0, n_frames) */
    const int32_t *point_off;            /* host, n_pairs + 1 entries, ascending from >= 0 */
    const amos_reloc_point *d_points;    /* pair k owns points [point_off[k], point_off[k + 1]): the list of amos_match_reloc_batch_device */
    const int32_t *d_bow_match;          /* [pairs][capacity]: SearchByBoW(pKF, F)'s row, index into the pair's points or -1 */
    const float *level_sigma2;           /* host, n_levels entries (mvLevelSigma2) */
    const amos_reloc_pnp_params *params; /* host, n_pairs entries */
    void *d_state;                       /* in / out, [pairs] blocks of amos_reloc_pnp_state_bytes(capacity) bytes: opaque */
    amos_reloc_pnp_result *d_result;     /* out, [pairs] */
    uint8_t *d_inlier;                   /* out, [pairs][capacity]: vbInliers by feature index; all zero without a pose */
    int32_t *d_match;                    /* out with a pose, [pairs][capacity]: d_bow_match[i] where feature i is an inlier, else -1 */
    uint8_t *d_found;                    /* out with a pose, one byte per point: sFound; may be NULL */
    int32_t n_frames, n_pairs, capacity, n_levels;
} amos_reloc_pnp;
size_t amos_reloc_pnp_state_bytes(int capacity);
/* Asynchronous on the matcher's stream (the host arrays are consumed before the call returns); ONE launch, one work-group per pair.
 * AMOS_ERR_INVALID, before the device is touched, for a NULL handle or pointer (d_found apart), n_pairs < 1, n_frames < 1, a capacity
 * outside 1 .. 65536, n_levels outside 1 .. AMOS_MAX_LEVELS, a frame_of_pair outside the frames, a point_off that descends or starts below
 * 0, a camera that is not finite, a probability outside (0, 1), an epsilon or th2 that is not finite and positive, a max_iterations or
 * n_iterations outside 1 .. 65536.  The host reads d_result: it decides on no_more and on an empty pose, and fills the amos_pose_camera of
 * the optimisation that follows from Tcw. */
int amos_match_reloc_pnp_batch_device(amos_match *m, const amos_reloc_pnp *s);
/* The host form for a C++ drop-in (amos-slam_amd/host/FrameRelocalizationPnP.h): ONE pair, host arrays in and out, synchronous: one upload,
 * the launch, one download.  state: amos_reloc_pnp_state_bytes(n) bytes, read (reset = 0) and written.  inlier [n] is always written;
 * match [n] and found [n_points] only with a pose. */
int amos_match_reloc_pnp(amos_match *m, const amos_keypoint *kps_un, int n, const int32_t *bow_match, const amos_reloc_point *points, int n_points,
                         const float *level_sigma2, int n_levels, const amos_reloc_pnp_params *params, void *state, amos_reloc_pnp_result *result,
                         uint8_t *inlier, int32_t *match, uint8_t *found);

/* ---------------------------------------------------------------- bag of words --------------- */

/* Tracking::TrackReferenceKeyFrame's two steps (Tracking.cc:1736-1794) for resident frames: Frame::ComputeBoW (Frame.cc:1033-1049), which is
 * TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259), and
 * ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:230-382).  Tracking::Relocalization runs the same two calls
 * against every candidate keyframe (Tracking.cc:2595, 2634).
 *
 * The vocabulary handle is built from host arrays that hold what TemplatedVocabulary::loadFromTextFile (:1338-1424) reads: k, L, scoring,
 * weighting and, for the nodes 1 .. n_nodes - 1 in file order, parent, is_leaf, descriptor and weight (entry 0 of each array belongs to
 * the implicit root and is not read).  Creation builds the children lists in ascending node id (the file's push_back order), numbers the
 * words over the leaves in node order, and lays the tree out so that the child descriptors of one node are contiguous on the device.
 * AMOS_ERR_INVALID, before the device is touched: a NULL argument; scoring other than AMOS_BOW_L1_NORM or weighting other than
 * AMOS_BOW_TF_IDF (ORBvoc.txt's 0 / 0: nothing else is built); L outside 1 .. 10; n_nodes < 2; parent[i] < 0 or >= i; a node that is no
 * leaf and has no children (the root too) or a leaf with children; more than AMOS_BOW_MAX_CHILDREN children on one node.
 *
 * Arithmetic (PINNED: restated from the reference's loops, integers and IEEE doubles, nothing reassociated or fused):
 *   descent (:1218-1259): from the root, at each level the child with the smallest Hamming distance, compared as integers, the FIRST child
 *   of equal distances (the loop's strict d < best_d); it stops at a leaf.  word = the leaf's word id, weight = the leaf's weight.
 *   nid: the node chosen at level L - levelsup (the root's children are level 1); node 0 when L - levelsup <= 0.  When the walk ends at a
 *   leaf ABOVE that level the reference leaves nid uninitialised: here it is the leaf's node id, and bit 0 (value 1) of the frame's status
 *   is set (whether or not the word is stopped).
 *   a feature whose word is stopped (not weight > 0, :1157) enters neither vector; its d_feat_word is AMOS_BOW_NO_WORD.
 *   FeatureVector (FeatureVector.cpp addFeature): node ids ascending, the features of a node ascending.
 *   BowVector (:1145-1162, BowVector.cpp:34-46): the value of a word is the double sum of its weight over its features in ascending
 *   feature order, starting FROM the first weight (v, then v + w, ...).  normalize (BowVector.cpp:62-84): norm = the double sum of
 *   fabs(value) from 0.0 in ascending word order, one addition per word; when norm > 0 every value becomes value / norm (correctly rounded). */
typedef struct amos_bow amos_bow;
#define AMOS_BOW_L1_NORM 0            /* DBoW2::ScoringType */
#define AMOS_BOW_TF_IDF 0             /* DBoW2::WeightingType */
#define AMOS_BOW_MAX_CHILDREN 32
#define AMOS_BOW_MAX_CAPACITY 16384   /* features per frame of a transform: its sort keys, 8 bytes each, live in 128 KB of the CU's 160 KB LDS */
#define AMOS_BOW_NO_WORD 0xFFFFFFFFu
#define AMOS_BOW_STATUS_EARLY_LEAF 1  /* amos_bow_stats.status bit 0 */

typedef struct amos_bow_stats {        /* 16 bytes */
    int32_t n_words;                   /* entries of the BowVector */
    int32_t n_nodes;                   /* entries of the FeatureVector */
    int32_t n_stopped;                 /* features whose word is stopped */
    int32_t status;                    /* bit 0: a walk reached a leaf above level L - levelsup */
} amos_bow_stats;

int amos_bow_create(int device, void *stream, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent,
                    const uint8_t *is_leaf, const uint8_t *desc, const double *weight, amos_bow **out);
void amos_bow_destroy(amos_bow *b);
int amos_bow_sync(amos_bow *b);
void *amos_bow_stream(amos_bow *b);
/* The argument checks of amos_bow_create alone (no device is touched): AMOS_OK or AMOS_ERR_INVALID; *n_words, if not NULL, gets the word count. */
int amos_bow_check(int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent, const uint8_t *is_leaf, int32_t *n_words);
/* The transform of n_frames resident frames: descriptors d_desc [frames][capacity][32], counts d_counts [frames] (a count above capacity is
 * read as capacity, one below 0 as 0).  Two launches, asynchronous on the handle's stream; nothing returns to the host.  Outputs, per frame f:
 *   d_feat_word, d_feat_node [frames][capacity]   per feature: its word id (AMOS_BOW_NO_WORD when stopped) and its nid
 *   d_n_nodes [frames]; d_node_ids [frames][capacity] ascending; d_node_off [frames][capacity + 1], n_nodes + 1 entries;
 *   d_node_idx [frames][capacity] feature indices, ascending inside a node: the FeatureVector as the CSR amos_bow_view reads
 *   d_n_words [frames]; d_words [frames][capacity] ascending; d_word_weights [frames][capacity] doubles: the BowVector
 *   d_stats [frames]
 * Entries past a frame's counts (features, nodes + 1 offsets, indexed features, words) are not written.  capacity 1 ..
 * AMOS_BOW_MAX_CAPACITY, AMOS_ERR_CAPACITY above it; AMOS_ERR_INVALID for a NULL argument, n_frames < 1 or levelsup < 0. */
int amos_bow_transform_batch_device(amos_bow *b, const uint8_t *d_desc, const int32_t *d_counts, int n_frames, int capacity, int levelsup,
                                    uint32_t *d_feat_word, uint32_t *d_feat_node, int32_t *d_n_nodes, uint32_t *d_node_ids,
                                    int32_t *d_node_off, int32_t *d_node_idx, int32_t *d_n_words, uint32_t *d_words,
                                    double *d_word_weights, amos_bow_stats *d_stats);
/* The host form: ONE frame of n descriptors, host arrays in and out, synchronous: one upload, the two launches, one download.  feat_word,
 * feat_node, node_ids, node_idx, words, word_weights hold n entries, node_off n + 1; entries past the counts in stats are left as they are. */
int amos_bow_transform(amos_bow *b, const uint8_t *desc, int n, int levelsup, uint32_t *feat_word, uint32_t *feat_node, uint32_t *node_ids,
                       int32_t *node_off, int32_t *node_idx, uint32_t *words, double *word_weights, amos_bow_stats *stats);

/* ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:230-382) for n_pairs (keyframe slot, frame slot) pairs of resident
 * frames whose FeatureVectors are the transform's CSR.  Two launches (eight lanes per keyframe feature find the best two frame features
 * of its node, taken or not; ONE wave per pair then runs the reference's sequential loop), nothing returns to the host.
 *   Only nodes present on both sides take part.  Keyframe features are visited in FeatureVector order (nodes ascending, in-node order);
 *   one without a good map point (d_has_point, NULL = all have one) is skipped.  Its candidates are the frame features of the same node
 *   that no earlier keyframe feature was matched to; best and second best start at 256 under strict <, the first of equal distances
 *   wins.  Accepted when best <= AMOS_TH_LOW and (float) best < nn_ratio * (float) second: d_match[best feature] = the keyframe feature.
 *   A frame feature is never overwritten.  Rotation consistency (check_orientation): rot = angleKF - angleF, + 360.0f when rot < 0,
 *   bin = (int) roundf(rot * (30 / 360.0f)), 30 becomes 0; one entry per accepted match; every entry of a bin that is not one of
 *   ComputeThreeMaxima's three (see the motion-model search) sets its frame feature to -1 and lowers n_matches.
 *   n_researched counts the keyframe features whose best or second best over ALL frame features of the node (the first of equal
 *   distances in list order each) had been taken when their turn came: their list is searched again against the taken features.
 *   A feature index outside [0, count) in a FeatureVector is never dereferenced: such a keyframe feature is skipped and sets bit 0 of the
 *   pair's status, such a frame feature is no candidate. */
typedef struct amos_bow_search_stats { /* 16 bytes */
    int32_t n_queries;                 /* keyframe features that reached the candidate loop: in a shared node, with a map point */
    int32_t n_matches;                 /* the search's return value */
    int32_t n_researched;
    int32_t status;                    /* bit 0: a keyframe feature index outside the keyframe's features */
} amos_bow_search_stats;

typedef struct amos_bow_search {
    const amos_keypoint *d_kps;        /* [frames][capacity]: KF mvKeysUn, F mvKeys (only .angle is read) */
    const uint8_t *d_desc;             /* [frames][capacity][32] */
    const int32_t *d_counts;           /* [frames] */
    const int32_t *d_n_nodes;          /* [frames]                 the FeatureVectors (amos_bow_transform_batch_device) */
    const uint32_t *d_node_ids;        /* [frames][capacity] */
    const int32_t *d_node_off;         /* [frames][capacity + 1] */
    const int32_t *d_node_idx;         /* [frames][capacity] */
    const uint8_t *d_has_point;        /* [frames][capacity] or NULL: vpMapPointsKF[i] && !isBad() */
    const int32_t *d_pairs_kf, *d_pairs_f; /* [n_pairs] frame slots */
    int32_t *d_match;                  /* out, [n_pairs][capacity]: the keyframe feature matched to frame feature i, or -1 (reset by the call) */
    amos_bow_search_stats *d_stats;    /* out, [n_pairs] */
    int32_t n_pairs, capacity;         /* capacity 1 .. 65536 */
    float nn_ratio;
    int32_t check_orientation;
} amos_bow_search;
/* Asynchronous on the matcher's stream.  AMOS_ERR_INVALID, before the device is touched, for a NULL handle or argument (d_has_point apart),
 * n_pairs < 1 or a capacity out of range. */
int amos_match_bow_batch_device(amos_match *m, const amos_bow_search *s);
struct amos_bow_view;                  /* include/amos_host_types.h */
/* The host form: one keyframe and one frame as amos_bow_view, host arrays in and out, synchronous: one upload, the two launches, one
 * download.  matches_f holds f->n entries.  AMOS_ERR_INVALID also for a view whose node ids do not ascend, whose offsets do not ascend from 0
 * to at most n, or whose feature indices leave [0, n). */
int amos_match_bow(amos_match *m, const struct amos_bow_view *kf, const struct amos_bow_view *f, float nn_ratio, int check_orientation,
                   int32_t *matches_f, amos_bow_search_stats *stats);

/* The two searches over a PAIR of keyframes' FeatureVectors, for n_pairs (keyframe-1 slot, keyframe-2 slot) pairs of resident frames:
 * ORBmatcher::SearchForTriangulation (ORBmatcher.cc:810-1009, CheckDistEpipolarLine :188-215), which LocalMapping::CreateNewMapPoints
 * calls once per neighbour of the current keyframe (LocalMapping.cc:324), and ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (:656-799),
 * which LoopClosing::ComputeSim3 calls once per loop candidate (LoopClosing.cc:346).  Two launches each (eight lanes per list position of
 * keyframe 1 find the best two keyframe-2 features of its node, taken or not; ONE wave per pair then runs the reference's sequential
 * loop with the taken keyframe-2 features as a bitmap), nothing returns to the host.
 *   Common: only nodes present on both sides take part; keyframe-1 features are visited in FeatureVector order.  d_match12[i] = the
 *   keyframe-2 feature matched to keyframe-1 feature i, or -1 (reset by the call; vMatchedPairs is its ascending scan); a keyframe-2
 *   feature is matched once.  Rotation consistency (check_orientation): rot = angle1 - angle2 and the bins as in the search above; one
 *   entry per accepted keyframe-1 feature; an entry of a losing bin sets d_match12[idx1] = -1 and lowers n_matches.  n_queries counts the
 *   keyframe-1 features that reach the candidate loop.  A keyframe-1 index outside [0, count) is skipped and sets status bit 0, a
 *   keyframe-2 index outside is no candidate.
 *   SearchByBoW(KF, KF): d_has_point[i] = the feature has a good map point (NULL = all have one); a keyframe-1 feature without one is
 *   skipped, a keyframe-2 feature without one is no candidate.  Best and second best start at 256 under strict <, the FIRST of equal
 *   distances wins; accepted when best < AMOS_TH_LOW (strictly) and (float) best < nn_ratio * (float) second.  n_researched counts
 *   the queries whose best or second best over all candidates of the node had been taken when their turn came.
 *   SearchForTriangulation: d_has_point[i] = GetMapPoint(i) != NULL (NULL = none has one): such a feature is skipped on side 1 and is
 *   no candidate on side 2.  A feature is stereo when d_u_right[i] >= 0 (NULL: none is); under only_stereo a mono feature is skipped /
 *   no candidate.  A candidate must have dist <= AMOS_TH_LOW; when both features are mono it must NOT lie near the epipole:
 *   (ex - x2) * (ex - x2) + (ey - y2) * (ey - y2) < 100 * scale_factors[octave2] rejects (float32, every operation rounded in source
 *   order); and it must pass the line test: a = x1 * F[0] + y1 * F[3] + F[6], b = x1 * F[1] + y1 * F[4] + F[7], c = x1 * F[2] + y1 * F[5]
 *   + F[8], num = a * x2 + b * y2 + c, den = a * a + b * b, den == 0 rejects, dsqr = num * num / den (float32, left to right), accepted
 *   when (double) dsqr < 3.84 * (double) level_sigma2[octave2].  The reference's running bound (dist > bestDist skips, an equal distance
 *   passes) makes the result the LAST candidate of the smallest distance in list order among those that pass every test and are not
 *   taken; there is no ratio test.  When that candidate over ALL passing candidates is taken the next one in the same order (if any)
 *   is the result when it is free; when both are taken the list is searched again against the taken features and the query counts in
 *   n_researched.  A keyframe-2 keypoint that passes the other filters and whose octave is outside [0, n_levels) is no candidate and
 *   sets status bit 1. */
typedef struct amos_kf_pair_search {
    const amos_keypoint *d_kps;        /* [frames][capacity]: mvKeysUn (x, y, angle, octave are read) */
    const uint8_t *d_desc;             /* [frames][capacity][32] */
    const int32_t *d_counts;           /* [frames] */
    const int32_t *d_n_nodes;          /* [frames]                 the FeatureVectors (amos_bow_transform_batch_device) */
    const uint32_t *d_node_ids;        /* [frames][capacity] */
    const int32_t *d_node_off;         /* [frames][capacity + 1] */
    const int32_t *d_node_idx;         /* [frames][capacity] */
    const uint8_t *d_has_point;        /* [frames][capacity] or NULL.  SearchByBoW(KF, KF): a good map point (NULL = all);
                                          SearchForTriangulation: any map point (NULL = none) */
    const float *d_u_right;            /* [frames][capacity] or NULL (monocular).  SearchForTriangulation only */
    const int32_t *d_pairs_1, *d_pairs_2; /* [n_pairs] frame slots */
    int32_t *d_match12;                /* out, [n_pairs][capacity] */
    amos_bow_search_stats *d_stats;    /* out, [n_pairs]; status bit 0: a keyframe-1 index outside the keyframe, bit 1: an octave outside */
    int32_t n_pairs, capacity;         /* capacity 1 .. 65536 */
} amos_kf_pair_search;
typedef struct amos_kf_geometry {      /* 44 bytes, per pair: the caller's, from the two poses */
    float f12[9];                      /* the fundamental matrix, row-major */
    float ex, ey;                      /* keyframe 1's camera centre in keyframe 2's image (ORBmatcher.cc:818-825) */
} amos_kf_geometry;
/* Asynchronous on the matcher's stream.  AMOS_ERR_INVALID, before the device is touched, for a NULL handle or argument (d_has_point and
 * d_u_right apart), n_pairs < 1, a capacity out of range or n_levels outside 1 .. AMOS_MAX_LEVELS.  d_geometry [n_pairs],
 * d_scale_factors and d_level_sigma2 [n_levels] are device arrays. */
int amos_match_bow_kf_batch_device(amos_match *m, const amos_kf_pair_search *s, float nn_ratio, int check_orientation);
int amos_match_triangulation_batch_device(amos_match *m, const amos_kf_pair_search *s, const amos_kf_geometry *d_geometry,
                                          const float *d_scale_factors, const float *d_level_sigma2, int n_levels, int only_stereo,
                                          int check_orientation);
/* The host forms, synchronous: one upload, the two launches, one download.  amos_match_bow_kf: two views; match12 holds k1->n entries.
 * amos_match_triangulation: ONE keyframe 1 against n2 keyframes 2 (keyframe 1 is staged once); geometry holds n2 records, scale_factors
 * and level_sigma2 n_levels floats (host arrays); match12 holds n2 rows of k1->n entries, stats n2.  AMOS_ERR_INVALID, before the device
 * is touched, for a NULL argument, n2 < 1, n_levels out of range or a view that amos_match_bow rejects. */
int amos_match_bow_kf(amos_match *m, const struct amos_bow_view *k1, const struct amos_bow_view *k2, float nn_ratio, int check_orientation,
                      int32_t *match12, amos_bow_search_stats *stats);
int amos_match_triangulation(amos_match *m, const struct amos_bow_view *k1, const struct amos_bow_view *const *k2s, int n2,
                             const amos_kf_geometry *geometry, const float *scale_factors, const float *level_sigma2, int n_levels,
                             int only_stereo, int check_orientation, int32_t *match12, amos_bow_search_stats *stats);

/* ---------------------------------------------------------------- new map points -------------- */

/* What LocalMapping::CreateNewMapPoints (LocalMapping.cc:313-626) does with the matches of SearchForTriangulation, for the n_pairs
 * (keyframe-1 slot, keyframe-2 slot) pairs of one search call: per match the parallax of the two rays, the 4 x 4 SVD or
 * KeyFrame::UnprojectStereo, the two depth signs, the two reprojection gates and the scale-consistency gate (:424-597).  It reads
 * d_match12 exactly as amos_match_triangulation_batch_device left it on the device: the two calls go to the matcher's stream back to
 * back, no copy and no synchronisation between them.  What remains on the host is `new MapPoint` and the observation bookkeeping
 * (:601-623) over the records of d_new.  The arithmetic is amos-slam_amd/csrc/amos_new_points_core.h (its header lists the convention
 * that fixes each expression, the reference's quirks that are kept and what a NaN does): PARITY WITH THE REFERENCE'S OPENCV-BACKED
 * ARITHMETIC UNPINNED; what is pinned, bit for bit, is tests/new_points_restatement.py.  The monocular median-depth gate is out of scope.
 *
 * Per pair: keyframe-1 features i < min(d_counts[slot 1], capacity) with j = d_match12[pair][i] != -1 are the matches; a j outside
 * [0, min(d_counts[slot 2], capacity)) is skipped and sets status bit 0.  Every match gets a verdict (AMOS_NEW_POINT_*); an octave
 * outside [0, n_levels) on either side gets OCTAVE and sets status bit 1 (the reference would index its tables out of range).
 *
 * THE CLAIM RULE (where this entry departs from the reference, by definition).  The reference searches neighbour k + 1 after neighbour
 * k's new points were added to the current keyframe, so a keyframe-1 feature that already produced a point is skipped there; the
 * one-call search for all neighbours cannot see that.  Here: among the enabled pairs that share a keyframe-1 slot, taken in pair order,
 * a keyframe-1 feature yields at most ONE point; the winner is the first pair in which its match is accepted (verdict 0, 1 or 2), an
 * accepted match of that feature in a later pair gets CLAIMED.  The reference's later search would not have visited the feature at all,
 * which could have freed its keyframe-2 candidate for another feature: the one-call search does not replay that; it is a property of the
 * merged search.  Two enabled pairs with the same keyframe-2 slot are outside the LocalMapping shape: AMOS_ERR_INVALID.
 *
 * Outputs.  d_new[pair][0 .. n_new): the accepted matches of the pair, compact, in ascending idx1 -- the order in which the reference
 * creates its MapPoints, so mnIds follow it; records at and beyond n_new are NOT written.  d_verdict[pair][0 .. capacity) (may be
 * NULL): the verdict of feature i, -1 without a match; written over the whole row.  d_stats[pair]: n_matches (the matches with a
 * verdict), n_new, n_verdict[v] and status.  A pair with enabled[pair] == 0 (the neighbour failed the baseline gate :361-374) writes zero
 * stats and a row of -1; a pair slot outside [0, n_frames) does the same and sets status bit 2.
 * TWO launches: k_new_points_solve (256 features x pairs per work-group, the matches compacted so that the lanes that run the Jacobi
 * are dense, one match per lane) and k_new_points_emit (one work-group per pair: the claim rule, the compaction, the sums). */
#define AMOS_NEW_POINT_TRIANGULATED 0   /* accepted, from the SVD */
#define AMOS_NEW_POINT_UNPROJECTED_1 1  /* accepted, UnprojectStereo of keyframe 1 */
#define AMOS_NEW_POINT_UNPROJECTED_2 2  /* accepted, UnprojectStereo of keyframe 2 */
#define AMOS_NEW_POINT_LOW_PARALLAX 3   /* the final `else continue` (:499) */
#define AMOS_NEW_POINT_W_ZERO 4
#define AMOS_NEW_POINT_BEHIND_1 5
#define AMOS_NEW_POINT_BEHIND_2 6
#define AMOS_NEW_POINT_REPROJECTION_1 7
#define AMOS_NEW_POINT_REPROJECTION_2 8
#define AMOS_NEW_POINT_DISTANCE_ZERO 9
#define AMOS_NEW_POINT_SCALE 10
#define AMOS_NEW_POINT_CLAIMED 11
#define AMOS_NEW_POINT_OCTAVE 12
#define AMOS_NEW_POINT_VERDICTS 13
#define AMOS_NEW_POINTS_BAD_MATCH 1     /* status bits */
#define AMOS_NEW_POINTS_BAD_OCTAVE 2
#define AMOS_NEW_POINTS_BAD_SLOT 4
#define AMOS_NEW_POINTS_MAX_PAIRS 64
typedef struct amos_kf_camera {         /* per keyframe: 96 bytes */
    float Rcw[9], tcw[3];               /* GetRotation(), GetTranslation() */
    float Ow[3];                        /* GetCameraCenter() */
    float fx, fy, cx, cy, invfx, invfy;
    float mb, mbf;
    float scale_factor;                 /* mfScaleFactor */
} amos_kf_camera;
typedef struct amos_new_point {         /* 24 bytes */
    int32_t idx1, idx2;
    float x, y, z;                      /* x3D */
    int32_t verdict;                    /* 0, 1 or 2: where x3D came from */
} amos_new_point;
typedef struct amos_new_points_stats {  /* 64 bytes */
    int32_t n_matches, n_new;
    int32_t n_verdict[AMOS_NEW_POINT_VERDICTS];
    int32_t status;
} amos_new_points_stats;
typedef struct amos_new_points {
    const amos_keypoint *d_kps;         /* [frames][capacity]: mvKeysUn (the arrays of amos_kf_pair_search) */
    const amos_keypoint *d_kps_raw;     /* [frames][capacity]: mvKeys (x and y are read, by UnprojectStereo), or NULL = d_kps (rectified input) */
    const int32_t *d_counts;            /* [frames] */
    const float *d_u_right;             /* [frames][capacity] or NULL (no feature is stereo) */
    const float *d_depth;               /* [frames][capacity]: mvDepth; may be NULL when d_u_right is */
    const int32_t *d_pairs_1, *d_pairs_2; /* [n_pairs] frame slots */
    const int32_t *d_match12;           /* [n_pairs][capacity]: the search's result, in place */
    const float *d_scale_factors, *d_level_sigma2; /* [n_levels] */
    const amos_kf_camera *cameras;      /* host, n_frames entries */
    const int32_t *pairs_1, *pairs_2;   /* host, [n_pairs]: the slots that d_pairs_1 / d_pairs_2 hold */
    const uint8_t *enabled;             /* host, [n_pairs]: 0 = the neighbour failed the baseline gate; NULL = all enabled */
    amos_new_point *d_new;              /* out, [n_pairs][capacity] */
    int32_t *d_verdict;                 /* out, [n_pairs][capacity], or NULL */
    amos_new_points_stats *d_stats;     /* out, [n_pairs] */
    int32_t n_frames, n_pairs, capacity, n_levels; /* n_pairs 1 .. 64, capacity 1 .. 65536, n_levels 1 .. AMOS_MAX_LEVELS */
} amos_new_points;
/* Asynchronous on the matcher's stream.  AMOS_ERR_INVALID, before the device is touched, for a NULL handle or argument (d_kps_raw,
 * d_u_right, d_depth with it, enabled and d_verdict apart), a count out of range, a host pair slot outside [0, n_frames), two enabled
 * pairs with the same keyframe-2 slot, or a camera of an enabled pair that is not finite or has fx, fy <= 0. */
int amos_match_new_points_batch_device(amos_match *m, const amos_new_points *s);
/* LocalMapping::ComputeF12 (:743-779), the epipole of ORBmatcher.cc:818-825 and the stereo / RGB-D baseline gate (:361-374) from the two
 * keyframes' records: the host compilation of amos_new_points_core.h's pair_geometry.  Returns 1, or 0 when |Ow2 - Ow1| < c2->mb (the
 * neighbour is skipped; g is written either way), AMOS_ERR_INVALID for a NULL argument. */
int amos_kf_geometry_from_poses(const amos_kf_camera *c1, const amos_kf_camera *c2, amos_kf_geometry *g);
/* The host form, synchronous: ONE keyframe 1 against n2 neighbours from host arrays.  Geometry and gate per neighbour
 * (amos_kf_geometry_from_poses); gated neighbours are dropped from the call, their stats are zero; ONE upload (keyframe 1 staged once),
 * the search's two launches, the two launches above, ONE download.  cams2, kps_raw2, depth2: n2 entries; kps_raw1 / kps_raw2[v] (the raw
 * keypoints, NULL = the view's keys) and depth1 / depth2[v] (NULL: allowed for a view without u_right) hold the view's n entries.
 * new_points holds n2 rows of k1->n records (row v: stats[v].n_new valid ones), stats n2.  AMOS_ERR_INVALID, before the device is
 * touched, for a NULL argument, n2 outside 1 .. 64, n_levels out of range, a view that amos_match_bow rejects or a stereo view without
 * depths. */
int amos_match_new_points(amos_match *m, const struct amos_bow_view *k1, const struct amos_bow_view *const *k2s, int n2,
                          const amos_kf_camera *cam1, const amos_kf_camera *cams2, const amos_keypoint *kps_raw1,
                          const amos_keypoint *const *kps_raw2, const float *depth1, const float *const *depth2, const float *scale_factors,
                          const float *level_sigma2, int n_levels, int only_stereo, int check_orientation, amos_new_point *new_points,
                          amos_new_points_stats *stats);

/* ---------------------------------------------------------------- loop-closing Sim3 ----------- */

/* Step 2 of LoopClosing::ComputeSim3's candidate loop (LoopClosing.cc:389-447): ORB-SLAM2's Sim3Solver (src/Sim3Solver.cc:48-523: the
 * constructor, SetRansacParameters, iterate, ComputeSim3 after Horn 1987, CheckInliers) for a batch of PAIRS (keyframe-1 slot, keyframe-2
 * slot) of resident keyframes, ONE iterate() call per pair and launch, and the loop of LoopClosing.cc:440-447 behind it.  The arithmetic is
 * amos-slam_amd/csrc/amos_sim3_core.h (its header lists the convention that fixes each cv::Mat expression): PARITY WITH THE REFERENCE'S
 * OPENCV-BACKED ARITHMETIC UNPINNED; what is pinned, bit for bit, is tests/sim3_restatement.py.
 *
 * Correspondences (the constructor): keyframe-1 features i1 < d_counts[slot 1] in ascending order with d_match12[i1] = j >= 0 whose point
 * records d_points[slot 1][i1] and d_points[slot 2][j] do not carry AMOS_SIM3_POINT_SKIP (no point, or isBad()).  X3Dc = Rcw * pos + tcw
 * with each keyframe's camera, the image points by FromCameraToImage, maxErr = (float)(9.210 * (double) level_sigma2[octave]) with the
 * octaves of d_kps[slot 1][i1] and d_kps[slot 2][j].  An octave outside [0, n_levels) skips the feature and sets bit 0 of status, a j
 * outside [0, d_counts[slot 2]) skips it and sets bit 1.  More than 2048 correspondences: code = -3; a slot outside [0, n_frames):
 * code = -4; with either no other output is written.
 * SetRansacParameters(probability, min_inliers, max_iterations) runs with reset = 1 (and when the carried state is not a solver of as
 * many correspondences: bit 2 of status; a reset does not read the state); min_inliers and fix_scale of that call are kept in the state.
 * The reference's unseeded rand() is one cv::RNG state per solver, seeded with `seed` at a reset and carried; every iteration consumes
 * exactly three draws.
 * iterate(n_iterations): N < min_inliers gives no_more at once, nothing drawn.  The loop runs while mnIterations < max_iterations (as
 * adjusted) and nCurrentIterations < n_iterations.  An iteration whose inlier count is >= mnBestInliers becomes the best (the LAST of
 * equal maxima stands); the call ends with that Sim3 at the first one that becomes the best with more than min_inliers inliers
 * (strictly), and later iterations leave no trace.  Without a Sim3, no_more is set when mnIterations >= max_iterations.  A hypothesis whose
 * quaternion has an imaginary part of norm exactly 0 has no inliers (the reference scores a NaN rotation there).  NaN is stored as
 * 0x7FC00000.
 * A carried state holds the best inlier set by correspondence index: the inputs of a pair must be the same in every call on its state,
 * and d_match_out must not be d_match12. */
typedef struct amos_sim3_point {        /* a keyframe's map point by feature: 16 bytes */
    float pos[3];                       /* GetWorldPos() */
    int32_t flags;                      /* bit 0 (AMOS_SIM3_POINT_SKIP): no point, or isBad() */
} amos_sim3_point;
#define AMOS_SIM3_POINT_SKIP 1

typedef struct amos_sim3_camera {       /* per keyframe: 64 bytes */
    float Rcw[9], tcw[3];               /* GetRotation(), GetTranslation() */
    float fx, fy, cx, cy;               /* mK */
} amos_sim3_camera;

typedef struct amos_sim3_params {       /* per pair: 40 bytes */
    double probability;                 /* in (0, 1): 0.99 */
    int32_t min_inliers, max_iterations; /* 20, 300 (LoopClosing.cc:390); min_inliers >= 3, max_iterations 1 .. 65536 */
    int32_t n_iterations;               /* iterate's argument: 5; 1 .. 65536 */
    int32_t fix_scale;                  /* mbFixScale */
    int32_t reset;                      /* 1: constructor + SetRansacParameters first; 0: go on from d_state */
    int32_t enabled;                    /* 0: only the result record is written (zeros, skipped = 1) */
    uint64_t seed;                      /* the generator's state at a reset */
} amos_sim3_params;

typedef struct amos_sim3_result {       /* per pair: 160 bytes */
    float R12[9], t12[3], s12, T12[16]; /* mBestRotation, mBestTranslation, mBestScale, mBestT12 row-major; zeros without a Sim3 */
    int32_t code;                       /* 0; -3: more than 2048 correspondences; -4: a slot outside the frames */
    int32_t has_sim3, no_more;          /* !Scm.empty(), bNoMore */
    int32_t n_inliers;                  /* nInliers (0 without a Sim3) */
    int32_t n_correspondences;          /* N */
    int32_t max_iterations;             /* mRansacMaxIts as SetRansacParameters adjusted it */
    int32_t iterations, iterations_call; /* mnIterations, nCurrentIterations */
    int32_t best_inliers;               /* mnBestInliers */
    int32_t status;                     /* bit 0: an octave outside the table; bit 1: a match outside keyframe 2; bit 2: state restarted */
    int32_t skipped;                    /* 1: enabled was 0 */
} amos_sim3_result;

typedef struct amos_sim3 {
    const amos_keypoint *d_kps;         /* [frames][capacity]: mvKeysUn (octave is read) */
    const int32_t *d_counts;            /* [frames] */
    const amos_sim3_point *d_points;    /* [frames][capacity]: GetMapPointMatches() by feature */
    const amos_sim3_camera *cameras;    /* host, n_frames entries */
    const int32_t *d_pairs_1, *d_pairs_2; /* [n_pairs] frame slots: the arrays of amos_kf_pair_search */
    const int32_t *d_match12;           /* [pairs][capacity]: SearchByBoW(KF, KF)'s rows, read in place */
    const float *level_sigma2;          /* host, n_levels entries (mvLevelSigma2) */
    const amos_sim3_params *params;     /* host, n_pairs entries */
    void *d_state;                      /* in / out, [pairs] blocks of amos_sim3_state_bytes(capacity) bytes: opaque */
    amos_sim3_result *d_result;         /* out, [pairs] */
    uint8_t *d_inlier;                  /* out, [pairs][capacity]: vbInliers by keyframe-1 feature; always written, all zero without a Sim3 */
    int32_t *d_match_out;               /* out with a Sim3, [pairs][capacity]: d_match12[i1] where i1 is an inlier, else -1: the row
                                           SearchBySim3 starts from */
    int32_t n_frames, n_pairs, capacity, n_levels;
} amos_sim3;
size_t amos_sim3_state_bytes(int capacity);
/* Asynchronous on the matcher's stream (the host arrays are consumed before the call returns); ONE launch, one work-group per pair.
 * AMOS_ERR_INVALID, before the device is touched, for a NULL handle or pointer, n_pairs < 1, n_frames < 1, a capacity outside 1 .. 65536,
 * n_levels outside 1 .. AMOS_MAX_LEVELS, a camera that is not finite, a probability outside (0, 1), min_inliers < 3 (so that
 * N >= min_inliers always leaves three indices to draw, which the reference takes for granted), a max_iterations or n_iterations
 * outside 1 .. 65536.  The host reads d_result; rows and flags stay on the device for SearchBySim3 and OptimizeSim3. */
int amos_match_sim3_batch_device(amos_match *m, const amos_sim3 *s);
/* The host form for a C++ drop-in (amos-slam_amd/host/KeyFrameSim3.h): ONE pair, host arrays in and out, synchronous: one upload, the
 * launch, one download.  Keyframe 1: kps1 / points1 [n1]; keyframe 2: kps2 / points2 [n2]; cameras [2]; match12 [n1].  state:
 * amos_sim3_state_bytes(n1) bytes, read (reset = 0) and written.  inlier [n1] is always written, match_out [n1] only with a Sim3. */
int amos_match_sim3(amos_match *m, const amos_keypoint *kps1, const amos_sim3_point *points1, int n1, const amos_keypoint *kps2,
                    const amos_sim3_point *points2, int n2, const amos_sim3_camera *cameras, const int32_t *match12, const float *level_sigma2,
                    int n_levels, const amos_sim3_params *params, void *state, amos_sim3_result *result, uint8_t *inlier, int32_t *match_out);

/* ---------------------------------------------------------------- loop-closing Sim3 search ---- */

/* Step 3 of LoopClosing::ComputeSim3's candidate loop (LoopClosing.cc:454): ORBmatcher::SearchBySim3 (ORBmatcher.cc:1314-1555) for a batch
 * of PAIRS of resident keyframes.  Pair p is keyframe slot d_pairs_1[p] (KF1, the current keyframe), slot d_pairs_2[p] (KF2, the candidate)
 * -- the arrays of amos_kf_pair_search and amos_sim3 -- and one Sim3.  N1 and N2 are min(d_counts[slot], capacity).  TWO launches: direction
 * 1 (KF1's points into KF2), then direction 2 with the agreement pass; nothing returns to the host.  PARITY WITH THE REFERENCE'S
 * OPENCV-BACKED ARITHMETIC UNPINNED; what is pinned, entry for entry, is tests/sim3_search_restatement.py.
 *
 * The Sim3 of a pair: pairs[p] (host), or with d_sim3 != NULL row p of the solver's amos_sim3_result array, read on the device (R12, t12, s12
 * are its first 13 floats); pairs[p] still supplies th and enabled.  A pair with enabled == 0, or whose d_sim3 row has has_sim3 == 0 or
 * code != 0, is SKIPPED: only its stats record is written (skipped = 1, counts 0), its rows in every output array are left untouched and
 * its d_match12 row is not read (the solver writes d_match_out only with a Sim3).  A slot outside [0, n_frames): code = -4 in the stats
 * record, nothing else is written for that pair.
 *
 * The row: d_match12 [pairs][capacity] in, d_match_out [pairs][capacity] out; d_match_out == d_match12 is allowed (the chained use behind
 * amos_match_sim3_batch_device).  Entry i1 < N1: -1 free; j in [0, N2): vpMatches12[i1] is KF2's point at feature j (vbAlreadyMatched1[i1]
 * and vbAlreadyMatched2[j]); any other value: matched, but GetIndexInKeyFrame(pKF2) is outside [0, N2) (vbAlreadyMatched1[i1] only;
 * AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE for a drop-in's use).  On return d_match_out[i1] is the input entry, or idx2 where the agreement pass
 * accepted (i1, idx2), which can only happen where the entry was -1.  Entries from N1 on are copied when the arrays differ, otherwise ignored.
 *
 * Hops (:1333-1335):  sR12[r][c] = (float) ((double) s12 * R12[r][c]);  sR21[r][c] = (float) ((1.0 / (double) s12) * R12[c][r]);
 *   t21[r] = (float) (-(((double) sR21[r][0] * t12[0] + (double) sR21[r][1] * t12[1]) + (double) sR21[r][2] * t12[2]));  t12 as given.
 * One direction (:1367-1449 into KF2 with (R1w, t1w) then (sR21, t21); :1456-1533 into KF1 with (R2w, t2w) then (sR12, t12)), for every
 * source feature that has a point without AMOS_MAP_POINT_SKIP and is not already matched on its side:
 *   pc = hop (Rfw * P + tfw)   two gemms: per row ((R0 P0 + R1 P1) + R2 P2) + t in double, one rounding to float;  pc.z < 0.0f is out
 *   invz = 1.0f / z;  x = X * invz;  u = fx * x + cx;  v alike, with KF1'S INTRINSICS IN BOTH DIRECTIONS (:1318-1321); every operation
 *   rounded, nothing fused
 *   KeyFrame::IsInImage: u >= min_x && u < max_x && v >= min_y && v < max_y; a projection that is not finite fails it
 *   dist3D = (float) sqrt(((double) X^2 + (double) Y^2) + (double) Z^2) of pc (cv::norm)
 *   dist3D < 0.8f * min_distance || dist3D > 1.2f * max_distance is out;  there is no viewing-angle test
 *   level = the table form of MapPoint::PredictScale (see "local map search" and "fuse search")
 * Search: exactly the AMOS_FUSE_SIM3 search with radius th * scale_factors[level]: KeyFrame::GetFeaturesInArea without a level filter,
 * octaves level - 1 .. level, no chi-square gate, the nearest descriptor by strict < in CSR order, accepted at bestDist <= AMOS_TH_HIGH.
 * The results are vnMatch1[i1] and vnMatch2[i2], each the accepted feature or -1.
 * Agreement (:1539-1552): i1 takes idx2 = vnMatch1[i1] when idx2 >= 0 && vnMatch2[idx2] == i1; n_found counts those. */
#define AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE (-2)
struct amos_frame_view;                 /* include/amos_host_types.h */
typedef struct amos_sim3_search_pair {  /* per pair: 60 bytes */
    float R12[9], t12[3], s12;          /* read when d_sim3 == NULL */
    float th;                           /* 7.5 in LoopClosing.cc:454 */
    int32_t enabled;                    /* 0: the pair is skipped */
} amos_sim3_search_pair;
typedef struct amos_sim3_search_stats { /* per pair: 32 bytes */
    int32_t n_found;                    /* the reference's return value */
    int32_t n_in_view_12, n_in_view_21; /* source features that reached their window, per direction */
    int32_t n_single_12, n_single_21;   /* accepted features per direction, before the agreement */
    int32_t skipped;                    /* 1: enabled == 0 or no Sim3 in d_sim3 */
    int32_t code;                       /* 0; -4: a slot outside the frames */
    int32_t pad;
} amos_sim3_search_stats;
typedef struct amos_sim3_search {
    const amos_keypoint *d_kps;         /* [frames][capacity]: mvKeysUn */
    const uint8_t *d_desc;              /* [frames][capacity][32] */
    const int32_t *d_counts;            /* [frames] */
    const int32_t *d_cell_start;        /* [frames][64*48+1]       (amos_frame_grid_build_batch_device) */
    const int32_t *d_items;             /* [frames][capacity] */
    const amos_map_point *d_points;     /* [frames][capacity]: GetMapPointMatches() by feature; AMOS_MAP_POINT_SKIP: no point, or isBad();
                                           pos, min_distance, max_distance (raw) and desc are read, normal is not */
    const amos_sim3_camera *cameras;    /* host, n_frames entries: the record the solver takes */
    const float *scale_factors;         /* host, n_levels entries: one table and one set of bounds per call */
    const int32_t *d_pairs_1, *d_pairs_2; /* [n_pairs] frame slots */
    const amos_sim3_search_pair *pairs; /* host, n_pairs entries */
    const amos_sim3_result *d_sim3;     /* [n_pairs] or NULL: amos_match_sim3_batch_device's d_result, read in place */
    const int32_t *d_match12;           /* [pairs][capacity] */
    int32_t *d_match_out;               /* [pairs][capacity]; may be d_match12 */
    int32_t *d_match1;                  /* out, [pairs][capacity]: vnMatch1, -1 from N1 on */
    int32_t *d_match2;                  /* out, [pairs][capacity]: vnMatch2, -1 from N2 on */
    amos_sim3_search_stats *d_stats;    /* out, [pairs] */
    int32_t n_frames, n_pairs, capacity, n_levels;
    float min_x, max_x, min_y, max_y;   /* KeyFrame::mnMinX .. mnMaxY */
} amos_sim3_search;
/* Asynchronous on the matcher's stream; the host arrays are consumed before the call returns.  AMOS_ERR_INVALID, with a text and before the
 * device is touched, for a NULL handle or required pointer, n_pairs < 1, n_frames < 1, a capacity outside 1 .. 65536, n_levels outside
 * 1 .. AMOS_MAX_LEVELS, empty bounds, a camera or (d_sim3 == NULL, enabled pairs) a host-side Sim3 that is not finite or has s12 <= 0, a th
 * that is not finite or <= 0, d_match1 or d_match2 aliasing a row array or each other. */
int amos_match_sim3_search_batch_device(amos_match *m, const amos_sim3_search *s);
/* The host form for a C++ drop-in (amos-slam_amd/host/KeyFrameSim3Search.h): ONE pair, host arrays in and out, synchronous: one upload
 * (Frame::PosInGrid on the way), AssignFeaturesToGrid for both keyframes, the two launches, one download.  points1 [kf1->n], points2
 * [kf2->n]; cameras [2]: KF1's, KF2's; the bounds are the views' (they must agree); match12, match_out [kf1->n]; match1 [kf1->n] and
 * match2 [kf2->n] may be NULL.  A keyframe without features is valid.  A skipped pair leaves match_out, match1 and match2 untouched. */
int amos_match_sim3_search(amos_match *m, const struct amos_frame_view *kf1, const amos_map_point *points1, const struct amos_frame_view *kf2,
                           const amos_map_point *points2, const amos_sim3_camera *cameras, const amos_sim3_search_pair *sim3,
                           const float *scale_factors, int n_levels, const int32_t *match12, int32_t *match_out, int32_t *match1,
                           int32_t *match2, amos_sim3_search_stats *stats);

/* ---------------------------------------------------------------- loop-closing Sim3 optimisation */

/* Step 4 of LoopClosing::ComputeSim3's candidate loop (LoopClosing.cc:461): Optimizer::OptimizeSim3 (Optimizer.cc:1364-1590) for a batch of
 * PAIRS of resident keyframes -- the arrays of amos_sim3 -- reading SearchBySim3's rows and the solver's result records in place.  ONE
 * launch, k_sim3_optimize, one work-group of 256 threads per pair; the host reads one amos_sim3_opt_result per pair.  The arithmetic is
 * amos-slam_amd/csrc/amos_sim3_opt_core.h (its header lists the deviations): g2o's 7-dof vertex, the two projection edges per
 * correspondence with g2o's numeric central-difference Jacobian (delta 1e-9), a Huber kernel of width (float) sqrt(th2) on every edge in
 * both optimisations, Levenberg-Marquardt as amos_pose_core.h restates it.  PARITY WITH A COMPILED g2o UNPINNED (g2o needs Eigen, which this
 * project does not carry); what is pinned, bit for bit, is tests/sim3_optimization_restatement.py.
 *
 * Correspondences: keyframe-1 features i < N1 in ascending order whose row entry j lies in [0, N2), where d_points[slot 1][i] and
 * d_points[slot 2][j] do not carry AMOS_SIM3_POINT_SKIP.  -1, AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE and any other value are no correspondence.
 * An octave outside [0, n_levels) (either keypoint) skips the feature and sets bit 0 of status.  There is no cap below capacity.
 * The Sim3 of a pair: pairs[p] (host), or with d_sim3 != NULL row p of the solver's amos_sim3_result array, read on the device; pairs[p]
 * still supplies th2, fix_scale and enabled.  A pair with enabled == 0, or whose d_sim3 row has has_sim3 == 0 or code != 0, is SKIPPED: only
 * its result record is written (zeros, skipped = 1), its rows are neither read nor written.  A slot outside [0, n_frames): code = -4 in
 * the record (zeros otherwise), nothing else is written for that pair.
 *
 * optimize(5); a correspondence with e12.chi2 > th2 || e21.chi2 > th2 (double; NaN is an inlier; the errors of the last evaluated estimate)
 * is cleared: d_match_out[i] = -1, and it leaves the problem.  n_correspondences - n_bad_first < 10: n_inliers = 0, rounds = 1, the row
 * keeps the cleared entries and the record carries THE INPUT Sim3 (R12, t12, s12 as given; q, t, s and Scw made from them).  Otherwise
 * optimize(n_bad_first > 0 ? 10 : 5) from the estimate reached, with a fresh lambda; it clears more entries and n_inliers counts the rest.
 * The row: d_match12 in, d_match_out out, [pairs][capacity]; d_match_out == d_match12 is allowed (the chained use behind
 * amos_match_sim3_search_batch_device); otherwise all capacity entries are copied first. */
typedef struct amos_sim3_opt_pair {     /* per pair: 64 bytes */
    float R12[9], t12[3], s12;          /* read when d_sim3 == NULL: g2o::Sim3(R, t, s) */
    float th2;                          /* 10 in LoopClosing.cc:461 */
    int32_t fix_scale;                  /* mbFixScale: 0 or 1 */
    int32_t enabled;                    /* 0: the pair is skipped */
} amos_sim3_opt_pair;
typedef struct amos_sim3_opt_result {   /* per pair: 256 bytes */
    double q[4], t[3], s;               /* the vertex's estimate: rotation x, y, z, w (not normalised, as g2o keeps it), translation, scale */
    double lambda[2], chi2[2];          /* per optimisation: the last lambda, the robust chi2 */
    float R12[9], t12[3], s12;          /* toRotationMatrix(q), t, s rounded once to float (the input floats when n_inliers = 0 came early) */
    float Scw[16];                      /* gScm * Sim3(R2w, t2w, 1.0) as Converter::toCvMat stores it: [s R | t] over 0 0 0 1, row-major */
    int32_t n_correspondences, n_bad_first;
    int32_t n_inliers;                  /* the reference's return value */
    int32_t rounds;                     /* optimisations run: 0 (no correspondence), 1 or 2 */
    int32_t iterations[2], trials[2];   /* per optimisation */
    int32_t status;                     /* bit 0: an octave outside the table */
    int32_t skipped;                    /* 1: enabled == 0 or no Sim3 in d_sim3 */
    int32_t code;                       /* 0; -4: a slot outside the frames */
} amos_sim3_opt_result;
typedef struct amos_sim3_optimize {
    const amos_keypoint *d_kps;         /* [frames][capacity]: mvKeysUn (pt and octave are read) */
    const int32_t *d_counts;            /* [frames] */
    const amos_sim3_point *d_points;    /* [frames][capacity]: GetMapPointMatches() by feature */
    const amos_sim3_camera *cameras;    /* host, n_frames entries */
    const int32_t *d_pairs_1, *d_pairs_2; /* [n_pairs] frame slots */
    const float *inv_level_sigma2;      /* host, n_levels entries (mvInvLevelSigma2) */
    const amos_sim3_opt_pair *pairs;    /* host, n_pairs entries */
    const amos_sim3_result *d_sim3;     /* [n_pairs] or NULL: amos_match_sim3_batch_device's d_result, read in place */
    const int32_t *d_match12;           /* [pairs][capacity] */
    int32_t *d_match_out;               /* [pairs][capacity]; may be d_match12 */
    amos_sim3_opt_result *d_result;     /* out, [pairs] */
    int32_t n_frames, n_pairs, capacity, n_levels;
} amos_sim3_optimize;
/* Asynchronous on the matcher's stream; the host arrays are consumed before the call returns.  The compacted correspondences live in a
 * workspace the handle owns; no atomics, nothing to zero between calls.  AMOS_ERR_INVALID, with a text and before the device is touched, for a
 * NULL handle or required pointer, n_pairs < 1, n_frames < 1, a capacity outside 1 .. 65536, n_levels outside 1 .. AMOS_MAX_LEVELS, a camera
 * that is not finite, a fix_scale or enabled other than 0 or 1, and for an enabled pair a th2 that is not finite or <= 0 or (d_sim3 == NULL)
 * a Sim3 that is not finite or has s12 <= 0. */
int amos_match_sim3_optimize_batch_device(amos_match *m, const amos_sim3_optimize *s);
/* The host form for a C++ drop-in (amos-slam_amd/host/KeyFrameSim3Optimize.h): ONE pair, host arrays in and out, synchronous: one upload,
 * the launch, one download.  Keyframe 1: kps1 / points1 [n1]; keyframe 2: kps2 / points2 [n2]; cameras [2]; match12 in and match_out out
 * [n1] (they may be the same array).  A skipped pair leaves match_out untouched. */
int amos_match_sim3_optimize(amos_match *m, const amos_keypoint *kps1, const amos_sim3_point *points1, int n1, const amos_keypoint *kps2,
                             const amos_sim3_point *points2, int n2, const amos_sim3_camera *cameras, const int32_t *match12,
                             const float *inv_level_sigma2, int n_levels, const amos_sim3_opt_pair *pair, int32_t *match_out,
                             amos_sim3_opt_result *result);

/* ---------------------------------------------------------------- loop-closing point search ---- */

/* The last step of LoopClosing::ComputeSim3 (LoopClosing.cc:534-546): ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
 * (ORBmatcher.cc:388-512) and the count that accepts or rejects the loop, for a batch of QUERIES on resident keyframes.  Query q is (the
 * current keyframe's slot queries[q].frame, the points point_first[q] .. point_first[q] + point_count[q] - 1 of d_points, an Scw, row q of
 * d_matched).  With d_opt the Scw is read on the device from amos_match_sim3_optimize_batch_device's result records, so the chain BoW search
 * -> Sim3Solver -> SearchBySim3 -> OptimizeSim3 -> this search stays resident and the host reads one amos_loop_points_stats per candidate.
 *
 * Scw (:397-403; amos-slam_amd/csrc/amos_loop_points_core.h, compiled for host and device):
 *   scw = (float) sqrt(((double) S00^2 + (double) S01^2) + (double) S02^2)            the first row of sRcw
 *   inv = (float) (1.0 / (double) scw);  Rcw = sRcw * inv,  tcw = st * inv            one float32 product per element
 *   Ow  = (float) -(((double) R0c t0 + (double) R1c t1) + (double) R2c t2)            -Rcw^T tcw
 * spAlreadyFound (:407-408, :420), either or both of: d_found[point_first[q] + i] != 0; with queries[q].found_from_match, the points that the
 * entry row names through d_point_of_feature2: for every feature i < N of the keyframe whose row entry j lies in [0, capacity) and whose map
 * entry p = d_point_of_feature2[q][j] lies in [0, point_count[q]), point p of the query is found.
 * Pre-filter (:416-462): a point with AMOS_MAP_POINT_SKIP (isBad()) or found is no candidate; the others pass the AMOS_FUSE_SIM3 pre-filter of
 * "fuse search" below, unchanged: p3Dc.z < 0.0f is out, invz = 1.0f / z, u = fx * (X * invz) + cx, the half-open KeyFrame::IsInImage, the
 * 0.8f / 1.2f distance band, the viewing angle in double, the level in its table form.  A u or v that is not finite is out of view and sets
 * bit 0 of the query's status.
 * Search (:464-507): radius th * scale_factors[level]; KeyFrame::GetFeaturesInArea without a level check, |kp.x - u| < r && |kp.y - v| < r;
 * levels level - 1 .. level; FEATURES THAT ARE OCCUPIED AT THAT MOMENT ARE PASSED OVER (:482); the nearest descriptor by strict < in the
 * order x-major cells, then y, then insertion; accepted when bestDist <= max_dist, and the accept occupies the feature.  The points are
 * decided in list order; there is no ratio test and no rotation histogram.  On entry feature i is occupied when d_matched[q][i] != -1: every
 * other value is a non-NULL pointer, AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE included, so the row amos_match_sim3_optimize_batch_device leaves in
 * d_match_out is read in place.  d_matched is never written.
 * Launches: k_loop_found (only when a query has found_from_match), k_loop_project (one thread per point), k_loop_window_best2 (eight lanes per
 * point in view: the best two of the features free ON ENTRY), k_loop_accept (one wave per query: the sequential loop over those records
 * against a bitmap of the occupied features; a point whose two recorded features both lay within max_dist and are both taken by then has
 * its window searched again by the whole wave, and n_researched counts these; a second beyond max_dist settles the point without a search,
 * since it is the nearest of everything but the best).
 * A query is SKIPPED when enabled == 0, or with d_opt when row q has skipped != 0, code != 0 or n_inliers < min_inliers (the test of
 * LoopClosing.cc:464): only its stats record is written (zeros, skipped = 1); its rows are neither read nor written. */
typedef struct amos_loop_points_query {  /* per query: 108 bytes */
    float Scw[16];                      /* read when d_opt == NULL: row-major, as Converter::toCvMat stores it */
    float fx, fy, cx, cy;               /* pKF->fx .. cy */
    float th;                           /* 10 in LoopClosing.cc:534 */
    int32_t frame;                      /* the current keyframe's slot, in [0, n_frames) */
    int32_t max_dist;                   /* TH_LOW = 50 */
    int32_t min_inliers;                /* 20 (LoopClosing.cc:464); read with d_opt */
    int32_t min_total;                  /* 40 (LoopClosing.cc:546) */
    int32_t enabled;                    /* 0: the query is skipped */
    int32_t found_from_match;           /* 0 or 1: mark the points of the entry row's features through d_point_of_feature2 */
} amos_loop_points_query;
typedef struct amos_loop_points_stats { /* per query: 32 bytes */
    int32_t n_candidates;               /* points neither bad nor found */
    int32_t n_in_view;                  /* candidates that passed the pre-filter */
    int32_t n_matches;                  /* the reference's return value */
    int32_t n_researched;               /* points whose window was searched again against the bitmap */
    int32_t n_total;                    /* features i < N occupied on entry + n_matches: nTotalMatches of LoopClosing.cc:538-543 */
    int32_t accepted;                   /* n_total >= min_total */
    int32_t status;                     /* bit 0: a projection was not finite */
    int32_t skipped;                    /* 1: nothing but this record was written */
} amos_loop_points_stats;
typedef struct amos_loop_points_search {
    const amos_keypoint *d_kps;         /* [frames][capacity]: mvKeysUn */
    const uint8_t *d_desc;              /* [frames][capacity][32] */
    const int32_t *d_counts;            /* [frames] */
    const int32_t *d_cell_start;        /* [frames][64*48+1]       (amos_frame_grid_build_batch_device) */
    const int32_t *d_items;             /* [frames][capacity] */
    const float *scale_factors;         /* host, n_levels entries */
    const amos_map_point *d_points;     /* n_points: mvpLoopMapPoints; bit 0 of flags: isBad() */
    const int32_t *point_first, *point_count; /* host, n_queries: ranges of different queries may coincide */
    const amos_loop_points_query *queries; /* host, n_queries */
    const amos_sim3_opt_result *d_opt;  /* [n_queries] or NULL: amos_match_sim3_optimize_batch_device's d_result, read in place */
    const int32_t *d_matched;           /* [queries][capacity]: vpMatched on entry, -1 = free */
    const uint8_t *d_found;             /* n_points or NULL */
    const int32_t *d_point_of_feature2; /* [queries][capacity] or NULL (required by found_from_match): keyframe-2 feature -> index in the query's list, or -1 */
    int32_t *d_loop_match;              /* out, [queries][capacity]: per feature the index in the query's list of the point this call matched to it, or -1 */
    amos_loop_points_stats *d_stats;    /* out, [n_queries] */
    int32_t n_frames, n_queries, n_points, capacity, n_levels;
    float min_x, max_x, min_y, max_y;   /* KeyFrame::mnMinX .. mnMaxY */
} amos_loop_points_search;
/* Asynchronous on the matcher's stream; every host array is consumed before the call returns.  The per-point records live in a workspace the
 * handle owns; nothing has to be zeroed between calls and a smaller call on a reused handle is valid.  All capacity entries of an executed
 * query's d_loop_match row are written.  AMOS_ERR_INVALID, with a text and before the device is touched, for a NULL handle or required
 * pointer, n_queries < 1, n_frames < 1, n_points < 0, a frame outside n_frames, a point range outside n_points, a capacity outside
 * 1 .. 65536, n_levels outside 1 .. AMOS_MAX_LEVELS, empty image bounds, a th or intrinsics that are not finite (th <= 0 included), with
 * d_opt == NULL an Scw that is not finite or whose first row has norm 0, a max_dist outside 0 .. 255, an enabled or found_from_match other
 * than 0 or 1, and found_from_match without d_point_of_feature2. */
int amos_match_loop_points_batch_device(amos_match *m, const amos_loop_points_search *s);
/* The host form for a C++ drop-in (amos-slam_amd/host/KeyFrameLoopPoints.h): ONE query, host arrays in and out, synchronous: one upload,
 * AssignFeaturesToGrid, the launches, one download.  matched [kf->n] (or NULL: every feature free); found [n_points] or NULL;
 * point_of_feature2 [n2] or NULL; loop_match [kf->n] out.  A keyframe without features and a list without points are valid.  A skipped
 * query leaves loop_match untouched. */
int amos_match_loop_points(amos_match *m, const struct amos_frame_view *kf, const amos_map_point *points, int n_points,
                           const amos_loop_points_query *query, const int32_t *matched, const uint8_t *found, const int32_t *point_of_feature2,
                           int n2, const float *scale_factors, int n_levels, int32_t *loop_match, amos_loop_points_stats *stats);

/* ---------------------------------------------------------------- fuse search ---------------- */

/* ORBmatcher::Fuse for a batch of PAIRS of resident keyframes: pair p is (keyframe pair_frame[p], the points point_first[p] ..
 * point_first[p] + point_count[p] - 1 of d_points, the camera cameras[p]).  For every (pair, point) the pre-filter of ORBmatcher.cc:1042-1083
 * and the search of :1085-1148, in ONE launch; nothing of the write-back (:1150-1170: Replace / AddObservation) is done here.
 *
 * Pre-filter (PARITY UNPINNED like the local map search above, whose arithmetic this is): float32, every operation rounded, nothing fused, except
 *   p3Dc = Rcw * P + tcw      one gemm per row: ((R0 P0 + R1 P1) + R2 P2) + t in double, one rounding to float; p3Dc.z < 0.0f is out
 *   invz = 1.0f / z           the reference writes `1/p3Dc.at<float>(2)`: a float division.  (float) (1.0 / (double) z) is the same value for
 *                             every z: a quotient of two floats rounded to 53 bits and then to 24 is the correctly rounded float quotient
 *   x = X * invz;  u = fx * x + cx;  v alike
 *   KeyFrame::IsInImage: u >= min_x && u < max_x && v >= min_y && v < max_y; a projection that is not finite fails it (z == 0 included)
 *   ur = u - mbf * invz       (AMOS_FUSE_LOCAL; 0 in AMOS_FUSE_SIM3)
 *   PO = P - Ow;  dist3D = (float) sqrt(((double) PO0^2 + (double) PO1^2) + (double) PO2^2)
 *   dist3D < 0.8f * min_distance || dist3D > 1.2f * max_distance is out
 *   (((double) PO0 Pn0 + (double) PO1 Pn1) + (double) PO2 Pn2) < 0.5 * (double) dist3D is out: a comparison in double, no division
 *   level = number of m in [0, n_levels) with max_distance / dist3D > scale_factors[m], at most n_levels - 1 (the table form of
 *   MapPoint::PredictScale of the local map search: it differs from the logf form only for a ratio within rounding of a table entry)
 * Search: radius th * scale_factors[level]; KeyFrame::GetFeaturesInArea (KeyFrame.cc:752-797: Frame's cell arithmetic, no level check) with
 * |kp.x - u| < r && |kp.y - v| < r; levels level - 1 .. level; in AMOS_FUSE_LOCAL the chi-square gate in float32, unfused: a feature with
 * u_right >= 0 is rejected when (double) (((ex ex + ey ey) + er er) * inv_level_sigma2[kpLevel]) > 7.8, any other when
 * (double) ((ex ex + ey ey) * inv_level_sigma2[kpLevel]) > 5.99 (ex = u - kp.x, ey = v - kp.y, er = ur - u_right); the nearest descriptor by
 * strict < in the order x-major cells, then y, then insertion; accepted when bestDist <= max_dist (TH_LOW for both reference callers).
 * AMOS_FUSE_SIM3 is Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1179-1312): no chi-square gate; the caller passes the unscaled Rcw, tcw
 * and Ow = -R^T t. */
#define AMOS_FUSE_LOCAL 0
#define AMOS_FUSE_SIM3 1
typedef struct amos_fuse_camera {      /* per pair: 84 bytes */
    float Rcw[9], tcw[3], Ow[3];       /* KeyFrame::GetRotation (row-major), GetTranslation, GetCameraCenter */
    float fx, fy, cx, cy, mbf;
    float th;
} amos_fuse_camera;
typedef struct amos_fuse_stats {       /* per pair: 8 bytes */
    int32_t n_in_view;                 /* points that passed the pre-filter */
    int32_t n_accepted;                /* points with an accepted feature */
} amos_fuse_stats;
struct amos_window_query;              /* include/amos_host_types.h */
struct amos_frame_view;
typedef struct amos_fuse_search {
    const amos_keypoint *d_kps;        /* [frames][capacity]: mvKeysUn */
    const uint8_t *d_desc;             /* [frames][capacity][32] */
    const int32_t *d_counts;           /* [frames] */
    const int32_t *d_cell_start;       /* [frames][64*48+1]       (amos_frame_grid_build_batch_device) */
    const int32_t *d_items;            /* [frames][capacity] */
    const float *d_u_right;            /* [frames][capacity] or NULL (monocular: every feature takes the 5.99 branch) */
    const float *scale_factors;        /* host, n_levels entries */
    const float *inv_level_sigma2;     /* host, n_levels entries; read in AMOS_FUSE_LOCAL */
    const amos_map_point *d_points;    /* n_points; bit 0 of flags: skip (NULL or isBad()) */
    const int32_t *pair_frame;         /* host, n_pairs: in [0, n_frames) */
    const int32_t *point_first, *point_count; /* host, n_pairs: ranges of different pairs may coincide (one list against many keyframes) */
    const int32_t *out_off;            /* host, n_pairs, ascending, out_off[p + 1] >= out_off[p] + point_count[p]: point i of pair p -> out_off[p] + i */
    const amos_fuse_camera *cameras;   /* host, n_pairs */
    const uint8_t *d_skip;             /* indexed like the outputs: 1 = skipped for this keyframe (IsInKeyFrame, spAlreadyFound); or NULL */
    struct amos_window_query *d_query; /* out: u, v, ur, level (0 where the point is not in view), src = i, the point's descriptor */
    uint8_t *d_in_view;                /* out: 1 where the point passed the pre-filter */
    int32_t *d_best_idx;               /* out: the accepted feature, or -1 */
    int32_t *d_best_dist;              /* out: the nearest candidate's distance, accepted or not; 256 where the window had none */
    amos_fuse_stats *d_stats;          /* out, [n_pairs] */
    int32_t n_frames, n_pairs, n_points, capacity, n_levels;
    int32_t mode, max_dist;
    float min_x, max_x, min_y, max_y;  /* KeyFrame::mnMinX .. mnMaxY */
} amos_fuse_search;
/* Asynchronous on the matcher's stream; every host array is consumed before the call returns.  capacity <= 65536.  AMOS_ERR_INVALID, with a
 * text, for a NULL argument (inv_level_sigma2 in AMOS_FUSE_LOCAL), a pair_frame outside n_frames, a point range outside n_points, an out_off
 * out of order, a capacity, n_levels or mode out of range or empty image bounds. */
int amos_match_fuse_batch_device(amos_match *m, const amos_fuse_search *s);
/* The host form for a C++ drop-in (amos-slam_amd/host/KeyFrameFuse.h): n_kfs keyframe views with the same image bounds, n_points points and
 * n_pairs pairs from host arrays, synchronous: ONE upload (every keyframe and the point list staged once, Frame::PosInGrid on the way),
 * AssignFeaturesToGrid for all keyframes, the launch, ONE download.  skip (or NULL), query, in_view, best_idx and best_dist hold n_out
 * entries, indexed out_off[p] + i; entries no pair owns are left alone.  A keyframe without features and a pair without points are valid
 * (no feature is accepted); n_pairs == 0 returns at once. */
int amos_match_fuse(amos_match *m, const struct amos_frame_view *kfs, int n_kfs, const amos_map_point *points, int n_points, int n_pairs,
                    const int32_t *pair_frame, const int32_t *point_first, const int32_t *point_count, const int32_t *out_off,
                    const amos_fuse_camera *cameras, const uint8_t *skip, int n_out, const float *scale_factors, const float *inv_level_sigma2,
                    int n_levels, int mode, int max_dist, struct amos_window_query *query, uint8_t *in_view, int32_t *best_idx, int32_t *best_dist,
                    amos_fuse_stats *stats);

/* ---------------------------------------------------------------- mask pre-processing (8f-4) - */

/* The pre-processing chain of the mask pass on the device, from the raw BGR frame to the network input:
 * yolact::evalImage's marshalling (yolact.cc:220, 385-451: cv::resize to W480 x H640, u8 / 255.0),
 * eval_image's "* 255" and cv2.resize back to 640 x 480 (yolact_interface.py:862-866) and FastBaseTransform
 * (utils/augmentations.py:616-657: bilinear to 550 x 550, (x - MEANS) / STD, BGR -> RGB).
 * d_bgr: [n_frames][height][width][3] uint8; d_out: [n_frames][3][550][550] float32.  Asynchronous on the
 * handle's stream (pass PyTorch's current stream so that the network simply follows). */
int amos_mask_pre_create(int device, void *stream, int width, int height, int max_batch, amos_mask_pre **out);
void amos_mask_pre_destroy(amos_mask_pre *p);
void *amos_mask_pre_stream(amos_mask_pre *p); /* the hipStream_t the handle issues on */
int amos_mask_preprocess_batch_device(amos_mask_pre *p, const uint8_t *d_bgr, int n_frames, float *d_out);
/* How the chain runs (this call and amos_orb_detect_color_with_mask_pre_batch_device).  1 (default): one kernel from the u8 frame to the
 * tensor, the two intermediate images staying in on-chip memory, for every frame size whose source windows fit there (640 x 480,
 * 1280 x 720; not 1920 x 1080 -- such sizes take the three kernels whatever the mode).  0: three kernels through two float intermediates
 * (2 x 3.7 MB per frame of max_batch, allocated on the first such call).  The tensor has the same bits either way.  Other values only
 * query.  Returns the previous mode; the initial value is AMOS_MASK_PRE_FUSED=0 / 1 in the environment, read once per process. */
int amos_mask_pre_mode(int mode);
/* 1 when calls on this handle take the one-pass kernel under the current mode, 0 when they take the three kernels;
 * source_window_bytes (may be NULL): what the frame size needs of the kernel's 16 KB source window. */
int amos_mask_pre_one_pass(const amos_mask_pre *p, int *source_window_bytes);

/* SURVEY 8f-4, "one pass over the RGB-D frame": the colour frame is read ONCE for both of its consumers -- the gray
 * conversion into the padded level 0 (Tracking.cc:308-321, then the rest of amos_orb_detect_batch_device) and stage A of
 * the mask pre-processing (yolact.cc:220, 385-451) -- and the network input appears in d_net_input ([n][3][550][550]
 * float32) on the extractor's stream.  Same results as amos_orb_extract_batch_device_color's detect part and
 * amos_mask_preprocess_batch_device; follow with amos_orb_gate_batch_device / amos_orb_describe_batch_device. */
int amos_orb_detect_color_with_mask_pre_batch_device(amos_orb *h, amos_mask_pre *pre, const uint8_t *d_color,
                                                     size_t frame_stride, size_t row_stride, int width, int height,
                                                     int n_frames, int channels, int rgb_order, float *d_net_input);

/* Fused epilogue of one convolution of the mask network, in place on a channels-last (NHWC) float32 tensor of n
 * elements: y = act((y + bias[c]) + residual), act = ReLU when relu != 0, residual may be NULL.  Replaces PyTorch's
 * separate bias-add, residual-add and clamp passes (same summation order: identical bits).  Asynchronous on `stream`
 * (a hipStream_t; pass PyTorch's current stream). */
int amos_mask_bias_act_device(void *stream, float *d_y, const float *d_bias, const float *d_residual, size_t n,
                              int channels, int relu);

/* The stem's tail (backbone.py ResNetBackbone.forward: bn1 folded -> relu -> maxpool): y = max_pool2d(relu(x + bias[c]), 3, stride 2,
 * padding 1) of a channels-last float32 tensor x [n][in_h][in_w][channels] (a convolution's raw output) in ONE pass; y is
 * [n][(in_h - 1) / 2 + 1][(in_w - 1) / 2 + 1][channels].  Bit-identical to the separate passes (max and the monotone bias + ReLU commute). */
int amos_mask_bias_relu_maxpool_device(void *stream, const float *d_x, const float *d_bias, float *d_y, int n, int in_h, int in_w,
                                       int channels);

/* The whole stem of the backbone (backbone.py:77-80,129-132: conv1 = Conv2d(3, 64, 7, stride 2, padding 3) with bn1 folded into weight and
 * bias, ReLU, MaxPool2d(3, stride 2, padding 1)) as ONE kernel on the fp32 MFMA units: the 7 x 7 convolution's output stays in registers /
 * LDS and only the pooled tensor is written.  x is float32 [batch][3][height][width] addressed through ELEMENT strides (frame, channel, row,
 * column: planar and channels-last inputs alike); y is channels-last [batch][ph][pw][64] with ch = (height - 1) / 2 + 1, ph = (ch - 1) / 2 + 1
 * (likewise for the width).  d_packed: the weights as amos_mask_stem_weights_device lays them out (amos_mask_stem_weight_floats() floats)
 * from a [64][3][7][7] tensor addressed through its element strides (out channel, in channel, row, column).  Sums in float32 in the
 * MFMA's order (the library's convolution sums in another order: results agree to float32 rounding of a 147-term sum, not bit for bit);
 * bias + ReLU after the maximum, which is bit-identical to before it.  Replaces F.conv2d + amos_mask_bias_relu_maxpool_device. */
int amos_mask_stem_weight_floats(void);
int amos_mask_stem_weights_device(void *stream, const float *d_w, long long stride_n, long long stride_c, long long stride_y, long long stride_x,
                                  float *d_packed);
int amos_mask_stem_device(void *stream, const float *d_x, long long stride_b, long long stride_c, long long stride_y, long long stride_x,
                          const float *d_packed, const float *d_bias, float *d_y, int batch, int height, int width);

/* A convolution of the mask network (yolact.py / backbone.py as amos-slam_amd/mask/net.py restates them: the ResNet-50
 * bottlenecks, the FPN, the prototype network, the prediction heads) on channels-last float32 tensors as one fp32 MFMA
 * (implicit) GEMM with the epilogue of amos_mask_bias_act_device fused:
 *   y[b][oy][ox][n] = act( sum_{dy,dx,k} x[b][oy*stride - pad + dy][ox*stride - pad + dx][k] * w[n][dy][dx][k]
 *                          + bias[n]  (+ residual[b][oy][ox][n]) )        (zeros outside the image, dilation 1, groups 1)
 * x: [batch][in_h][in_w][cin]; w: [cout][kh][kw][cin], i.e. a Conv2d weight in channels-last memory format (for 1 x 1 either
 * format); y and residual: [batch][oh][ow][cout] with oh = (in_h + 2 pad - kh) / stride + 1; bias and residual may be NULL.
 * Requires cin % 32 == 0, cout % 64 == 0, kernel <= 7 x 7, pad < kernel, stride 1..4, 16-byte aligned pointers
 * (amos_mask_conv_supported returns AMOS_OK for such a shape, AMOS_ERR_INVALID otherwise: the caller then keeps its library
 * convolution).  The sum is taken in another order than MIOpen's: results agree to float32 rounding, not bit for bit.
 * Asynchronous on `stream`.  amos_mask_conv1x1_* are the kh = kw = 1, pad = 0 case. */
int amos_mask_conv_supported(int cin, int cout, int kh, int kw, int stride, int pad);
int amos_mask_conv_device(void *stream, const float *d_x, const float *d_w, const float *d_bias, const float *d_residual,
                          float *d_y, int batch, int in_h, int in_w, int cin, int cout, int kh, int kw, int stride, int pad,
                          int relu);
/* The same convolution with split-K for SMALL launches (one frame per pass: a 1 x 1 layer at 35 x 35 or 18 x 18 is 3 - 40 work-groups of up
 * to 64 k-stages on 256 CUs): the k loop is cut into splits, one work-group per (tile, split); every split leaves its tile in the workspace
 * and the last work-group to arrive at a tile adds the splits in split order (the same bits whichever group that is) and applies bias,
 * residual and ReLU -- one launch, no zero fill, no reduction pass.  amos_mask_conv_workspace_bytes: scratch this shape wants (0: the plan
 * for it is an ordinary launch; d_workspace may then be NULL).  The first 16 KB of the workspace are tile counters: ZERO before the first
 * use, left zero by every launch; launches that share a workspace must be ordered on one stream. */
size_t amos_mask_conv_workspace_bytes(int batch, int in_h, int in_w, int cin, int cout, int kh, int kw, int stride, int pad);
int amos_mask_conv_ws_device(void *stream, const float *d_x, const float *d_w, const float *d_bias, const float *d_residual, float *d_y,
                             int batch, int in_h, int in_w, int cin, int cout, int kh, int kw, int stride, int pad, int relu,
                             void *d_workspace, size_t workspace_bytes);
/* Work-group tile of amos_mask_conv_device: -1 = automatic (128 x 128 outputs unless that leaves fewer than 1 024 work-groups or
 * cout % 128 != 0, then 128 x 64), 0 = 128 x 128 wherever cout allows, 1 = always 128 x 64.  Returns the mode in force before
 * the call; any other argument only queries.  The environment's AMOS_GEMM_NARROW (0 / 1) is the initial mode, read once.
 * amos_mask_conv_kernel_name writes the name of the kernel the call with these arguments launches (as a profiler shows it). */
int amos_mask_conv_tile_mode(int mode);
int amos_mask_conv_kernel_name(int batch, int in_h, int in_w, int cin, int cout, int kh, int kw, int stride, int pad, char *name,
                               int name_len);
/* The first block of a ResNet stage, its projection shortcut fused into its expanding 1 x 1 convolution (one launch):
 *   d = (conv1x1(x, wd, stride) + bd) + 0      x [batch][in_h][in_w][cin], wd [cout][cin]
 *   y = relu((conv1x1(yc, w3) + b3) + d)        yc [batch][oh][ow][planes], w3 [cout][planes], y [batch][oh][ow][cout]
 * with oh = (in_h - 1) / stride + 1 (ow alike).  d stays on chip.  Every value of y is the float the two amos_mask_conv_device calls
 * (d stored, then read back as the residual) produce.  amos_mask_conv_chain_supported: AMOS_OK where amos_mask_conv_device would run
 * both as 128 x 128 tiles without split-K (amos_mask_conv_tile_mode taken into account), AMOS_ERR_INVALID otherwise, and then
 * amos_mask_conv_chain_device refuses the call too.  Asynchronous on `stream`; 16-byte aligned channels-last float32 tensors. */
int amos_mask_conv_chain_supported(int batch, int in_h, int in_w, int cin, int planes, int cout, int stride);
int amos_mask_conv_chain_device(void *stream, const float *d_x, const float *d_wd, const float *d_bd, const float *d_yc, const float *d_w3,
                                const float *d_b3, float *d_y, int batch, int in_h, int in_w, int cin, int planes, int cout, int stride);
int amos_mask_conv1x1_supported(int cin, int cout, int stride);
/* The feature pyramid's lateral 1 x 1 convolution with the top-down resize of the level above in its epilogue (one launch):
 *   y = act((conv1x1(x, w) + bias) + bilinear(up))    x [batch][in_h][in_w][cin], up [batch][up_h][up_w][cout], y [batch][in_h][in_w][cout]
 * bilinear = amos_mask_bilinear_nhwc_device(up -> in_h x in_w, scale_h, scale_w): the same taps, weights and order of roundings, so every
 * value of y is the float that call followed by amos_mask_conv_device (d_residual = its output) stores; the resized tensor is never
 * written.  Tiles as amos_mask_conv_device picks them (amos_mask_conv_tile_mode), no split-K.  d_bias may be NULL.
 * amos_mask_fpn_fold_mode: 1 = the network's pyramid uses this entry where its lateral runs on the GEMM (default), 0 = resize and
 * convolution as two launches; returns the mode in force before the call, any other argument only queries.  AMOS_MASK_FPN_FOLD=0 / 1 in
 * the environment is the initial value. */
int amos_mask_conv_upsampled_residual_device(void *stream, const float *d_x, const float *d_w, const float *d_bias, const float *d_up,
                                             float *d_y, int batch, int in_h, int in_w, int cin, int cout, int up_h, int up_w,
                                             float scale_h, float scale_w, int relu);
int amos_mask_fpn_fold_mode(int mode);

/* The same convolution for 3 x 3 kernels with stride 1 and pad 1 (the prototype network, the prediction head, the FPN's prediction layers
 * and the bottlenecks' conv2 of yolact.py / backbone.py: 70 % of the network's multiply-accumulates) as Winograd F(2 x 2, 3 x 3) on the
 * fp32 MFMA units: 2.25 x fewer multiplies, float32 in and float32 accumulate; the result differs from the direct form by float32
 * rounding of the transforms (tests/test_mask.py holds both to the same bound against a float64 convolution).
 *   amos_mask_winograd_supported(cin, cout): AMOS_OK when cin % 16 == 0, cin >= 32 and cout % 64 == 0.
 *   amos_mask_winograd_weight_floats(cin, cout): size of the transformed weight in floats (16 * cin * cout; 0 if unsupported).
 *   amos_mask_winograd_weights_device: d_w [cout][3][3][cin] (a channels-last Conv2d weight) -> d_u = G g G^T of every filter, laid
 *     out in the order the kernel's MFMA fragments are read; once per layer.
 *   amos_mask_winograd_conv_device: y = act(conv3x3(x, w) + bias (+ residual)); x [batch][h][w][cin] (below 2 GiB), y and residual
 *     [batch][h][w][cout], all 16-byte aligned; bias and residual may be NULL.  Asynchronous on `stream`. */
int amos_mask_winograd_supported(int cin, int cout);
size_t amos_mask_winograd_weight_floats(int cin, int cout);
int amos_mask_winograd_weights_device(void *stream, const float *d_w, float *d_u, int cin, int cout);
int amos_mask_winograd_conv_device(void *stream, const float *d_x, const float *d_u, const float *d_bias, const float *d_residual,
                                   float *d_y, int batch, int h, int w, int cin, int cout, int relu);
/* The same layers as Winograd F(2 x 4, 3 x 3): F(2, 3) vertically, F(4, 3) horizontally -- 24 multiplies per 2 x 4 outputs and channel
 * pair (3.0 per output against 4.0 for F(2 x 2) and 9.0 direct); same arguments, same support rule (amos_mask_winograd_supported),
 * same epilogue; the transformed weight G2 g G4^T has 24 * cin * cout floats and its own layout (make it with the matching function).
 * Rounding: the F(4, 3) transforms carry the factors 4, 5, 8 and 1 / 24, so its error against a float64 convolution is a few times
 * that of F(2 x 2) -- tests/test_mask.py holds both to the direct kernels' bound (1e-5 of the sum of |terms|). */
size_t amos_mask_winograd24_weight_floats(int cin, int cout);
int amos_mask_winograd24_weights_device(void *stream, const float *d_w, float *d_u, int cin, int cout);
int amos_mask_winograd24_conv_device(void *stream, const float *d_x, const float *d_u, const float *d_bias, const float *d_residual,
                                     float *d_y, int batch, int h, int w, int cin, int cout, int relu);
/* The same convolution with the channel-blocked activation layout on either side: in_blocked != 0 reads d_x as [batch][cin / 8][h][w][8]
 * floats, out_blocked != 0 writes d_y (and reads d_residual) as [batch][cout / 8][h][w][8]; 0 = channels-last [batch][h][w][c] (what
 * amos_mask_winograd24_conv_device takes).  A stage of the kernel reads 8 input channels of every pixel of its patch: blocked, those are
 * contiguous whole cache lines used once; channels-last, a quarter of every line four times.  Same arithmetic, same bits. */
int amos_mask_winograd24_conv_layout_device(void *stream, const float *d_x, const float *d_u, const float *d_bias, const float *d_residual,
                                            float *d_y, int batch, int h, int w, int cin, int cout, int relu, int in_blocked, int out_blocked);
/* Which launch form the F(2 x 4) kernel takes: -1 automatic and 0: one work-group per (tile block, channel tile) id (the default form);
 * 1: the PERSISTENT form -- one work-group per CU walking the ids, the next id's first requests travelling under the current id's last
 * stages and epilogue.  Measured 3.5 - 5 % slower on the network's large layers (tools/r5_w24_persist.py), hence not the automatic choice;
 * kept selectable and under test.  Returns the previous mode (-2 or anything else out of range: query only).  Same bits either way;
 * AMOS_W24_PERSIST=0 / 1 in the environment is the initial value. */
int amos_mask_winograd24_persistent_mode(int mode);
/* Output channels per work-group of the F(2 x 4) kernel: -1 by launch size (the default: 32 per group -- twice the groups -- while 64-channel
 * groups would leave most CUs without one, i.e. one-frame launches), 0 always 64, 1 always 32.  Returns the previous mode (out of range:
 * query only).  Same bits either way; AMOS_W24_NARROW=0 / 1 in the environment is the initial value. */
int amos_mask_winograd24_narrow_mode(int mode);
int amos_mask_conv1x1_device(void *stream, const float *d_x, const float *d_w, const float *d_bias, const float *d_residual,
                             float *d_y, int batch, int in_h, int in_w, int cin, int cout, int stride, int relu);

/* F.interpolate(x, mode="bilinear", align_corners=False) of a channels-last float32 tensor [n][in_h][in_w][channels] ->
 * [n][out_h][out_w][channels] (the FPN's top-down path and the prototype network's x2 step).  scale_h / scale_w as
 * PyTorch derives them: 1 / scale_factor when a scale factor was given, else in / out (float32).  channels % 4 == 0. */
int amos_mask_bilinear_nhwc_device(void *stream, const float *d_x, float *d_y, int n, int in_h, int in_w, int out_h,
                                   int out_w, int channels, float scale_h, float scale_w);

/* The same with a ReLU on the result when relu != 0 (the prototype network's upsample, yolact.py proto_net[6..7]). */
int amos_mask_bilinear_nhwc_act_device(void *stream, const float *d_x, float *d_y, int n, int in_h, int in_w, int out_h,
                                       int out_w, int channels, float scale_h, float scale_w, int relu);

/* An exact x 2 enlargement (out = 2 x in, scale 0.5: the prototype network's upsampling step) runs a form of the kernel that makes 2 x 2 outputs
 * per thread from the 3 x 3 source pixels they touch (the same bits, fewer reads).  mode 1: where it applies (default), 0: never (A/B runs,
 * tests); any other value only reports.  Returns the mode in force before the call. */
int amos_mask_bilinear_x2_mode(int mode);

/* The suppression term of Fast NMS (layers/functions/detection.py:103-170 fast_nms, layers/box_utils.py jaccard): d_boxes holds
 * n_lists lists of k boxes [x1, y1, x2, y2] sorted by descending score; d_out[list][j] = max over i < j of IoU(box i, box j), 0 for
 * j == 0 -- what `jaccard(boxes, boxes).triu_(diagonal=1).max(dim=1)` yields, in jaccard's float32 arithmetic (bit-identical to
 * PyTorch's elementwise kernels), without materialising the k x k matrices.  1 <= k <= 256. */
int amos_mask_nms_column_max_device(void *stream, const float *d_boxes, float *d_out, int n_lists, int k);

/* Class scores for Fast NMS in the static-shape batch form (layers/functions/detection.py:46-75 as mask/detect.py detect_batch
 * restates it): d_conf [batch][n_priors][n_classes_with_background] (the network's softmax output) -> d_scores
 * [batch][n_classes_with_background - 1][n_priors]: the background column dropped, the class axis first (the layout top-k
 * reads), and -1 for every prior whose best non-background score is not > threshold.  Pure selection: exact. */
int amos_mask_class_scores_device(void *stream, const float *d_conf, float *d_scores, int batch, int n_priors,
                                  int n_classes_with_background, float threshold);

/* The tail of yolact_interface.py postprocess + prep_display (:678-779, :806-832): d_masks [batch][n_det][mask_h][mask_w] are the
 * cropped sigmoid masks, d_flags [batch][n_det] != 0 marks the detections that count (displayed persons); d_out [batch][out_h][out_w]
 * = (number of flagged detections whose mask, upsampled bilinearly (align_corners = False) to the frame, is > 0.5) * 255 modulo 256,
 * the reference's `(m * 255).byte()`.  Same source index and weights as PyTorch's upsample_bilinear2d. */
int amos_mask_person_mask_device(void *stream, const float *d_masks, const uint8_t *d_flags, uint8_t *d_out, int batch, int n_det,
                                 int mask_h, int mask_w, int out_h, int out_w);
/* The same with the masks' crop rectangles: d_rects [batch][n_det][4] = (x0, x1, y0, y1) in mask pixels (16-byte aligned), and mask
 * (b, i) must be ZERO at every pixel outside x0 <= x < x1, y0 <= y < y1 (what postprocess's crop leaves).  A work-group then stages and
 * evaluates only the flagged detections whose rectangle reaches its source window; the others add nothing anywhere under it.  Same bytes
 * as amos_mask_person_mask_device; d_rects NULL is that call.
 * amos_mask_person_window_mode: 1 = staging rows derived from the scale and the rectangles used (default), 0 = six staging rows and the
 * rectangles ignored (the earlier form); returns the mode in force before the call, any other argument only queries.
 * AMOS_MASK_PERSON_WINDOW=0 / 1 in the environment is the initial value. */
int amos_mask_person_mask_rects_device(void *stream, const float *d_masks, const uint8_t *d_flags, const float *d_rects, uint8_t *d_out,
                                       int batch, int n_det, int mask_h, int mask_w, int out_h, int out_w);
int amos_mask_person_window_mode(int mode);

/* The prediction head's outputs for one pyramid level (yolact.py PredictionModule.forward and the cat / softmax of Yolact.forward):
 * d_raw [batch][cells][channels_padded] = the merged output convolution WITHOUT bias, channels [anchors x 4 | anchors x
 * n_classes_with_background | anchors x mask_dim | padding]; the level's priors (cell-major, anchor-minor) start at prior_offset of
 * d_loc [batch][n_priors_total][4] = raw + bias, d_conf [..][n_classes_with_background] = softmax(raw + bias), d_coef [..][mask_dim]
 * = tanh(raw + bias).  loc and coef equal PyTorch's bit for bit, conf to float32 rounding (order of the softmax sum). */
int amos_mask_head_outputs_device(void *stream, const float *d_raw, const float *d_bias, float *d_loc, float *d_conf, float *d_coef,
                                  int batch, int cells, int channels_padded, int anchors, int n_classes_with_background, int mask_dim,
                                  int n_priors_total, int prior_offset);
/* The same with Detect's class scores written by the same kernel: d_scores [batch][classes][n_priors_total] (background column dropped, -1 for
 * every prior whose best class is not above `threshold`) exactly as amos_mask_class_scores_device makes them from d_conf -- one pass over the
 * softmax tensor saved, and d_conf itself may be NULL when only the detector reads the head (d_scores may be NULL instead: the plain form).
 * d_coef NULL: the layer has no coefficient channels (channels [anchors x 4 | anchors x n_classes_with_background | padding]). */
int amos_mask_head_outputs_scores_device(void *stream, const float *d_raw, const float *d_bias, float *d_loc, float *d_conf, float *d_coef, float *d_scores,
                                         float threshold, int batch, int cells, int channels_padded, int anchors, int n_classes_with_background,
                                         int mask_dim, int n_priors_total, int prior_offset);

/* Row-wise top-k, sorted descending (the per-class `scores.topk(200)` of Fast NMS, layers/functions/detection.py:103-111): d_x
 * [rows][n] -> d_values [rows][k], d_indices [rows][k] (int64, as torch.topk returns them).  Values equal torch.topk's; among equal
 * values the lower index comes first (torch leaves that order unspecified).  1 <= k <= min(256, n). */
int amos_mask_topk_rows_device(void *stream, const float *d_x, float *d_values, long long *d_indices, int rows, int n, int k);
/* The same result for rows that are mostly ONE value `fill` with everything of interest above it (the class-score rows: -1 for the priors
 * under the confidence threshold): one scan of the row instead of five -- the values above `fill` are compacted and sorted in LDS, a
 * result short of k is completed with `fill` at its first indices.  Rows that do not fit the assumption (more than 1 024 values above
 * `fill`, or values below it when the list is short of k) take the generic path inside the same launch: always amos_mask_topk_rows_device's
 * result. */
int amos_mask_topk_rows_sparse_device(void *stream, const float *d_x, float *d_values, long long *d_indices, int rows, int n, int k, float fill);

/* ---- the post-processing of the mask pass as ONE call: Detect (box decoding, per-class top 200, Fast NMS at IoU 0.5, class-confidence
 * threshold 0.05; layers/functions/detection.py:27-170, layers/box_utils.py:268-312) + postprocess / prep_display (score threshold 0.15, the
 * 15 best detections, masks = sigmoid(proto . coefficients) cropped to the box with 1 px padding, bilinear to the frame, > 0.5, the persons
 * summed, x 255 modulo 256; yolact_interface.py:678-779, 806-832) in the static-shape form of mask/detect.py detect_batch and mask/post.py
 * person_mask_batch.  Inputs (float32, device): loc [batch][P][4], conf [batch][P][classes incl. background] (softmax output), coef
 * [batch][P][mask_dim], priors [P][4], proto [batch][proto_h][proto_w][mask_dim].  Outputs: masks uint8 [batch][out_h][out_w], found uint8
 * [batch] (0: no detection above the score threshold -- the reference raises there and its caller keeps an all-zero mask).
 * d_workspace: amos_mask_post_workspace_bytes(...) bytes of device scratch (16-byte aligned).  Seven launches on `stream`. */
#define AMOS_MASK_NMS_TOP_K 200
#define AMOS_MASK_NMS_THRESH 0.5f
#define AMOS_MASK_CONF_THRESH 0.05f
#define AMOS_MASK_SCORE_THRESHOLD 0.15f
#define AMOS_MASK_TOP_K_DISPLAY 15
#define AMOS_MASK_PERSON_CLASS 0
size_t amos_mask_post_workspace_bytes(int batch, int n_priors, int n_classes_with_background, int mask_dim, int proto_h, int proto_w);
int amos_mask_person_masks_device(void *stream, const float *d_loc, const float *d_conf, const float *d_coef, const float *d_priors,
                                  const float *d_proto, int batch, int n_priors, int n_classes_with_background, int mask_dim, int proto_h,
                                  int proto_w, int out_h, int out_w, void *d_workspace, size_t workspace_bytes, uint8_t *d_masks,
                                  uint8_t *d_found);
/* The same from the class scores amos_mask_head_outputs_scores_device wrote (d_scores [batch][classes][n_priors], threshold
 * AMOS_MASK_CONF_THRESH) instead of the softmax tensor: six launches. */
int amos_mask_person_masks_scores_device(void *stream, const float *d_loc, const float *d_scores, const float *d_coef, const float *d_priors,
                                         const float *d_proto, int batch, int n_priors, int n_classes_with_background, int mask_dim, int proto_h,
                                         int proto_w, int out_h, int out_w, void *d_workspace, size_t workspace_bytes, uint8_t *d_masks,
                                         uint8_t *d_found);

/* The mask layer of the prediction head (3 x 3, cin -> anchors x mask_dim, + bias, tanh) evaluated at GIVEN priors rather than at every cell:
 * the display selection keeps at most AMOS_MASK_TOP_K_DISPLAY priors of a frame, and nothing else reads a coefficient.  The levels are the
 * head's `upfeature` outputs (after ReLU), float32 on the device: d_levels, level_h, level_w, level_blocked, level_offsets are HOST arrays of
 * n_levels (<= 8) entries, read during the call -- level i is [batch][h][w][cin] (channels-last) or, with level_blocked[i] != 0,
 * [batch][cin / 8][h][w][8]; its priors (cell-major, anchor-minor) start at level_offsets[i] = the sum of h x w x anchors over the levels
 * before it.  d_weight: the layer's weight in channels-last memory [anchors x mask_dim][3][3][cin] (16-byte aligned), d_bias [anchors x
 * mask_dim].  d_prior_idx int32 [batch][n_slots]: prior p of level l is cell (p - offset_l) / anchors, anchor (p - offset_l) % anchors; a
 * negative index (or one past the last level) is an empty slot.  d_out [batch][n_slots][mask_dim]: tanh(patch . filter[anchor x mask_dim + d]
 * + bias), zeros for empty slots.  Float32 sums in an order fixed by cin alone: either layout and every call give the same bits.
 * cin % 8 == 0, cin <= 1024; mask_dim a multiple of 8, at most 32. */
int amos_mask_coef_at_priors_device(void *stream, const float *const *d_levels, const int *level_h, const int *level_w, const int *level_blocked,
                                    const int *level_offsets, int n_levels, int cin, const float *d_weight, const float *d_bias,
                                    const int *d_prior_idx, int batch, int n_slots, int anchors, int mask_dim, float *d_out);
/* amos_mask_person_masks_device / amos_mask_person_masks_scores_device without a coefficient tensor: the display selection records its
 * priors, amos_mask_coef_at_priors_device's kernel evaluates the mask layer there (levels, weight and bias as above; the levels together
 * hold n_priors priors), the rest is unchanged.  One launch more; the head then needs no coefficient channels at all. */
int amos_mask_person_masks_at_priors_device(void *stream, const float *d_loc, const float *d_conf, const float *const *d_levels, const int *level_h,
                                            const int *level_w, const int *level_blocked, const int *level_offsets, int n_levels, int cin,
                                            int anchors, const float *d_mask_weight, const float *d_mask_bias, const float *d_priors,
                                            const float *d_proto, int batch, int n_priors, int n_classes_with_background, int mask_dim, int proto_h,
                                            int proto_w, int out_h, int out_w, void *d_workspace, size_t workspace_bytes, uint8_t *d_masks,
                                            uint8_t *d_found);
int amos_mask_person_masks_scores_at_priors_device(void *stream, const float *d_loc, const float *d_scores, const float *const *d_levels,
                                                   const int *level_h, const int *level_w, const int *level_blocked, const int *level_offsets,
                                                   int n_levels, int cin, int anchors, const float *d_mask_weight, const float *d_mask_bias,
                                                   const float *d_priors, const float *d_proto, int batch, int n_priors,
                                                   int n_classes_with_background, int mask_dim, int proto_h, int proto_w, int out_h, int out_w,
                                                   void *d_workspace, size_t workspace_bytes, uint8_t *d_masks, uint8_t *d_found);

/* ---- candidate lists: the detector's tail from the scores that can be displayed alone.  Only detections with score > AMOS_MASK_SCORE_THRESHOLD
 * are displayed, Fast NMS suppresses a box only through higher-scored boxes of its class, and a score at or under the threshold sorts behind
 * every score above it (per class and across classes, ties by index): such a score can neither be displayed nor change what is.  So the head
 * writes, instead of a softmax or class-score tensor, one list per (frame, class) of the (score, prior) pairs above the threshold, and top-k and
 * Fast NMS run over those lists.  Masks and `found` equal the dense entries' bit for bit.
 * d_candidates: amos_mask_candidates_bytes(batch, n_priors, n_classes_with_background) bytes (16-byte aligned): batch x classes int32 counters
 * (padded to 256 bytes), then batch x classes lists of n_priors 8-byte entries (score key << 32 | ~prior; only the first `count` of a list are
 * ever touched).  amos_mask_candidates_reset_device zeroes the counters (one hipMemsetAsync); it goes on a stream every level's
 * amos_mask_head_candidates_device launch is ordered behind.  The order of a list's entries depends on the run; nothing computed from it does. */
size_t amos_mask_candidates_bytes(int batch, int n_priors, int n_classes_with_background);
int amos_mask_candidates_reset_device(void *stream, void *d_candidates, int batch, int n_classes_with_background);
/* amos_mask_head_outputs_device's kernel for one level with the lists as its class output: d_loc (and d_coef unless NULL) as there, the same
 * softmax quotients, and every class c >= 1 of prior p with softmax > threshold appended to list (frame, c - 1).  One global atomic per
 * work-group and list that gains entries.  threshold: AMOS_MASK_SCORE_THRESHOLD for the entries below (any value in [0, that] gives their
 * result).  n_classes_with_background <= 257. */
int amos_mask_head_candidates_device(void *stream, const float *d_raw, const float *d_bias, float *d_loc, float *d_coef, void *d_candidates, float threshold,
                                     int batch, int cells, int channels_padded, int anchors, int n_classes_with_background, int mask_dim,
                                     int n_priors_total, int prior_offset);
/* Form of that kernel: 1 = where anchors x n_classes_with_background <= 256, a thread owns one (anchor, class) column and walks the
 * work-group's cells (default: the kernel is bound by vector instruction issue, and this form spends none on stepping indices), 0 = the
 * element loops of amos_mask_head_outputs_device.  The same d_loc and d_coef bits and the same entries in every list.  Returns the mode in
 * force before the call; any other argument only queries.  AMOS_MASK_HEAD_COLUMNS=0 / 1 in the environment is the initial value. */
int amos_mask_head_form_mode(int mode);
/* Top-k of `rows` lists of unique 8-byte entries (key << 32 | ~index, key = the order-preserving integer image of a float32 score): d_counts
 * int32 [rows], list r at d_entries + r x capacity.  d_values / d_indices [rows][k]: score descending, equal scores lowest index first; slots
 * past a list's count hold score -1 and index 0.  Independent of the order of the entries.  1 <= k <= 256. */
int amos_mask_topk_lists_device(void *stream, const int *d_counts, const unsigned long long *d_entries, int capacity, float *d_values,
                                long long *d_indices, int rows, int k);
/* amos_mask_person_masks_device / amos_mask_person_masks_at_priors_device from the lists amos_mask_head_candidates_device wrote. */
int amos_mask_person_masks_candidates_device(void *stream, const float *d_loc, const void *d_candidates, const float *d_coef, const float *d_priors,
                                             const float *d_proto, int batch, int n_priors, int n_classes_with_background, int mask_dim, int proto_h,
                                             int proto_w, int out_h, int out_w, void *d_workspace, size_t workspace_bytes, uint8_t *d_masks,
                                             uint8_t *d_found);
int amos_mask_person_masks_candidates_at_priors_device(void *stream, const float *d_loc, const void *d_candidates, const float *const *d_levels,
                                                       const int *level_h, const int *level_w, const int *level_blocked, const int *level_offsets,
                                                       int n_levels, int cin, int anchors, const float *d_mask_weight, const float *d_mask_bias,
                                                       const float *d_priors, const float *d_proto, int batch, int n_priors,
                                                       int n_classes_with_background, int mask_dim, int proto_h, int proto_w, int out_h, int out_w,
                                                       void *d_workspace, size_t workspace_bytes, uint8_t *d_masks, uint8_t *d_found);


/* ---------------------------------------------------------------- SLIC superpixels (8f-2) ---- */

/* ORB_SLAM2::center, include/cluster.h:21-30. */
typedef struct amos_slic_center {
    int32_t x, y; /* column, row */
    int32_t L, A, B, D;
    int32_t label; /* 1 .. n_centers */
    int32_t id;    /* k-means cluster, filled by the caller (cluster.cc:18-24); 0 here */
} amos_slic_center;

/* cluster::SLIC (src/cluster.cc:300-343) from the Lab image on -- initilizeCenters, fituneCenter (Sobel gradient),
 * `iterations` (5 in the reference) rounds of clustering + updateCenter with grid step `len` (5) and weight `m` (10).
 * The cv::cvtColor(image, imageLAB, COLOR_BGR2Lab) of cluster.cc:310 stays with the caller (its 8-bit path is table
 * driven inside OpenCV), as does the k-means over the centres that follows (cluster.cc:345-464).
 *   lab:    height x width x 3 uint8 (imageLAB);   depth: height x width uint16 (imD)
 *   labels: height x width float64 (labelMask / imLS: the label of the centre a pixel belongs to, 0 = none)
 *   centers: amos_slic_center_count(width, height, len) records in creation order (row-major grid) */
typedef struct amos_slic amos_slic;
int amos_slic_center_count(int width, int height, int len, int *nx, int *ny);
int amos_slic_create(int device, void *stream, int max_width, int max_height, int max_batch, amos_slic **out);
void amos_slic_destroy(amos_slic *s);
void *amos_slic_stream(amos_slic *s);
int amos_slic_run(amos_slic *s, const uint8_t *lab, const uint16_t *depth, int width, int height, int len, int m, int iterations,
              double *labels, amos_slic_center *centers, int *n_centers);
/* The same for n_frames resident frames: d_lab [n][h][w][3], d_depth [n][h][w], d_labels [n][h][w],
 * d_centers [n][center_count].  Asynchronous on the handle's stream. */
int amos_slic_batch_device(amos_slic *s, const uint8_t *d_lab, const uint16_t *d_depth, int width, int height, int n_frames,
                           int len, int m, int iterations, double *d_labels, amos_slic_center *d_centers);

/* cv::cvtColor(image, imageLAB, COLOR_BGR2Lab) of cluster::SLIC (src/cluster.cc:310), 8-bit: OpenCV 4.5's fixed-point RGB2Lab_b
 * (gamma and cube-root tables, 12-bit XYZ coefficients over the D65 white point).  Tables are built in double on the host
 * (OpenCV uses its softfloat: PARITY UNPINNED at the level of single table entries; primaries and grays match OpenCV's
 * documented values).  d_bgr / d_lab: n_pixels x 3 bytes; rgb_order != 0 for RGB input.  With amos_slic_batch_device and
 * amos_cluster_kmeans_batch_device this is the whole `cluster` constructor (cluster.cc:9-43) on the device. */
int amos_cluster_bgr2lab_batch_device(amos_slic *s, const uint8_t *d_bgr, size_t n_pixels, int rgb_order, uint8_t *d_lab);

/* cluster::randCent + cluster::kmeans (src/cluster.cc:353-460): the k-means over the SLIC centres that gives every
 * superpixel its cluster id (center::id, read by the label gate of amos_orb_gate through center_ids[label - 1]).
 * k = 15 in the reference (Frame.cc:525).  Distances as cluster::distEclud (:374-387); the loop runs until no
 * assignment changes (at most max_iter passes; *passes = -1 if the bound was hit).  The reference's undefined
 * behaviours are given a definition -- rand() becomes glibc's TYPE_0 generator (state * 1103515245 + 12345, low 31
 * bits) on the caller's seed, the one-past-the-end draw wraps to centre 0, the redraw on zero depth is bounded, the
 * uninitialised accumulator of the update step is zero -- so the result is a function of (centres, k, seed).
 * Centres must carry label = index + 1 (as amos_slic_* writes them).  d_centers: [n_frames][n_centers]. */
int amos_cluster_kmeans_batch_device(amos_slic *s, amos_slic_center *d_centers, int n_centers, int n_frames, int k,
                                     uint32_t seed, int max_iter, int32_t *d_passes /* [n_frames] or NULL */);
int amos_cluster_kmeans(amos_slic *s, amos_slic_center *centers, int n_centers, int k, uint32_t seed, int max_iter,
                        int *passes);

/* ---------------------------------------------------------------- scene flow, point arithmetic (8f-3) ---- */

/* The reference's own per-point arithmetic inside Tracking::GetSceneFlowObj (src/Tracking.cc:850-1186), between its
 * OpenCV calls (goodFeaturesToTrack, cornerSubPix, calcOpticalFlowPyrLK, findFundamentalMat, solvePnPRansac; their device
 * forms: amos_corners_*, amos_lk_*, amos_fmat_*, amos_pnp_* below).  Points are interleaved (x, y) float pairs; all pointers are device pointers; asynchronous on `stream`.
 *
 * amos_flow_check_device (:902-925): state_out[i] = 0 when either position lies within 5 px of the image edge or the
 * 3 x 3 sum of absolute gray differences between (last, pre) and (cur, next) exceeds 2520; else state_in[i].  The
 * match lists of the reference are the points with state_out != 0, in order. */
int amos_flow_check_device(void *stream, const uint8_t *d_last_gray, size_t last_stride, const uint8_t *d_cur_gray,
                           size_t cur_stride, int cols, int rows, const float *d_pre_xy, const float *d_next_xy,
                           const uint8_t *d_state_in, int n, uint8_t *d_state_out);
/* (:928-946, 1141-1152): dd[i] = |l . (next, 1)| / sqrt(l0^2 + l1^2) with l = F * (pre, 1), F row-major 3 x 3 doubles on
 * the device; -1 where d_state (may be NULL) is 0.  The reference keeps dd <= 0.5 for the second F and marks dd > 1. */
int amos_flow_epipolar_device(void *stream, const double *d_F, const float *d_pre_xy, const float *d_next_xy,
                              const uint8_t *d_state, int n, double *d_dd);
/* (:955-990, 1153-1183): per match the world point of the LAST frame's pixel (pre_3d, through mLastFrame.mTcw), of the
 * CURRENT frame's pixel (cur_3d, through mRwc / mOw), the flow norm sqrt(dx^2 + dz^2) and a validity flag (z1 > 0 &&
 * z2 > 0): out[i] = {pre_3d.xyz, cur_3d.xyz, sf_norm, valid}.  Depth maps are float32 (rows `stride` floats apart).
 * PRECONDITION: the call has no width or height and reads depth[(int)y][(int)x] unguarded, as the reference does after its border
 * check: every match position must lie inside both depth maps (what amos_flow_check_device's survivors do). */
typedef struct amos_scene_flow_camera {
    float cx, cy, invfx, invfy; /* Frame::cx, cy, invfx, invfy */
    float Tlw[12];              /* mLastFrame.mTcw, first three rows (row-major 3 x 4) */
    float Rwc[9], Ow[3];        /* mCurrentFrame.mRwc (row-major), mOw */
} amos_scene_flow_camera;
int amos_flow_scene_flow_device(void *stream, const float *d_depth_last, size_t last_stride, const float *d_depth_cur,
                                size_t cur_stride, const float *d_match_pre_xy, const float *d_match_cur_xy, int n,
                                const amos_scene_flow_camera *cam, float *d_out);
/* Hypothesis scoring for the three RANSACs of GetSceneFlowObj (Tracking.cc:927, 945: cv::findFundamentalMat(pre, cur, FM_RANSAC, 0.1, 0.99);
 * :1006: cv::solvePnPRansac(pre_3d, cur_2d, K, 0, rvec, tvec, false, 500, 0.4, 0.98, inliers, SOLVEPNP_P3P)).  For a caller that runs its own RANSAC loop
 * (the whole RANSACs: amos_fmat_* and amos_pnp_* below): the device takes what touches every point: the error of every
 * correspondence under every hypothesis (OpenCV's FMEstimatorCallback / PnPRansacCallback::computeError restated -- symmetric squared epipolar
 * distance in doubles; squared reprojection error of cv::projectPoints without distortion), the inlier test `err <= (float)(threshold^2)` and
 * the inlier count per hypothesis.  d_F: n_hypotheses x 9 doubles (row-major 3 x 3); d_Rt: n_hypotheses x 12 doubles (R row-major, then t);
 * points as float pairs / triples.  Outputs: d_inliers [n_hypotheses]; optional d_err [n_hypotheses][n] float and d_mask
 * [n_hypotheses][n] uint8 (NULL: not written).  One work-group per hypothesis, no atomics. */
int amos_flow_fundamental_score_device(void *stream, const double *d_F, int n_hypotheses, const float *d_points1_xy, const float *d_points2_xy,
                                       int n, double threshold, float *d_err, int32_t *d_inliers, uint8_t *d_mask);
int amos_flow_pnp_score_device(void *stream, const double *d_Rt, int n_hypotheses, const float *d_object_xyz, const float *d_image_xy, int n,
                               double fx, double fy, double cx, double cy, double reprojection_error, float *d_err, int32_t *d_inliers,
                               uint8_t *d_mask);

/* cv::calcOpticalFlowPyrLK(imlast, gray, prepoint, nextpoint, state, err, Size(22, 22), 5, TermCriteria(COUNT | EPS, 20, 0.01))
 * (Tracking.cc:896) on given points: pyramids of both gray frames (pyrDown, REFLECT_101 borders of the window size), Scharr
 * derivatives of the previous one, the iterative tracker from the top level down -- one wave per point.  Restated from OpenCV
 * 4.5's published algorithm; the float accumulation order is defined as the scalar path's (row by row, left to right) because
 * OpenCV's own depends on the SIMD width of its build: PARITY UNPINNED.  win_size <= 22.
 * amos_lk_levels = buildOpticalFlowPyramid's return (4 for 640 x 480: the 20 x 15 level is smaller than the window). */
typedef struct amos_lk amos_lk;
int amos_lk_create(int device, void *stream, int width, int height, int win_size, int max_level, amos_lk **out);
void amos_lk_destroy(amos_lk *k);
void *amos_lk_stream(amos_lk *k);
int amos_lk_levels(const amos_lk *k);
int amos_lk_track_device(amos_lk *k, const uint8_t *d_prev_gray, size_t prev_stride, const uint8_t *d_next_gray,
                         size_t next_stride, const float *d_prev_xy, int n, int max_count, double epsilon,
                         float min_eig_threshold, float *d_next_xy, uint8_t *d_status, float *d_err /* or NULL */);

/* The corner source of Tracking::GetSceneFlowObj (Tracking.cc:894-895), resident on the device so that the corners go into
 * amos_lk_track_device without a host round trip:
 *   cv::goodFeaturesToTrack(imlast, prepoint, 1000, 0.01, 8, cv::Mat(), 3, true, 0.04)   -> amos_corners_good_features_device
 *   cv::cornerSubPix(imlast, prepoint, Size(10, 10), Size(-1, -1), TermCriteria(ITER | EPS, 20, 0.03)) -> amos_corners_subpix_device
 * Harris detector, blockSize 3, Sobel aperture 3, no mask (what the reference passes).  d_xy receives (x, y) pairs in the library's
 * order (strongest first, equal responses: the later pixel first), d_count their number (<= max_corners, <= xy_capacity);
 * d_response (or NULL) the Harris response plane [height][width].  amos_corners_subpix_device refines d_xy in place for the first
 * *d_count points (d_count == NULL: n points); 1 <= win <= 15 and a frame of at least (2 win + 5) pixels either way, anything else
 * is AMOS_ERR_INVALID (every window of that range launches: four corners per work-group up to win 14, three at 15, whose patch and
 * products fit a CU's LDS only three times).  Restated from OpenCV 4.5's published algorithms; PARITY UNPINNED like the other
 * OpenCV-derived stages.  A frame with more than 65 536 local maxima above the quality threshold is truncated:
 * amos_corners_candidate_count (synchronising) reports AMOS_ERR_CAPACITY then.  Asynchronous on the handle's stream. */
typedef struct amos_corners amos_corners;
int amos_corners_create(int device, void *stream, int max_width, int max_height, amos_corners **out);
void amos_corners_destroy(amos_corners *c);
void *amos_corners_stream(amos_corners *c);
int amos_corners_good_features_device(amos_corners *c, const uint8_t *d_gray, size_t stride, int width, int height, int max_corners,
                                      double quality_level, double min_distance, double harris_k, float *d_xy, int xy_capacity,
                                      int *d_count, float *d_response /* or NULL */);
int amos_corners_candidate_count(amos_corners *c, int *count);
int amos_corners_subpix_device(amos_corners *c, const uint8_t *d_gray, size_t stride, int width, int height, float *d_xy,
                               const int *d_count /* or NULL */, int n, int win, int max_count, double epsilon);

/* cv::findFundamentalMat(p1, p2, FM_RANSAC, threshold, confidence) of Tracking::GetSceneFlowObj (Tracking.cc:927, 945) on the device:
 * OpenCV 4.5's classic RANSAC (cv::RNG((uint64)-1) local to the call, getSubset with 10 000 attempts and the collinearity check,
 * run7Point, FMEstimatorCallback::computeError, best model when inliers > max(best, 6), RANSACUpdateNumIters; no refit) restated
 * from the published algorithm, written from memory: PARITY WITH OPENCV UNPINNED.  The SVD, the cubic solver and the log of the
 * iteration count are replaced by + - * / sqrt constructions (amos_fmat_core.h), so the last bits differ
 * from OpenCV's; the duplicate redraw of the sampler, unbounded in OpenCV, stops after 2^20 draws of one slot (status -2).
 * One work-group per problem; a batch of problems is one launch; asynchronous on the handle's stream, no host synchronisation.
 *
 * amos_fmat_ransac_device: problem p reads the input points [d_offsets[p], d_offsets[p] + d_counts[p]) of d_p1_xy / d_p2_xy
 * ((x, y) float pairs; d_offsets NULL: p * max_points) and uses those with d_select[i] != 0 (d_select NULL: all), in order --
 * OpenCV's input list.  d_counts[p] <= max_points (else status -3).  Outputs: d_F [p][9] (row-major, F[8] = 1 or 0; zeros without
 * a model), d_status [p][4] = {result, inliers, iterations run, points used} with result 1 = model, 0 = no model (fewer than 7
 * points, or no subset passes the sampler at the first iteration), -1 = 7 <= points < 15 (OpenCV's LMeDS / 7-point branches,
 * not built: keep OpenCV there), -2 = sampler redraw cap hit, -3 = count out of range; d_mask (or NULL) indexed like the input,
 * 1 for the inliers of the returned model, 0 elsewhere and for points not selected.  threshold > 0, 0 < confidence < 1,
 * 1 <= max_iters <= 2^20 (OpenCV: 0.1, 0.99, 1000 in the reference); n_problems <= max_problems.
 *
 * amos_fmat_scene_flow_pair_device: Tracking.cc:927-945 as one call on n = *d_n tracked points (n <= max_points): F1 on the points
 * with d_state != 0; d_keep[i] = state != 0 && dd <= 0.5 under F1 (amos_flow_epipolar_device's arithmetic) -- the F_prepoint
 * selection; F2 on the kept points.  d_status [2][4] (F1, F2).  Where F1 has no model the reference would fail on F.at(); here keep
 * is all 0 and F2 is "no model" (result 0).
 *
 * amos_fmat_ransac: one problem from host pointers (n <= max_points), synchronous; mask (or NULL) [n], status [4]. */
typedef struct amos_fmat amos_fmat;
int amos_fmat_create(int device, void *stream, int max_points /* <= 4096 */, int max_problems, amos_fmat **out);
void amos_fmat_destroy(amos_fmat *h);
void *amos_fmat_stream(amos_fmat *h);
int amos_fmat_ransac_device(amos_fmat *h, int n_problems, const float *d_p1_xy, const float *d_p2_xy, const int32_t *d_offsets,
                            const int32_t *d_counts, const uint8_t *d_select, double threshold, double confidence, int max_iters,
                            double *d_F, int32_t *d_status, uint8_t *d_mask);
int amos_fmat_scene_flow_pair_device(amos_fmat *h, const float *d_pre_xy, const float *d_next_xy, const uint8_t *d_state,
                                     const int32_t *d_n, double *d_F1, double *d_F2, uint8_t *d_keep, int32_t *d_status);
int amos_fmat_ransac(amos_fmat *h, int n, const float *p1_xy, const float *p2_xy, double threshold, double confidence, int max_iters,
                     double *F, uint8_t *mask, int32_t *status);

/* cv::solvePnPRansac(obj, img, K, 0, rvec, tvec, false, max_iters, reprojection_error, confidence, inliers, SOLVEPNP_P3P) of
 * Tracking::GetSceneFlowObj (Tracking.cc:1006) on the device: OpenCV 4.5's RANSAC with 4-point samples (cv::RNG((uint64)-1) local to
 * the call, getSubset without a subset check, P3P (Gao et al.) choosing among its solutions by the 4th point, PnPRansacCallback::
 * computeError, best model when inliers > max(best, 3), RANSACUpdateNumIters(p, ep, 4, n)), then solvePnP(SOLVEPNP_EPNP) on the RANSAC
 * inliers (Lepetit et al.), restated from the published algorithms, written from memory: PARITY WITH OPENCV UNPINNED.  Every SVD, the
 * quartic and the logarithm are replaced by + - * / sqrt constructions (amos_pnp_core.h); the pose is R | t, not
 * OpenCV's R -> rvec -> R round trip.  Zero distortion.  One work-group per problem; a batch of problems is one launch; asynchronous on
 * the handle's stream, no host synchronisation.
 *
 * amos_pnp_ransac_device: problem p reads the points [d_offsets[p], d_offsets[p] + d_counts[p]) of d_object_xyz ((x, y, z) float
 * triples) and d_image_xy ((u, v) float pairs, pixels) (d_offsets NULL: p * max_points) and uses those with d_select[i] != 0
 * (d_select NULL: all), in order.  d_counts[p] <= max_points (else status -3).  Outputs: d_Rt [p][12] (R row-major, then t: the
 * layout amos_flow_pnp_score_device takes; zeros without a model); d_status [p][5] = {result, inliers, iterations run, points used,
 * refit} with result 1 = model, 0 = no model, -1 = fewer than 4 points (OpenCV asserts), -2 = sampler redraw cap hit, -3 = count out
 * of range; refit 1 = the EPnP refit on the inliers is returned, -1 = the refit was not finite and the RANSAC model is returned, 0 = no
 * refit (no model, or exactly 4 points: OpenCV's direct P3P call, all four inliers, 0 iterations); d_mask (or NULL) indexed like the
 * input: the RANSAC inliers of the returned result (OpenCV's _inliers), 0 elsewhere and for points not selected.  fx, fy > 0;
 * reprojection_error > 0, 0 < confidence < 1, 1 <= max_iters <= 2^20 (the reference: 0.4, 0.98, 500); n_problems <= max_problems.
 *
 * amos_pnp_scene_flow_device: Tracking.cc:955-1007 as one call on n = *d_n tracked points (n <= max_points): the reference's point
 * lists over the points with d_state != 0, in order -- where z1 > 0 && z2 > 0 (depth of the last frame at pre, of the current one at
 * next; a pixel outside the width x height maps counts as no depth) the entry is pre_3d (amos_flow_scene_flow_device's arithmetic)
 * -> next, elsewhere (0, 0, 0) -> (0, 0), kept in the list -- then the RANSAC with 500 iterations, 0.4 px, confidence 0.98 and
 * K = (fx, fy, cam->cx, cam->cy) (the reference's camera_mat from mK).  d_Rt [12], d_status [5], d_mask (or NULL) [n].  No host
 * synchronisation: capturable in a graph.
 *
 * amos_pnp_ransac: one problem from host pointers (n <= max_points), synchronous; Rt [12], mask (or NULL) [n], status [5]. */
typedef struct amos_pnp amos_pnp;
int amos_pnp_create(int device, void *stream, int max_points /* <= 4096 */, int max_problems, amos_pnp **out);
void amos_pnp_destroy(amos_pnp *h);
void *amos_pnp_stream(amos_pnp *h);
int amos_pnp_ransac_device(amos_pnp *h, int n_problems, const float *d_object_xyz, const float *d_image_xy, const int32_t *d_offsets,
                           const int32_t *d_counts, const uint8_t *d_select, double fx, double fy, double cx, double cy,
                           double reprojection_error, double confidence, int max_iters, double *d_Rt, int32_t *d_status, uint8_t *d_mask);
int amos_pnp_scene_flow_device(amos_pnp *h, const float *d_pre_xy, const float *d_next_xy, const uint8_t *d_state, const int32_t *d_n,
                               const float *d_depth_last, size_t last_stride, const float *d_depth_cur, size_t cur_stride, int width,
                               int height, const amos_scene_flow_camera *cam, double fx, double fy, double *d_Rt, int32_t *d_status,
                               uint8_t *d_mask);
int amos_pnp_ransac(amos_pnp *h, int n, const float *object_xyz, const float *image_xy, double fx, double fy, double cx, double cy,
                    double reprojection_error, double confidence, int max_iters, double *Rt, uint8_t *mask, int32_t *status);

/* ---------------------------------------------------------------- dynamic-object test (8f-3 tail, CalDyna) ----
 * The tail of Tracking::GetSceneFlowObj (src/Tracking.cc:1012-1184) and the decision of Frame::CalDyna (src/Frame.cc:552-628) on the
 * device, so that GetSceneFlowObj -> cluster -> decision -> labelled gate -> describe is one stream of work without a host
 * synchronisation (capturable in a graph).  Asynchronous on the handle's stream.  A handle holds max_frames result slots of
 * max_points (<= 4096) entries each.
 *
 * amos_dyna_tail_device: on n = *d_n tracked points (the lists of the reference are the points with d_state != 0, in order; N of them):
 *   z1 / z2 = depth of the last frame at (int) pre, of the current one at (int) next (outside the width x height maps: no depth);
 *   pre_3d / cur_2d = (amos_flow_scene_flow_device's pre_3d, next) where z1 > 0 && z2 > 0, else (0, 0, 0) / (0, 0) -- the PnP's lists;
 *   Mod = d_Rt (R row-major, then t: amos_pnp_scene_flow_device's output) cast to float; MotionModel = poses->motion.
 *   For every list entry with pre_3d.z > 0 && cur_2d.x != 0 && cur_2d.y != 0 (the mvMatch entries, in order): Rpe under
 *   (poses->lk if has_lk, else Mod) and under MotionModel -- cv::projectPoints evaluated with R itself (no Rodrigues round trip: the
 *   pose's floats as doubles, 1 / z or 1 where z == 0, u and v stored as float), Rpe = sqrtf(du^2 + dv^2) in float; an inlier when
 *   (double) Rpe <= 0.4.  PnP inliers >= motion-model inliers chooses Mod (choice 1; also when has_lk: the LK pose scores, Mod is the
 *   output), else MotionModel (choice 0); mvRpe is the chosen list.  Frame::SetPose: Rwc = Rcw^T, Ow = -Rcw^T tcw (double accumulation,
 *   one rounding).  mvepipolar[i] (i < n) = dd under d_F2 (amos_flow_epipolar_device's arithmetic) where state != 0, 0 elsewhere;
 *   T_M = next[i] where state != 0 && !(dd <= 1), in order.  vFlow_3d = (next.x, next.y, sf_norm) for the list entries with
 *   z1 > 0 && z2 > 0 and sf_norm > 3, sf_norm as amos_flow_scene_flow_device computes it but with the chosen Rwc / Ow.
 *   Where the PnP has no model (d_pnp_status[0] != 1; the reference fails in Rodrigues) Mod is the zeros d_Rt holds and
 *   AMOS_DYNA_NO_PNP is set: the caller keeps its host path there.  Where F2 has no model (d_fmat_status[4] != 1: amos_fmat_scene_flow_pair_device's
 *   [2][4] status) the zero F gives dd = NaN, so every tracked point is in T_M, and AMOS_DYNA_NO_F2 is set.  Camera, poses: copied at the call.
 * amos_dyna_reset_frame_device: slot `frame` holds the first frame's empty lists (GetSceneFlowObj is not called, Tracking.cc:377).
 * amos_dyna_decide_batch_device: frame f of the batch reads slot f and the labels (labelMask, doubles, frame f at d_labels +
 *   f * label_frame_stride, rows label_row_stride elements apart) and centres (d_centers + f * centers_frame_stride records, center.id
 *   the k-means cluster) of that frame.  clusterRpe: mvRpe[i] goes to cluster centers[(int) labelMask((int) y, (int) x) - 1].id of
 *   mvMatch[i]; AveClusterRpe[c] = (float sum in list order) / (float) count (an empty cluster: 0 / 0 = NaN, never removed); epNum[c]
 *   = the number of distinct superpixels holding a T_M point whose centre has id c; d_rm[f * rm_frame_stride + c] = epNum[c] > 0 &&
 *   AveClusterRpe[c] >= 3, for c < k (k <= 64).  A label of 0 or above n_centers (the reference reads centers[-1]), a point outside the map or
 *   an id outside [0, k) is skipped and flagged in the slot's decide status.
 * amos_dyna_scene_flow_obj_device: the whole of GetSceneFlowObj (Tracking.cc:894-1184) as one call on the four handles (which must share
 *   the dyna handle's stream): goodFeaturesToTrack(imlast, 1000, 0.01, 8, 3, Harris 0.04) -> cornerSubPix(10 x 10, 20, 0.03) ->
 *   calcOpticalFlowPyrLK(22 x 22, 20, 0.01) -> the SAD / border check -> the two findFundamentalMat RANSACs -> solvePnPRansac -> the
 *   tail into slot `frame`.  The working lists stay in the handle (amos_dyna_results_device); LK and the check run on all
 *   min(1000, max_points) corner slots (the unused ones zeroed), the RANSACs and the tail on the *d_n found.
 * Invalid arguments: AMOS_ERR_INVALID; create without a device: AMOS_ERR_DEVICE. */
#define AMOS_DYNA_MAX_K 64
#define AMOS_DYNA_COUNTS 6       /* N (state != 0), mvMatch, PNP_inlier, MM_inlier, T_M, vFlow_3d */
#define AMOS_DYNA_NO_PNP 1       /* tail status bits */
#define AMOS_DYNA_NO_F2 2
#define AMOS_DYNA_BAD_N 4        /* *d_n outside [0, max_points]: nothing computed, counts 0 */
#define AMOS_DYNA_RESET 8        /* amos_dyna_reset_frame_device */
#define AMOS_DYNA_BAD_MATCH_LABEL 1  /* decide status bits */
#define AMOS_DYNA_BAD_TM_LABEL 2
#define AMOS_DYNA_BAD_ID 4
typedef struct amos_dyna amos_dyna;
typedef struct amos_dyna_poses {
    float motion[12]; /* MotionModel = mVelocity * mLastFrame.mTcw (or mLastFrame.mTcw), rows of [R | t] */
    float lk[12];     /* computeMtcwUseLK's mTcw, rows of [R | t], read when has_lk != 0 */
    int32_t has_lk;
} amos_dyna_poses;
typedef struct amos_dyna_results {
    int32_t max_points, max_frames;
    float *pose;            /* [frame][12] chosen Tcw, rows of [R | t] */
    float *rwc, *ow;        /* [frame][9], [frame][3] Frame::mRwc, mOw after SetPose */
    int32_t *choice;        /* [frame] 1 = PnP (Mod), 0 = motion model */
    int32_t *counts;        /* [frame][AMOS_DYNA_COUNTS] */
    float *match_xy;        /* [frame][max_points][2] mvMatch */
    float *rpe;             /* [frame][max_points] mvRpe */
    double *epipolar;       /* [frame][max_points] mvepipolar (n entries) */
    float *tm_xy;           /* [frame][max_points][2] T_M */
    float *flow;            /* [frame][max_points][3] vFlow_3d */
    int32_t *status;        /* [frame] tail status bits */
    float *ave_rpe;         /* [frame][AMOS_DYNA_MAX_K] AveClusterRpe (k entries) */
    int32_t *ep_num;        /* [frame][AMOS_DYNA_MAX_K] epNum (k entries) */
    int32_t *decide_status; /* [frame] decide status bits */
    /* working lists of the last amos_dyna_scene_flow_obj_device call */
    float *pre_xy, *next_xy; /* [max_points][2] prepoint (sub-pixel corners), nextpoint */
    uint8_t *state;          /* [max_points] after the SAD / border check */
    int32_t *n;              /* [1] corner count */
    double *F1, *F2;         /* [9] each */
    int32_t *fmat_status;    /* [2][4] */
    double *Rt;              /* [12] */
    int32_t *pnp_status;     /* [5] */
} amos_dyna_results;
int amos_dyna_create(int device, void *stream, int max_points /* <= 4096 */, int max_frames, amos_dyna **out);
void amos_dyna_destroy(amos_dyna *h);
void *amos_dyna_stream(amos_dyna *h);
int amos_dyna_results_device(amos_dyna *h, amos_dyna_results *out);
/* Synchronous copy of `bytes` from a result array (d_src, device) to host memory on the handle's stream (callers that need a list on
 * the host, e.g. a drawer; tests). */
int amos_dyna_copy_to_host(amos_dyna *h, void *dst, const void *d_src, size_t bytes);
int amos_dyna_tail_device(amos_dyna *h, int frame, const float *d_pre_xy, const float *d_next_xy, const uint8_t *d_state, const int32_t *d_n,
                          const double *d_F2, const int32_t *d_fmat_status, const double *d_Rt, const int32_t *d_pnp_status,
                          const float *d_depth_last, size_t last_stride, const float *d_depth_cur, size_t cur_stride, int width, int height,
                          const amos_scene_flow_camera *cam, double fx, double fy, const amos_dyna_poses *poses);
int amos_dyna_reset_frame_device(amos_dyna *h, int frame);
int amos_dyna_decide_batch_device(amos_dyna *h, int n_frames, const double *d_labels, size_t label_frame_stride, size_t label_row_stride,
                                  int width, int height, const amos_slic_center *d_centers, size_t centers_frame_stride, int n_centers, int k,
                                  int32_t *d_rm, size_t rm_frame_stride);
int amos_dyna_scene_flow_obj_device(amos_dyna *h, int frame, amos_corners *corners, amos_lk *lk, amos_fmat *fmat, amos_pnp *pnp,
                                    const uint8_t *d_imlast_gray, size_t last_gray_stride, const uint8_t *d_gray, size_t gray_stride, int width,
                                    int height, const float *d_depth_last, size_t last_stride, const float *d_depth_cur, size_t cur_stride,
                                    const amos_scene_flow_camera *cam, double fx, double fy, const amos_dyna_poses *poses);

#ifdef __cplusplus
}
#endif
#endif /* AMOS_FRONTEND_H */
